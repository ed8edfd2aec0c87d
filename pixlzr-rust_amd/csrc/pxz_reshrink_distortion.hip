// pxz_reshrink_distortion.hip -- what a re-shrunk tile lost against the archive it came from
// (pxz_reshrink_distortion_varied_device): per tile, set and channel the sum over the tile's fw x fh pixels of
//   (expand(reference stored tile, expand_filter) - expand(set's stored tile, filter_up))^2,
// both expands being what varied_expand_kernel writes for that stored tile.  For an unchanged block size tile t of the image a
// .pixlzr file decodes to IS the expansion of stored tile t, so the error of rung r against "what the file decodes
// to now" needs two tile-sized images in LDS and nothing of image size anywhere.  The reference has no such function.
//
// reshrink_distortion_kernel: the tile loop of distortion_kernel (pxz_distortion.hip) -- one wave per tile, the owner search,
// the sets in the inner loop, the windows of an axis kept while the next set stores that axis at the same size, wave_sum_sgpr,
// 64-bit integer atomics into the per-image totals -- with another source.  There the source pixel is an unaligned HBM read per
// pixel and set; here it is a third LDS plane of one dword per pixel, expanded once per tile by varied_resize_tile (pxz_device.h)
// with the reference's tables, and kept across all sets.  Both expands are the shared varied_resize_tile; nothing of the resize
// arithmetic is written here.
// A wave's LDS: three planes of bw * bh dwords and the windows of both axes (reshrink_distortion_tile_dw, pxz_launch.h).  The
// reference is expanded with P0 / P1 as varied_resize_tile's planes; whichever holds the result becomes the reference plane and
// the other two serve the sets -- no copy.  The reference's windows are staged before the first set's (staged sizes start at 0),
// and at the stride of its own tables (r.wdw); the region holds the wider of the two strides.
// Conventions (those of distortion_kernel, so that the result is the composition expand + distortion):
//   reference stored at full size: its bytes are the reference (varied_resize_tile's clone: staged, no resize);
//   set tile stored at full size: zeros, its slot is not read (block.rs:279-281: it IS the reference);
//   bad stored size in a set (zero, or beyond its place): that entry all-ones, status bit 0, the image's flag, not in the totals;
//   bad reference tile: every set's entry all-ones, flagged, in no total, and nothing of the tile is read.
// The reference is expanded lazily, by the first set that needs it: a tile whose sets are all clones or bad reads no slot at all.
#include "pxz_device.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(512) reshrink_distortion_kernel(const ReshrinkDistortionArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wpb = blockDim.x / 64u, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
	// (between a phase that writes the wave's image and one that reads it)
	auto wsync = [&]() __attribute__((always_inline)) { tile_sync<1>(); };
	stage_first_tiles(lds, a.t0_dw, a.images, a.n_images);
	const uint32_t plane = a.r.bw * a.r.bh;
	uint32_t *s_p0 = lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_p1 = s_p0 + plane, *s_p2 = s_p1 + plane;
	uint32_t *s_wx = s_p2 + plane, *s_wy = s_wx + a.wdw * a.r.bw;

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the image and the tile's size
		const uint32_t lo = owner_of_tile(lds, a.t0_dw, a.images, a.n_images, t);
		const VariedImage im = a.images[lo];
		const uint32_t tl = t - im.tile0;
		const uint32_t ty = tl / im.cols, tx = tl - ty * im.cols;
		const uint32_t fw = tx + 1u == im.cols ? im.edge_w : a.r.bw, fh = ty + 1u == im.rows ? im.edge_h : a.r.bh;
		const uint32_t n = fw * fh;

		const uint32_t rw = __builtin_amdgcn_readfirstlane(a.r.tile_w[t]), rh = __builtin_amdgcn_readfirstlane(a.r.tile_h[t]);
		if (bad_stored_size(rw, rh, fw, fh, lane, a.r.status, a.image_flags, lo)) {
			// a reference that cannot be: every set's entry is all-ones, no total has the tile
			if (a.tile_sse)
				for (uint32_t e = lane; e < a.n_sets * (uint32_t)C; e += 64u)
					a.tile_sse[((size_t)(e / (uint32_t)C) * a.n_tiles + t) * (uint32_t)C + e % (uint32_t)C] = ~0ull;
			continue;
		}
		const uint32_t *ref = nullptr;           // the reference plane, once a set has needed it
		uint32_t *s_src = s_p1, *s_tmp = s_p2;   // the sets' planes: the two the reference does not hold
		uint32_t staged_tw = 0u, staged_th = 0u;  // the stored sizes whose windows s_wx / s_wy hold (0: none yet for this tile)

		for (uint32_t s = 0; s < a.n_sets; ++s) {
			const size_t idx = (size_t)s * a.n_tiles + t;
			const uint32_t tw = __builtin_amdgcn_readfirstlane(a.u.tile_w[idx]), th = __builtin_amdgcn_readfirstlane(a.u.tile_h[idx]);
			if (bad_stored_size(tw, th, fw, fh, lane, a.r.status, a.image_flags, lo)) {
				if (a.tile_sse && lane < (uint32_t)C) a.tile_sse[idx * (uint32_t)C + lane] = ~0ull;
				continue;
			}
			if (tw == fw && th == fh) {  // block.rs:279-281: the stored tile is the reference
				if (a.tile_sse && lane < (uint32_t)C) a.tile_sse[idx * (uint32_t)C + lane] = 0ull;
				continue;
			}

			// ---- 2. the reference, once: stored tile t of the archive at its full size, by its own tables
			if (ref == nullptr) {
				ref = varied_resize_tile<C>(a.r, lane, a.r.slots + (size_t)t * a.r.slot_bytes, rw, rh, fw, fh, s_p0, s_p1, s_wx, s_wy, true, true, wsync);
				s_src = ref == s_p0 ? s_p1 : s_p0;
			}

			// ---- 3. the set's stored tile at its full size
			const uint32_t *out = varied_resize_tile<C>(a.u, lane, a.u.slots + idx * a.u.slot_bytes, tw, th, fw, fh, s_src, s_tmp, s_wx, s_wy,
			                                            tw != staged_tw, th != staged_th, wsync);
			if (tw != fw) staged_tw = tw;
			if (th != fh) staged_th = th;

			// ---- 4. the squared error, pixel by pixel, both pixels from LDS.  u32 holds: a wave's three planes are in LDS beside
			// the owners' table, so a tile has fewer than 163840 / 12 < 13654 pixels; a lane sees at most 214 of them,
			// 214 * 255^2 < 2^24 per channel, and the whole tile 13654 * 255^2 < 8.88e8 < 2^32, so the sum over the wave does not
			// wrap either.
			uint32_t acc[4] = {0u, 0u, 0u, 0u};
			for (uint32_t i = lane; i < n; i += 64u) {
				const uint32_t px = ref[i], ex = out[i];
#pragma unroll
				for (uint32_t c = 0; c < (uint32_t)C; ++c) {
					const int32_t d = (int32_t)((px >> (8u * c)) & 255u) - (int32_t)((ex >> (8u * c)) & 255u);
					acc[c] += (uint32_t)(d * d);
				}
			}
			uint32_t sum[4] = {0u, 0u, 0u, 0u};
#pragma unroll
			for (uint32_t c = 0; c < (uint32_t)C; ++c) sum[c] = wave_sum_sgpr(acc[c]);
			if (lane == 0u) {
#pragma unroll
				for (uint32_t c = 0; c < (uint32_t)C; ++c) {
					if (a.tile_sse) a.tile_sse[idx * (uint32_t)C + c] = sum[c];
					if (sum[c]) atomicAdd(a.image_sse + ((size_t)s * a.n_images + lo) * (uint32_t)C + c, (unsigned long long)sum[c]);
				}
			}
			wsync();  // the next set reuses the sets' planes, the next tile all three
		}
	}
}

hipError_t launch_reshrink_distortion(const ReshrinkDistortionArgs &args, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (args.n_tiles == 0u || args.n_sets == 0u) return hipSuccess;
	ReshrinkDistortionArgs a = args;
	if (a.tile_dw == 0xffffffffu) return hipErrorInvalidValue;
	// one wave per tile, as many waves to a block as kLdsPerCu holds of their images beside the owners' first tiles
	const LaunchGeom g = varied_expand_geom(a.n_images, a.n_tiles, a.tile_dw, n_cus, &a.t0_dw);
	if (g.threads == 0u) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, g.blocks, g.threads, g.lds_bytes, stream, a); };
	return channels == 4u ? go(reshrink_distortion_kernel<4>) : go(reshrink_distortion_kernel<3>);
}

}  // namespace pxz
