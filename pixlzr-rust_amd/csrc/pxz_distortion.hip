// pxz_distortion.hip -- what a stored tile lost (pxz_distortion_frames_device, pxz_distortion_varied_frames_device): per tile
// and channel the sum over the tile's pixels of (source - expanded)^2, where `expanded` is what Pixlzr::expand (reference
// pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) would put in the tile's place -- what varied_expand_kernel writes -- and
// `source` is the image the tile was shrunk from.  The expanded image is never written anywhere.  The reference has no such
// function: src/bin/whole-folder.rs:69-117 writes the PNG that comes back and leaves the comparison to a person.
//
// distortion_kernel: the tile loop of varied_expand_kernel<C, false> (pxz_varied_expand.hip; steps 1 to 3, the grid and the
// tables are described there) with another fourth step.  A tile
//   1. finds its image and its place (its own copy of owner_of_tile and bad_stored_size, pxz_device.h: with the shared forms and
//      the shared argument block this kernel measured 1.0-1.5 % slower);
//   2., 3. is staged and resized;
//   4. is compared: the lanes walk the full tile, read the source pixel at its place in the image (any pitch, any byte
//      alignment) and add (source - expanded)^2 per channel; the wave's sums go to the tile's entries and, by 64-bit integer
//      atomics, to the image's totals -- integer sums, so the order of the atomics does not show.
// Sets: the call holds n_sets stored versions of every tile (the rungs of a factor ladder).  A wave takes its tile through all
// sets before it moves on, so that the source tile's second and later reads come from L2, and the windows of an axis stay in
// LDS while the next set stores that axis at the same size.
// Clones: a tile stored at its full size IS the source (block.rs:279-281): zeros, and neither its slot nor the source is read.
// A tile whose stored size is zero or exceeds its place is skipped as pxz_expand_frames_device skips it (status bit 0, the
// image's flag); its entries are all-ones and the totals leave it out.
// There is no HBM form: a wave's image that exceeds LDS is refused by the entry points.
#include "pxz_device.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(512) distortion_kernel(const DistortionArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wpb = blockDim.x / 64u, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
	// (between a phase that writes the wave's image and one that reads it)
	auto wsync = [&]() __attribute__((always_inline)) { tile_sync<1>(); };
	uint32_t *s_t0 = lds;
	for (uint32_t i = threadIdx.x; i < a.t0_dw; i += blockDim.x) s_t0[i] = i < a.n_images ? a.images[i].tile0 : 0xffffffffu;
	__syncthreads();
	uint32_t *s_src = lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.wdw * a.bw;
	typedef uint32_t u32_a1 __attribute__((aligned(1)));

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the image and the tile's place in it
		uint32_t lo = 0, hi = a.n_images - 1u;
		while (lo < hi) {
			const uint32_t mid = (lo + hi + 1u) >> 1;
			const uint32_t t0 = a.t0_dw ? s_t0[mid] : a.images[mid].tile0;
			if ((uint32_t)__builtin_amdgcn_readfirstlane(t0) <= t) lo = mid;
			else hi = mid - 1u;
		}
		const VariedImage im = a.images[lo];
		const uint32_t tl = t - im.tile0;
		const uint32_t ty = tl / im.cols, tx = tl - ty * im.cols;
		const uint32_t fw = tx + 1u == im.cols ? im.edge_w : a.bw, fh = ty + 1u == im.rows ? im.edge_h : a.bh;
		const uint8_t *origin = a.base + im.offset + (size_t)(ty * a.bh) * im.pitch + (size_t)(tx * a.bw) * (uint32_t)C;
		// the image's last column: the dword read of an RGB pixel would end a byte behind the row
		const bool row_end = tx + 1u == im.cols;
		uint32_t staged_tw = 0u, staged_th = 0u;  // the stored sizes whose windows s_wx / s_wy hold (0: none yet for this tile)

		for (uint32_t s = 0; s < a.n_sets; ++s) {
			const size_t idx = (size_t)s * a.n_tiles + t;
			const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[idx]), th = __builtin_amdgcn_readfirstlane(a.tile_h[idx]);
			if (tw == 0u || th == 0u || tw > fw || th > fh) {
				if (lane == 0u) {
					atomicOr(a.status, 1u);
					if (a.image_flags) a.image_flags[lo] = 1u;
				}
				if (a.tile_sse && lane < (uint32_t)C) a.tile_sse[idx * (uint32_t)C + lane] = ~0ull;
				continue;
			}
			if (tw == fw && th == fh) {  // block.rs:279-281: the stored tile is the source
				if (a.tile_sse && lane < (uint32_t)C) a.tile_sse[idx * (uint32_t)C + lane] = 0ull;
				continue;
			}

			// ---- 2., 3. the stored pixels and the windows of both axes -> LDS; the resize into an image of fw x fh dwords
			const uint32_t *out = varied_resize_tile<C>(a, lane, a.slots + idx * a.slot_bytes, tw, th, fw, fh, s_src, s_tmp, s_wx, s_wy,
			                                            tw != staged_tw, th != staged_th, wsync);
			if (tw != fw) staged_tw = tw;
			if (th != fh) staged_th = th;

			// ---- 4. the squared error against the source, pixel by pixel.  u32 holds: a wave's image is in LDS, so a tile has fewer
			// than 163840 / 8 = 20480 pixels; a lane sees at most 320 of them, 320 * 255^2 < 2^25 per channel, and the whole tile
			// 20480 * 255^2 < 1.34e9 < 2^32, so the sum over the wave does not wrap either.
			uint32_t acc[4] = {0u, 0u, 0u, 0u};
			RowWalker rw(lane, 64u, fw);
			for (uint32_t i = lane; i < fw * fh; i += 64u, rw.next()) {
				const uint8_t *p = origin + (size_t)rw.row * im.pitch + rw.col * (uint32_t)C;
				uint32_t px;
				if constexpr (C == 4) {
					px = *reinterpret_cast<const u32_a1 *>(p);  // a dword at whatever byte address it has
				} else if (!(row_end && rw.col + 1u == fw)) {
					px = *reinterpret_cast<const u32_a1 *>(p);  // (the fourth byte is the next pixel's red)
				} else if (im.width >= 2u) {
					px = *reinterpret_cast<const u32_a1 *>(p - 1) >> 8;  // the row's last pixel: from a byte earlier, shifted
				} else {  // (images one pixel wide)
					px = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
				}
				const uint32_t ex = out[i];
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
			wsync();  // the next set, or the next tile, reuses this wave's image
		}
	}
}

hipError_t launch_distortion(const DistortionArgs &args, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (args.n_tiles == 0u || args.n_sets == 0u) return hipSuccess;
	DistortionArgs a = args;
	const LaunchGeom g = varied_expand_geom(a.n_images, a.n_tiles, a.tile_dw, n_cus, &a.t0_dw);  // launch_varied_expand's grid
	if (g.threads == 0u) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, g.blocks, g.threads, g.lds_bytes, stream, a); };
	return channels == 4u ? go(distortion_kernel<4>) : go(distortion_kernel<3>);
}

}  // namespace pxz
