// pxz_varied_expand.hip -- decode side of batches of differently sized images (pxz_expand_varied_frames_device):
// Pixlzr::expand (reference pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) of every image of a varied batch in one
// launch.  The tile space is pxz_varied_layout's: image i owns tiles [tile0, tile0 + cols * rows).
//
// varied_expand_kernel: one wave per tile, grid-stride over the batch.  A tile
//   1. finds its image by a binary search over the images' first tiles (a copy of them in LDS while the batch has at most
//      kVxImages images, the per-image table itself beyond), and from the image's entry its place: origin, pitch and the full
//      size fw x fh (the block, or that image's edge);
//   2. stages its stored pixels (tw x th, one dword per pixel; RGBA under a convolution alpha-premultiplied as fir does) and
//      the windows of its two axis tables -- directory entry (full size, stored size), one table for both axes -- in LDS;
//   3. is resized as PixlzrBlock::resize does (block.rs:273-334): a clone when the sizes agree, the Nearest pick, else the
//      horizontal then the vertical pass with i16 weights and i32 accumulators, u8 between the passes, un-premultiplied at
//      the end -- expand_kernel's general form, the same arithmetic term for term -- into an LDS image of the full tile;
//   4. is written to its place: every row segment once, 16 bytes per lane with streaming stores where the segment starts on
//      a dword (any image whose offset and pitch are multiples of 4), pixel by pixel where an odd offset or pitch puts it
//      elsewhere; RGB rows as 12-byte groups of four pixels.
// Steps 2 and 3 are varied_resize_tile (pxz_device.h), which distortion_kernel (pxz_distortion.hip) runs too.
// Tiles whose image (two tile-sized planes and the windows) exceeds LDS keep it in HBM, one image per wave of the grid
// (BIG: RGB blocks above 20 000 pixels), as expand_kernel<C, false, true> does.
#include "pxz_device.h"
#include "pxz_launch.h"

namespace pxz {

constexpr uint32_t kVxImages = 2048;  // images whose first tiles a block keeps in LDS (8 KB)

template <int C, bool BIG>
__global__ void __launch_bounds__(512) varied_expand_kernel(const VariedExpandArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wpb = blockDim.x / 64u, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
	// (between a phase that writes the wave's image and one that reads it)
	auto wsync = [&]() __attribute__((always_inline)) {
		if constexpr (BIG) {
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the wave's stores to its image have landed
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
		} else {
			tile_sync<1>();
		}
	};
	uint32_t *s_t0 = lds;
	for (uint32_t i = threadIdx.x; i < a.t0_dw; i += blockDim.x) s_t0[i] = i < a.n_images ? a.images[i].tile0 : 0xffffffffu;
	__syncthreads();
	uint32_t *s_src = BIG ? a.big_scratch + (size_t)(blockIdx.x * wpb + sub) * a.tile_dw : lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.wdw * a.bw;

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
		const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[t]), th = __builtin_amdgcn_readfirstlane(a.tile_h[t]);
		if (tw == 0u || th == 0u || tw > fw || th > fh) {
			if (lane == 0u) {
				atomicOr(a.status, 1u);
				if (a.image_flags) a.image_flags[lo] = 1u;
			}
			continue;
		}
		uint8_t *dst = a.base + im.offset + (size_t)(ty * a.bh) * im.pitch + (size_t)(tx * a.bw) * (uint32_t)C;
		const uint8_t *src = a.slots + (size_t)t * a.slot_bytes;
		// ---- 2., 3. the stored pixels and the windows of both axes -> LDS; the resize into an image of fw x fh dwords
		const uint32_t *out = varied_resize_tile<C>(a, lane, src, tw, th, fw, fh, s_src, s_tmp, s_wx, s_wy, true, true, wsync);

		// ---- 4. the image to its place, row segment by row segment: item = (row, group of four pixels)
		const uint32_t q4 = (fw + 3u) >> 2;
		typedef uint32_t u32_a1 __attribute__((aligned(1)));
		if (C == 4 && ((reinterpret_cast<uintptr_t>(dst) | im.pitch) & 3u) == 0u) {
			typedef uint32_t u32q __attribute__((ext_vector_type(4), aligned(4)));
			RowWalker rw(lane, 64u, q4);
			for (uint32_t i = lane; i < q4 * fh; i += 64u, rw.next()) {
				const uint32_t x = 4u * rw.col;
				const uint32_t *p = out + rw.row * fw + x;
				uint8_t *d = dst + (size_t)rw.row * im.pitch + x * 4u;
				if (x + 4u <= fw) {
					const u32q v = {p[0], p[1], p[2], p[3]};
					__builtin_nontemporal_store(v, reinterpret_cast<u32q *>(d));
				} else {
					for (uint32_t k = 0; x + k < fw; ++k) __builtin_nontemporal_store(p[k], reinterpret_cast<uint32_t *>(d) + k);
				}
			}
		} else if (C == 4) {
			// an odd offset or pitch: dwords at whatever byte address they have
			RowWalker rw(lane, 64u, fw);
			for (uint32_t i = lane; i < fw * fh; i += 64u, rw.next())
				*reinterpret_cast<u32_a1 *>(dst + (size_t)rw.row * im.pitch + rw.col * 4u) = out[i];
		} else {
			RowWalker rw(lane, 64u, q4);
			for (uint32_t i = lane; i < q4 * fh; i += 64u, rw.next()) {
				const uint32_t x = 4u * rw.col;
				const uint32_t *p = out + rw.row * fw + x;
				uint8_t *d = dst + (size_t)rw.row * im.pitch + x * 3u;
				if (x + 4u <= fw) {
					// four pixels as twelve bytes, three dwords at whatever byte address they have
					const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
					u32_a1 *o = reinterpret_cast<u32_a1 *>(d);
					o[0] = (p0 & 0xffffffu) | (p1 << 24);
					o[1] = ((p1 >> 8) & 0xffffu) | (p2 << 16);
					o[2] = ((p2 >> 16) & 0xffu) | (p3 << 8);
				} else {
					for (uint32_t k = 0; x + k < fw; ++k) {
						const uint32_t px = p[k];
						d[3u * k] = (uint8_t)px;
						d[3u * k + 1u] = (uint8_t)(px >> 8);
						d[3u * k + 2u] = (uint8_t)(px >> 16);
					}
				}
			}
		}
		wsync();  // the next tile reuses this wave's image
	}
}

// LDS dwords of one wave's image: the stored pixels and the other plane (bw * bh each), then the staged windows
uint32_t varied_expand_tile_dw(uint32_t bw, uint32_t bh, uint32_t wdw) { return (2u * bw * bh + wdw * (bw + bh) + 3u) & ~3u; }

LaunchGeom varied_expand_geom(uint32_t n_images, uint32_t n_tiles, uint32_t tile_dw, uint32_t n_cus, uint32_t *t0_dw)
{
	constexpr uint32_t kLds = 160u * 1024u;
	*t0_dw = n_images <= kVxImages ? (n_images + 3u) & ~3u : 0u;
	const uint32_t tile_bytes = tile_dw * 4u;
	uint32_t wpb = (kLds - *t0_dw * 4u) / tile_bytes;
	if (wpb > 8u) wpb = 8u;
	if (wpb < 1u) return LaunchGeom{0u, 0u, 0u};
	const uint32_t lds_bytes = *t0_dw * 4u + wpb * tile_bytes;
	uint32_t per_cu = kLds / lds_bytes;
	per_cu = per_cu < 1u ? 1u : (per_cu > 4u ? 4u : per_cu);
	// (a few waves' worth of tiles per wave: the tiles of a batch differ in cost, the grid-stride loop evens them out)
	const uint64_t need = ((uint64_t)n_tiles + wpb - 1u) / wpb, cap = (uint64_t)n_cus * per_cu * 4u;
	return LaunchGeom{(uint32_t)(need < cap ? need : cap), 64u * wpb, lds_bytes};
}

hipError_t launch_varied_expand(const VariedExpandArgs &args, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (args.n_tiles == 0u) return hipSuccess;
	VariedExpandArgs a = args;
	const LaunchGeom g = varied_expand_geom(a.n_images, a.n_tiles, a.tile_dw, n_cus, &a.t0_dw);
	hipError_t e;
	if (a.big_waves != 0u) {
		// tile images in HBM: blocks of 4 waves, as many as the scratch holds images for
		const uint32_t wpb = 4u, blocks_max = a.big_waves / wpb, need = (a.n_tiles + wpb - 1u) / wpb;
		const uint32_t blocks = need < blocks_max ? need : blocks_max;
		if (channels == 4u) hipLaunchKernelGGL((varied_expand_kernel<4, true>), dim3(blocks), dim3(64u * wpb), a.t0_dw * 4u, stream, a);
		else hipLaunchKernelGGL((varied_expand_kernel<3, true>), dim3(blocks), dim3(64u * wpb), a.t0_dw * 4u, stream, a);
		return hipGetLastError();
	}
	if (g.threads == 0u) return hipErrorInvalidValue;
	auto go = [&](auto kernel) -> hipError_t {
		if (g.lds_bytes > 64u * 1024u &&
		    (e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes)) != hipSuccess)
			return e;
		hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, stream, a);
		return hipGetLastError();
	};
	return channels == 4u ? go(varied_expand_kernel<4, false>) : go(varied_expand_kernel<3, false>);
}

}  // namespace pxz
