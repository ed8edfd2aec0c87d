// pxz_varied_expand.hip -- decode side of batches of differently sized images (pxz_expand_varied_frames_device):
// Pixlzr::expand (reference pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) of every image of a varied batch in one
// launch.  The tile space is pxz_varied_layout's: image i owns tiles [tile0, tile0 + cols * rows).
//
// varied_expand_kernel: one wave per tile, grid-stride over the batch.  A tile
//   1. finds its image by owner_of_tile (pxz_device.h: a binary search over the images' first tiles, a copy of them in LDS
//      while the batch has at most kVxImages images), and from the image's entry its place: origin, pitch and the full size
//      fw x fh (the block, or that image's edge); a stored size that cannot be is skipped by bad_stored_size;
//   2., 3. is staged and resized into an LDS image of its full size by varied_resize_tile (pxz_device.h);
//   4. is written to its place by store_tile_part (pxz_device.h): the whole tile, rows fw dwords apart.
// distortion_kernel (pxz_distortion.hip) and window_expand_kernel (pxz_window.hip) are this loop with another fourth step.
// Tiles whose image (two tile-sized planes and the windows) exceeds LDS keep it in HBM, one image per wave of the grid
// (BIG: RGB blocks above 20 000 pixels), as expand_kernel<C, false, true> does.
#include "pxz_device.h"
#include "pxz_launch.h"

namespace pxz {

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
	stage_first_tiles(lds, a.t0_dw, a.images, a.n_images);
	uint32_t *s_src = BIG ? a.big_scratch + (size_t)(blockIdx.x * wpb + sub) * a.tile_dw : lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.wdw * a.bw;

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the image and the tile's place in it
		const uint32_t lo = owner_of_tile(lds, a.t0_dw, a.images, a.n_images, t);
		const VariedImage im = a.images[lo];
		const uint32_t tl = t - im.tile0;
		const uint32_t ty = tl / im.cols, tx = tl - ty * im.cols;
		const uint32_t fw = tx + 1u == im.cols ? im.edge_w : a.bw, fh = ty + 1u == im.rows ? im.edge_h : a.bh;
		const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[t]), th = __builtin_amdgcn_readfirstlane(a.tile_h[t]);
		if (bad_stored_size(tw, th, fw, fh, lane, a.status, a.image_flags, lo)) continue;
		uint8_t *dst = a.base + im.offset + (size_t)(ty * a.bh) * im.pitch + (size_t)(tx * a.bw) * (uint32_t)C;
		const uint8_t *src = a.slots + (size_t)t * a.slot_bytes;
		// ---- 2., 3. the stored pixels and the windows of both axes -> LDS; the resize into an image of fw x fh dwords
		const uint32_t *out = varied_resize_tile<C>(a, lane, src, tw, th, fw, fh, s_src, s_tmp, s_wx, s_wy, true, true, wsync);

		// ---- 4. the image to its place
		store_tile_part<C>(lane, out, fw, fw, fh, dst, im.pitch);
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
	if (a.big_waves != 0u) {
		// tile images in HBM: blocks of 4 waves, as many as the scratch holds images for
		const uint32_t wpb = 4u, blocks_max = a.big_waves / wpb, need = (a.n_tiles + wpb - 1u) / wpb;
		const uint32_t blocks = need < blocks_max ? need : blocks_max;
		if (channels == 4u) hipLaunchKernelGGL((varied_expand_kernel<4, true>), dim3(blocks), dim3(64u * wpb), a.t0_dw * 4u, stream, a);
		else hipLaunchKernelGGL((varied_expand_kernel<3, true>), dim3(blocks), dim3(64u * wpb), a.t0_dw * 4u, stream, a);
		return hipGetLastError();
	}
	if (g.threads == 0u) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, g.blocks, g.threads, g.lds_bytes, stream, a); };
	return channels == 4u ? go(varied_expand_kernel<4, false>) : go(varied_expand_kernel<3, false>);
}

}  // namespace pxz
