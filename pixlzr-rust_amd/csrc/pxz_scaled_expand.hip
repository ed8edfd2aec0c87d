// pxz_scaled_expand.hip -- decode at reduced scale (pxz_expand_varied_scaled_frames_device, pxz_expand_windows_scaled_device):
// Pixlzr::expand (reference pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) of files whose public width, height and block
// sizes were divided by s = 2^shift first -- every stored tile resized to ceil(fw / s) x ceil(fh / s) instead of its full place
// fw x fh, and written at (x0 / s, y0 / s).  The tile grids are the files' own: pxz_varied_layout's and pxz_window_layout's.
//
// scaled_expand_kernel: the tile loop of varied_expand_kernel<C, false> (pxz_varied_expand.hip) with the image's shift in step 1
//   and scaled_resize_tile (pxz_scaled_tile.h) in steps 2 and 3; step 4 is store_tile_part (pxz_device.h) as there.
// scaled_window_expand_kernel: the tile loop of window_expand_kernel (pxz_window.hip) likewise; of each covered tile it writes
//   the intersection with the window in SCALED coordinates.
// A stored size is refused only when it is zero or exceeds the FULL place (bad_stored_size); above the target it is ordinary.
// One wave per tile, the wave's image in LDS (its layout and the largest block: pxz_scaled_tile.h); there is no HBM form, a
// wave's image beyond LDS is refused by the entry points.
#include "pxz_device.h"
#include "pxz_launch.h"
#include "pxz_scaled_tile.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(512) scaled_expand_kernel(const ScaledExpandArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wpb = blockDim.x / 64u, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
	auto wsync = [&]() __attribute__((always_inline)) { tile_sync<1>(); };
	stage_first_tiles(lds, a.t0_dw, a.images, a.n_owners);
	uint32_t *s_src = lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.win_dw;

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the image, the tile's full place in it and its target
		const uint32_t lo = owner_of_tile(lds, a.t0_dw, a.images, a.n_owners, t);
		const ScaledImage im = a.images[lo];
		const uint32_t tl = t - im.tile0;
		const uint32_t ty = tl / im.cols, tx = tl - ty * im.cols;
		const uint32_t fw = tx + 1u == im.cols ? im.edge_w : a.bw, fh = ty + 1u == im.rows ? im.edge_h : a.bh;
		const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[t]), th = __builtin_amdgcn_readfirstlane(a.tile_h[t]);
		if (bad_stored_size(tw, th, fw, fh, lane, a.status, a.flags, lo)) continue;
		const uint32_t round = (1u << im.shift) - 1u;
		const uint32_t nw = (fw + round) >> im.shift, nh = (fh + round) >> im.shift;
		// (the shift divides the block: the tile's origin is exact)
		uint8_t *dst = a.base + im.offset + (size_t)(ty * (a.bh >> im.shift)) * im.pitch + (size_t)(tx * (a.bw >> im.shift)) * (uint32_t)C;
		const uint8_t *src = a.slots + (size_t)t * a.slot_bytes;
		// ---- 2., 3. the stored pixels and the windows of both axes -> LDS; the resize into an image of nw x nh dwords
		const uint32_t *out = scaled_resize_tile<C>(a, lane, src, tw, th, nw, nh, s_src, s_tmp, s_wx, s_wy, wsync);

		// ---- 4. the image to its place
		store_tile_part<C>(lane, out, nw, nw, nh, dst, im.pitch);
		wsync();  // the next tile reuses this wave's image
	}
}

template <int C>
__global__ void __launch_bounds__(512) scaled_window_expand_kernel(const ScaledExpandArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wpb = blockDim.x / 64u, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
	auto wsync = [&]() __attribute__((always_inline)) { tile_sync<1>(); };
	stage_first_tiles(lds, a.t0_dw, a.windows, a.n_owners);
	uint32_t *s_src = lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.win_dw;

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the window, the tile's full place in the image, its target and the part of that the window wants
		const uint32_t lo = owner_of_tile(lds, a.t0_dw, a.windows, a.n_owners, t);
		const ScaledWindow wn = a.windows[lo];
		const uint32_t tl = t - wn.tile0;
		const uint32_t cty = tl / wn.ccols, ctx = tl - cty * wn.ccols;
		const uint32_t tx = wn.c0 + ctx, ty = wn.r0 + cty;
		const uint32_t fw = tx + 1u == wn.cols ? wn.edge_w : a.bw, fh = ty + 1u == wn.rows ? wn.edge_h : a.bh;
		const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[t]), th = __builtin_amdgcn_readfirstlane(a.tile_h[t]);
		if (bad_stored_size(tw, th, fw, fh, lane, a.status, a.flags, lo)) continue;
		const uint32_t round = (1u << wn.shift) - 1u;
		const uint32_t nw = (fw + round) >> wn.shift, nh = (fh + round) >> wn.shift;
		// the target is [px0, px0 + nw) x [py0, py0 + nh) of the scaled image; a covered tile shares at least one scaled pixel
		// with the rectangle (its corners lie on multiples of the scale, or on the image's edge)
		const uint32_t px0 = tx * (a.bw >> wn.shift), py0 = ty * (a.bh >> wn.shift);
		const uint32_t cx0 = wn.x0 > px0 ? wn.x0 - px0 : 0u, cy0 = wn.y0 > py0 ? wn.y0 - py0 : 0u;
		const uint32_t cx1 = wn.x1 < px0 + nw ? wn.x1 - px0 : nw, cy1 = wn.y1 < py0 + nh ? wn.y1 - py0 : nh;
		uint8_t *dst = a.base + wn.offset + (size_t)(py0 + cy0 - wn.y0) * wn.pitch + (size_t)(px0 + cx0 - wn.x0) * (uint32_t)C;
		const uint8_t *src = a.slots + (size_t)t * a.slot_bytes;
		// ---- 2., 3. staged and resized whole, whatever part of it is wanted
		const uint32_t *out = scaled_resize_tile<C>(a, lane, src, tw, th, nw, nh, s_src, s_tmp, s_wx, s_wy, wsync);

		// ---- 4. the wanted part to its place: rows nw dwords apart
		store_tile_part<C>(lane, out + cy0 * nw + cx0, nw, cx1 - cx0, cy1 - cy0, dst, wn.pitch);
		wsync();  // the next tile reuses this wave's image
	}
}

hipError_t launch_scaled_expand(const ScaledExpandArgs &args, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (args.n_tiles == 0u || args.n_owners == 0u) return hipSuccess;
	ScaledExpandArgs a = args;
	const LaunchGeom g = varied_expand_geom(a.n_owners, a.n_tiles, a.tile_dw, n_cus, &a.t0_dw);  // launch_varied_expand's grid
	if (g.threads == 0u) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, g.blocks, g.threads, g.lds_bytes, stream, a); };
	if (a.windows) return channels == 4u ? go(scaled_window_expand_kernel<4>) : go(scaled_window_expand_kernel<3>);
	return channels == 4u ? go(scaled_expand_kernel<4>) : go(scaled_expand_kernel<3>);
}

}  // namespace pxz
