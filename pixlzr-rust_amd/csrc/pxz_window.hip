// pxz_window.hip -- pixel windows of .pixlzr files (pxz_expand_windows_device): Pixlzr::expand (reference pixlzr.rs:77-122) +
// to_image (pixlzr_image.rs:24-74) for the tiles a set of pixel rectangles covers, each rectangle written as an image of its
// own.  The tile space is pxz_window_layout's: window k owns tiles [tile0, tile0 + ccols * crows), the tiles of its covered
// grid in row-major order.
//
// window_expand_kernel: the tile loop of varied_expand_kernel<C, false> (pxz_varied_expand.hip; steps 1 to 3, the grid and the
// tables are described there) over the windows' table, with a clipped fourth step.  A tile
//   1. finds its window, and from the window's entry its place in the image's grid, its full size fw x fh (the block, or
//      that image's edge) and the part [cx0, cx1) x [cy0, cy1) of it that lies inside the rectangle; a covered tile whose
//      stored size is zero or exceeds its place is skipped (bad_stored_size: status bit 0, the window's flag);
//   2., 3. is staged and resized whole, whatever part of it is wanted;
//   4. has that part written to the window's output by store_tile_part (pxz_device.h), which writes no byte behind column
//      cx1: the clipped edge lies in the middle of an output row, or beside another window's pixels.
// There is no HBM form: a wave's image that exceeds LDS is refused by the entry point.
#include "pxz_device.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(512) window_expand_kernel(const WindowExpandArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const uint32_t wpb = blockDim.x / 64u, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
	// (between a phase that writes the wave's image and one that reads it)
	auto wsync = [&]() __attribute__((always_inline)) { tile_sync<1>(); };
	stage_first_tiles(lds, a.t0_dw, a.windows, a.n_windows);
	uint32_t *s_src = lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.wdw * a.bw;

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the window, the tile's place in the image and the part of it the window wants
		const uint32_t lo = owner_of_tile(lds, a.t0_dw, a.windows, a.n_windows, t);
		const WindowEntry wn = a.windows[lo];
		const uint32_t tl = t - wn.tile0;
		const uint32_t cty = tl / wn.ccols, ctx = tl - cty * wn.ccols;
		const uint32_t tx = wn.c0 + ctx, ty = wn.r0 + cty;
		const uint32_t fw = tx + 1u == wn.cols ? wn.edge_w : a.bw, fh = ty + 1u == wn.rows ? wn.edge_h : a.bh;
		const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[t]), th = __builtin_amdgcn_readfirstlane(a.tile_h[t]);
		if (bad_stored_size(tw, th, fw, fh, lane, a.status, a.window_flags, lo)) continue;
		// the tile is [px0, px0 + fw) x [py0, py0 + fh) of the image; a covered tile shares at least one pixel with the rectangle
		const uint32_t px0 = tx * a.bw, py0 = ty * a.bh;
		const uint32_t cx0 = wn.x > px0 ? wn.x - px0 : 0u, cy0 = wn.y > py0 ? wn.y - py0 : 0u;
		const uint32_t cx1 = wn.x + wn.w < px0 + fw ? wn.x + wn.w - px0 : fw, cy1 = wn.y + wn.h < py0 + fh ? wn.y + wn.h - py0 : fh;
		const uint32_t nw = cx1 - cx0, nh = cy1 - cy0;
		// where pixel (cx0, cy0) of the tile goes: row py0 + cy0 - y, column px0 + cx0 - x of the window's output
		uint8_t *dst = a.base + wn.offset + (size_t)(py0 + cy0 - wn.y) * wn.pitch + (size_t)(px0 + cx0 - wn.x) * (uint32_t)C;
		const uint8_t *src = a.slots + (size_t)t * a.slot_bytes;
		// ---- 2., 3. the stored pixels and the windows of both axes -> LDS; the resize into an image of fw x fh dwords
		const uint32_t *out = varied_resize_tile<C>(a, lane, src, tw, th, fw, fh, s_src, s_tmp, s_wx, s_wy, true, true, wsync);

		// ---- 4. the wanted part to its place: nh rows of nw dwords, fw apart
		store_tile_part<C>(lane, out + cy0 * fw + cx0, fw, nw, nh, dst, wn.pitch);
		wsync();  // the next tile reuses this wave's image
	}
}

hipError_t launch_window_expand(const WindowExpandArgs &args, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (args.n_tiles == 0u || args.n_windows == 0u) return hipSuccess;
	WindowExpandArgs a = args;
	const LaunchGeom g = varied_expand_geom(a.n_windows, a.n_tiles, a.tile_dw, n_cus, &a.t0_dw);  // launch_varied_expand's grid
	if (g.threads == 0u) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, g.blocks, g.threads, g.lds_bytes, stream, a); };
	return channels == 4u ? go(window_expand_kernel<4>) : go(window_expand_kernel<3>);
}

}  // namespace pxz
