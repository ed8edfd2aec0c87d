// pxz_window.hip -- pixel windows of .pixlzr files (pxz_expand_windows_device): Pixlzr::expand (reference pixlzr.rs:77-122) +
// to_image (pixlzr_image.rs:24-74) for the tiles a set of pixel rectangles covers, each rectangle written as an image of its
// own.  The tile space is pxz_window_layout's: window k owns tiles [tile0, tile0 + ccols * crows), the tiles of its covered
// grid in row-major order.
//
// window_expand_kernel: varied_expand_kernel<C, false> (pxz_varied_expand.hip) with another fourth step -- one wave per covered
// tile, grid-stride, the wave's image (two tile-sized dword planes and the staged windows of the axis tables) in LDS, the same
// tables and the same grid.  A tile
//   1. finds its window by a binary search over the windows' first tiles (a copy of them in LDS while the call has at most
//      kVxImages windows, the table itself beyond), and from the window's entry its place in the image's grid, its full size
//      fw x fh (the block, or that image's edge) and the part [cx0, cx1) x [cy0, cy1) of it that lies inside the rectangle;
//   2., 3. is staged and resized into an LDS image of its full size by varied_resize_tile (pxz_device.h), the code
//      varied_expand_kernel runs: the whole tile, whatever part of it is wanted;
//   4. has that part written to the window's output: every row segment once, from column cx0 on -- 16 bytes per lane with
//      streaming stores where the segment starts on a dword (RGBA, output start and pitch multiples of 4), dwords at whatever
//      address they have where it does not; RGB rows as 12-byte groups of four pixels, bytes at the tail.  No form writes a
//      byte behind column cx1: the clipped edge lies in the middle of an output row, or beside another window's pixels.
// A covered tile whose stored size is zero or exceeds its place is skipped as pxz_expand_frames_device skips it (status bit
// 0, the window's flag).  There is no HBM form: a wave's image that exceeds LDS is refused by the entry point.
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
	uint32_t *s_t0 = lds;
	for (uint32_t i = threadIdx.x; i < a.t0_dw; i += blockDim.x) s_t0[i] = i < a.n_windows ? a.windows[i].tile0 : 0xffffffffu;
	__syncthreads();
	uint32_t *s_src = lds + a.t0_dw + sub * a.tile_dw;
	uint32_t *s_tmp = s_src + a.bw * a.bh;
	uint32_t *s_wx = s_tmp + a.bw * a.bh, *s_wy = s_wx + a.wdw * a.bw;

	for (uint32_t t = blockIdx.x * wpb + sub; t < a.n_tiles; t += gridDim.x * wpb) {
		// ---- 1. the window, the tile's place in the image and the part of it the window wants
		uint32_t lo = 0, hi = a.n_windows - 1u;
		while (lo < hi) {
			const uint32_t mid = (lo + hi + 1u) >> 1;
			const uint32_t t0 = a.t0_dw ? s_t0[mid] : a.windows[mid].tile0;
			if ((uint32_t)__builtin_amdgcn_readfirstlane(t0) <= t) lo = mid;
			else hi = mid - 1u;
		}
		const WindowEntry wn = a.windows[lo];
		const uint32_t tl = t - wn.tile0;
		const uint32_t cty = tl / wn.ccols, ctx = tl - cty * wn.ccols;
		const uint32_t tx = wn.c0 + ctx, ty = wn.r0 + cty;
		const uint32_t fw = tx + 1u == wn.cols ? wn.edge_w : a.bw, fh = ty + 1u == wn.rows ? wn.edge_h : a.bh;
		const uint32_t tw = __builtin_amdgcn_readfirstlane(a.tile_w[t]), th = __builtin_amdgcn_readfirstlane(a.tile_h[t]);
		if (tw == 0u || th == 0u || tw > fw || th > fh) {
			if (lane == 0u) {
				atomicOr(a.status, 1u);
				if (a.window_flags) a.window_flags[lo] = 1u;
			}
			continue;
		}
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
		const uint32_t *part = out + cy0 * fw + cx0;  // the wanted part: nh rows of nw dwords, fw apart

		// ---- 4. that part to its place, row segment by row segment: item = (row, group of four pixels)
		const uint32_t q4 = (nw + 3u) >> 2;
		typedef uint32_t u32_a1 __attribute__((aligned(1)));
		if (C == 4 && ((reinterpret_cast<uintptr_t>(dst) | wn.pitch) & 3u) == 0u) {
			typedef uint32_t u32q __attribute__((ext_vector_type(4), aligned(4)));
			RowWalker rw(lane, 64u, q4);
			for (uint32_t i = lane; i < q4 * nh; i += 64u, rw.next()) {
				const uint32_t x = 4u * rw.col;
				const uint32_t *p = part + rw.row * fw + x;
				uint8_t *d = dst + (size_t)rw.row * wn.pitch + x * 4u;
				if (x + 4u <= nw) {
					const u32q v = {p[0], p[1], p[2], p[3]};
					__builtin_nontemporal_store(v, reinterpret_cast<u32q *>(d));
				} else {
					for (uint32_t k = 0; x + k < nw; ++k) __builtin_nontemporal_store(p[k], reinterpret_cast<uint32_t *>(d) + k);
				}
			}
		} else if (C == 4) {
			// an odd offset or pitch: dwords at whatever byte address they have
			RowWalker rw(lane, 64u, nw);
			for (uint32_t i = lane; i < nw * nh; i += 64u, rw.next())
				*reinterpret_cast<u32_a1 *>(dst + (size_t)rw.row * wn.pitch + rw.col * 4u) = part[rw.row * fw + rw.col];
		} else {
			RowWalker rw(lane, 64u, q4);
			for (uint32_t i = lane; i < q4 * nh; i += 64u, rw.next()) {
				const uint32_t x = 4u * rw.col;
				const uint32_t *p = part + rw.row * fw + x;
				uint8_t *d = dst + (size_t)rw.row * wn.pitch + x * 3u;
				if (x + 4u <= nw) {
					// four pixels as twelve bytes, three dwords at whatever byte address they have: the last byte written is the
					// fourth pixel's blue, so a group that ends at cx1 ends there
					const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
					u32_a1 *o = reinterpret_cast<u32_a1 *>(d);
					o[0] = (p0 & 0xffffffu) | (p1 << 24);
					o[1] = ((p1 >> 8) & 0xffffu) | (p2 << 16);
					o[2] = ((p2 >> 16) & 0xffu) | (p3 << 8);
				} else {
					for (uint32_t k = 0; x + k < nw; ++k) {
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

hipError_t launch_window_expand(const WindowExpandArgs &args, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (args.n_tiles == 0u || args.n_windows == 0u) return hipSuccess;
	WindowExpandArgs a = args;
	const LaunchGeom g = varied_expand_geom(a.n_windows, a.n_tiles, a.tile_dw, n_cus, &a.t0_dw);  // launch_varied_expand's grid
	if (g.threads == 0u) return hipErrorInvalidValue;
	hipError_t e;
	auto go = [&](auto kernel) -> hipError_t {
		if (g.lds_bytes > 64u * 1024u &&
		    (e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes)) != hipSuccess)
			return e;
		hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, stream, a);
		return hipGetLastError();
	};
	return channels == 4u ? go(window_expand_kernel<4>) : go(window_expand_kernel<3>);
}

}  // namespace pxz
