// pxz_scaled_tile.h -- one stored tile at ANY target size, in an LDS image: the general form of varied_resize_tile
// (pxz_device.h) that the kernels of pxz_scaled_expand.hip run, one wave per tile.  varied_resize_tile brings a stored tile
// tw x th back to its full place fw x fh and rests on tw <= fw, th <= fh; this one brings it to nw x nh = ceil(fw / s) x
// ceil(fh / s) for a power of two s, so an axis may grow, keep its size or shrink, each on its own.
//   2. the stored pixels (tw x th at src, tightly packed) -> one dword per pixel in s_src (RGBA under a convolution
//      alpha-premultiplied as fir does), and the windows of both axis tables in s_wx / s_wy: per output sample tab.wdw dwords,
//      first | count << 16, then the weights as i16 pairs.  The tables are ScaledExpandArgs' (pxz_internal.h): entry (target
//      size, stored size) of a.dir, or of a.mixed for the axis that shrinks while the other one grows -- PixlzrBlock::resize
//      hands ONE flag, nw > tw || nh > th, to both axes (block.rs:301-304), and it picks the kernel of Triangle.
//   3. the resize of PixlzrBlock::resize (block.rs:273-334): a clone when the sizes agree, the Nearest pick, else the
//      horizontal pass (nw x th, into s_tmp) and then the vertical one (nw x nh) with i16 weights and i32 accumulators, u8
//      between the passes -- so the order is part of the result -- and un-premultiplied at the end.
// Returns the plane (s_src or s_tmp) that holds the nw x nh result, one dword per pixel, rows nw apart; wsync() has run behind
// its last write.
//
// The wave's LDS image (scaled_tile_dw, pxz_launch.h: the kernels' launch, the entry points' check and the size query all take
// it from there):
//   [s_src: bw * bh dwords] [s_tmp: bw * bh] [s_wx: win_dw] [s_wy: win_dw] [pad: bw]
// Neither pass's result exceeds a plane: nw <= fw <= bw and th <= fh <= bh.  The staged windows are sized by the taps the
// call's largest scale needs (scaled_window_dw), not by the block: a down-scaling window has up to 2 * ceil(support * s) + 1
// taps, clipped to the stored size -- 49 at 8:1 with Lanczos3 -- but there are only ceil(side / s) of them.
// Odd tap counts: the loops take two taps per v_dot2_i32_i16, and an odd window has a zero weight for the pixel read past it.
// Under down-scaling that pixel can lie behind a row's end or behind the last pixel of a full plane: the horizontal pass then
// reads at most s_src[tw * th], the first dword of s_tmp; the vertical pass reads at most nw - 1 dwords behind the nw x th
// rows it walks, which from s_src lands in s_tmp and from s_tmp in s_wx .. pad.  Every such read stays INSIDE the wave's own
// image (the pad is what guarantees it for the last wave of a block, whatever win_dw is), and its value meets a zero weight.
// Largest block: the image is 8 * bw * bh bytes and the windows, and has to fit 160 KB with the 8 KB of owners' first tiles
// beside it: 128x128 blocks fit (131 KB + 5.6 KB of windows and pad, one wave per block), 144x144 RGB blocks do not (and RGBA
// blocks above 128x128 exceed the calls' 65536-byte tile).  There is no HBM form.
#pragma once
#include "pxz_device.h"

namespace pxz {

template <int C, class Sync>
__device__ __forceinline__ const uint32_t *scaled_resize_tile(const ScaledExpandArgs &a, uint32_t lane, const uint8_t *src, uint32_t tw, uint32_t th,
                                                              uint32_t nw, uint32_t nh, uint32_t *s_src, uint32_t *s_tmp, uint32_t *s_wx, uint32_t *s_wy,
                                                              Sync wsync)
{
	const bool same = tw == nw && th == nh;
	const bool conv = a.filter != 0u && !same;

	// ---- 2. stored pixels -> one dword per pixel; the windows of both axes
	const uint32_t n = tw * th;
	for (uint32_t i = lane; i < n; i += 64u) {
		uint32_t px;
		if constexpr (C == 4) {
			px = reinterpret_cast<const uint32_t *>(src)[i];
			if (conv) px = premultiply(px);  // fir: U8x4 is alpha-premultiplied before a convolution
		} else {
			// one dword from the pixel's byte address (the slot's last pixel: from a byte earlier, shifted), as varied_resize_tile
			typedef uint32_t u32_a1 __attribute__((aligned(1)));
			if (a.slot_bytes >= 4u) {
				const uint32_t at = 3u * i + 4u <= a.slot_bytes ? 3u * i : a.slot_bytes - 4u;
				px = (*reinterpret_cast<const u32_a1 *>(src + at) >> (8u * (3u * i - at))) | 0xff000000u;
			} else {  // (1x1 blocks)
				px = (uint32_t)src[3 * i] | ((uint32_t)src[3 * i + 1] << 8) | ((uint32_t)src[3 * i + 2] << 16) | 0xff000000u;
			}
		}
		s_src[i] = px;
	}
	const bool need_h = tw != nw, need_v = th != nh;
	const bool grows = nw > tw || nh > th;  // block.rs:301-304: one flag for both axes
	ScaledTab tab_x{0, 0, 0, 0, 0, 1}, tab_y{0, 0, 0, 0, 0, 1};
	// item = (output sample, dword of its staged window): the header, or a pair of weights (zero behind the window's end)
	auto stage_windows = [&](uint32_t *wd, const ScaledTab &tab, uint32_t outs) {
		const uint32_t stride = tab.wdw;
		RowWalker rw(lane, 64u, stride);
		for (uint32_t i = lane; i < outs * stride; i += 64u, rw.next()) {
			const uint32_t o = rw.row, q = rw.col;
			const uint32_t cnt = a.filter == 0u ? 1u : a.sizes[tab.start_off + o];
			uint32_t v;
			if (q == 0u) {
				v = (uint32_t)a.starts[tab.start_off + o] | (cnt << 16);
			} else {
				const uint32_t j = 2u * (q - 1u);
				const int16_t *k = a.coeffs + tab.coeff_off + o * tab.window;
				v = (j < cnt ? (uint32_t)(uint16_t)k[j] : 0u) | (j + 1u < cnt ? (uint32_t)(uint16_t)k[j + 1u] << 16 : 0u);
			}
			wd[i] = v;
		}
	};
	if (need_h) {
		const size_t at = (size_t)a.slot[nw] * a.stride + tw;
		tab_x = tw > nw && grows ? a.mixed[at] : a.dir[at];
		stage_windows(s_wx, tab_x, nw);
	}
	if (need_v) {
		const size_t at = (size_t)a.slot[nh] * a.stride + th;
		tab_y = th > nh && grows ? a.mixed[at] : a.dir[at];
		stage_windows(s_wy, tab_y, nh);
	}
	wsync();

	// ---- 3. the resize into an image of nw x nh dwords
	const uint32_t *out = s_src;  // block.rs:279-281: clone
	if (same) {
	} else if (a.filter == 0u) {  // ResizeAlg::Nearest
		RowWalker rw(lane, 64u, nw);
		for (uint32_t i = lane; i < nw * nh; i += 64u, rw.next()) {
			const uint32_t x = need_h ? (s_wx[tab_x.wdw * rw.col] & 0xffffu) : rw.col, y = need_v ? (s_wy[tab_y.wdw * rw.row] & 0xffffu) : rw.row;
			s_tmp[i] = s_src[y * tw + x];
		}
		out = s_tmp;
		wsync();
	} else {
		if (need_h) {
			// horizontal pass: item = (ox, y) of the th stored rows
			const int prec = tab_x.precision;
			const int32_t init = 1 << (prec - 1);
			RowWalker rw(lane, 64u, nw);
			for (uint32_t i = lane; i < nw * th; i += 64u, rw.next()) {
				const uint32_t *wd = s_wx + tab_x.wdw * rw.col;
				const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
				const uint32_t *row = s_src + rw.row * tw + first;
				int32_t acc[4] = {init, init, init, init};
				// two taps per v_dot2_i32_i16 (an odd count: see the header comment)
				for (uint32_t j = 0; j < cnt; j += 2u) {
					const uint32_t w2 = wd[1u + (j >> 1)], p0 = row[j], p1 = row[j + 1u];
#pragma unroll
					for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
				}
				uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
				px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
				if (C == 4 && !need_v) px = unpremultiply(px);
				s_tmp[i] = px;
			}
			out = s_tmp;
			wsync();
		}
		if (need_v) {
			// vertical pass: item = (ox, oy); the rows it reads are nw wide (nw == tw when only this pass runs)
			const uint32_t *cur = need_h ? s_tmp : s_src;
			uint32_t *o = need_h ? s_src : s_tmp;
			const int prec = tab_y.precision;
			const int32_t init = 1 << (prec - 1);
			RowWalker rw(lane, 64u, nw);
			for (uint32_t i = lane; i < nw * nh; i += 64u, rw.next()) {
				const uint32_t *wd = s_wy + tab_y.wdw * rw.row;
				const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
				const uint32_t *col = cur + first * nw + rw.col;
				int32_t acc[4] = {init, init, init, init};
				for (uint32_t j = 0; j < cnt; j += 2u) {
					const uint32_t w2 = wd[1u + (j >> 1)], p0 = col[j * nw], p1 = col[(j + 1u) * nw];
#pragma unroll
					for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
				}
				uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
				px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
				if constexpr (C == 4) px = unpremultiply(px);
				o[i] = px;
			}
			out = o;
			wsync();
		}
	}
	return out;
}

}  // namespace pxz
