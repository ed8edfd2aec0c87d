// pxz_reshrink_ladder.hip -- stored tiles of a varied batch shrunk again at several factors in one launch
// (pxz_reshrink_varied_ladder_frames_device): reshrink_kernel (pxz_reshrink.hip) up to the detector's raw result, then
// varied_ladder_kernel (pxz_varied_ladder.hip) from the rungs' decisions on.  The expand and the detector do not depend on the
// factor, so a stored tile is expanded once and measured once; each rung only decides its levels, and the tile is resampled once
// per distinct pair of levels among its rungs.
//
// reshrink_ladder_kernel: one tile per block of 256 threads, grid-stride over the flat tile space of pxz_varied_layout, owners by
// owner_of (pxz_device.h), the grid sized as launch_varied sizes it.  A tile
//   1. reads      its stored size (tw, th) and, from its owner's grid, its full size (fw, fh);
//   2. is flagged and skipped when its stored size cannot be (zero, or beyond its place), as reshrink_kernel does it: status bit
//                 0, the image's flag, and for EVERY rung outputs 0 x 0 with value bits 0; every rung's slot is left as it was;
//   3. is cloned in when it is stored at full size, or
//   4. is expanded otherwise: steps 3 and 4 of reshrink_kernel, COPIED UNCHANGED -- A FIX TO THE ARITHMETIC THERE (or in
//                 varied_resize_tile, pxz_device.h) BELONGS HERE TOO, and the other way round.  RGB is packed to 3 bytes, so that
//                 what follows reads the tile image varied_ladder_kernel reads.  X is the plane the result lies in;
//   5. is measured once: x = total / count, or the two integer sums (varied_oklab_raw, varied_sobel_sums: pxz_varied_tile.h);
//   6. is decided per rung, by thread r for rung r: value and sizes go to index r * n_tiles + tile, the pair of levels that shrink
//                 to LDS; cloned to the slot of every rung that keeps both sizes, before the premultiply; premultiplied once, in
//                 place, and only if some rung shrinks; resampled once per distinct pair of levels (X -> I -> F, or X -> A alone)
//                 and stored to every rung with that pair: steps 3 to 6 of varied_ladder_kernel, with varied_pass and
//                 varied_store of pxz_varied_tile.h.
// X is never written after the premultiply, so it serves every pair.  In place: tile t's stored size and slot are read only by
// the block of tile t, into registers and LDS and before its first store (barriers lie between), and rungs of 1 and above lie
// beyond the inputs, so rung 0 of out_w / out_h / out_px may be the input arrays.
//
// LDS of one block (reshrink_ladder_lds):
//   [oklab tables, shrink_by only: 14 336 B] [P0: plane] [P1: plane] [windows of both axes: (bw + bh) * wdw dwords] [A, if own]
// A plane is bw * bh dwords, as in reshrink_kernel.  After the expand X is P0 or P1 (which one depends on the tile) and the other
// plane is free; it serves as A: the detector's planes [4][kVariedChunk], then the passes' I at its start and F behind I
// (varied_ladder_lds' sizes for the tile's channel count).  A does not always fit one plane -- shrink_by's detector takes 16 KB
// whatever the block, and a 3x5 RGBA block has a plane of 64 B and I + F of 48 + 32 B -- so the layout function compares the two
// and gives A a region of its own behind the windows when the plane is too small.  At 128x128 RGBA: 14 KB + 64 KB + 64 KB + 5 KB,
// I + F = 48 KB inside the free plane.  The call's limit is the re-shrink's: block_w * block_h * 4 <= 65536 for RGB and RGBA.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

constexpr uint32_t kReshrinkLadderMaxPlaneBytes = 65536;

// Where a block of reshrink_ladder_kernel keeps its images: byte offsets into its dynamic LDS, and their sum (0xffffffff: a plane
// beyond the call's limit).  The kernel, its launcher and the host's limit check all take the layout from here.
struct ReshrinkLadderLds {
	uint32_t p0, p1, wx;  // the two planes and the staged windows
	uint32_t own;         // A's own region, or 0: A is the plane the expand leaves free
	uint32_t f;           // F, from the start of A (= the room of I)
	uint32_t total;
};

__host__ __device__ inline ReshrinkLadderLds reshrink_ladder_lds(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t channels, uint32_t wdw)
{
	auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
	ReshrinkLadderLds l{0, 0, 0, 0, 0, 0xffffffffu};
	const uint64_t plane64 = ((uint64_t)bw * bh * 4u + 15u) & ~(uint64_t)15u;
	if (bw == 0u || bh == 0u || plane64 > kReshrinkLadderMaxPlaneBytes) return l;
	const uint32_t plane = (uint32_t)plane64;
	// A: the widest horizontal result I and the result F behind it, or a vertical-only result (varied_ladder_lds)
	const uint32_t hw = bw > 1u ? (bw + 1u) / 2u : 0u, hh = bh > 1u ? (bh + 1u) / 2u : 0u;
	const uint32_t i_bytes = up16(hw * bh * channels);
	const uint32_t hv = i_bytes + up16(hw * hh * channels), v_only = up16(bw * hh * channels);
	uint32_t a_bytes = hv > v_only ? hv : v_only;
	if (mode == 0u && a_bytes < kVariedPlaneBytes) a_bytes = kVariedPlaneBytes;  // the detector's planes
	l.p0 = mode == 0u ? kVariedTables * 4u : 0u;
	l.p1 = l.p0 + plane;
	l.wx = l.p1 + plane;
	const uint32_t after = l.wx + (((bw + bh) * wdw + 3u) & ~3u) * 4u;
	l.own = a_bytes > plane ? after : 0u;
	l.f = i_bytes;
	l.total = a_bytes > plane ? after + a_bytes : after;
	return l;
}

template <int C>
__global__ void __launch_bounds__(kVariedThreads) reshrink_ladder_kernel(const ReshrinkLadderArgs la)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	__shared__ uint32_t s_key[kVariedLadderMaxRungs];  // per rung: mx | my << 8 of the axes that shrink (0: a clone)
	const VariedArgs &a = la.r.v;
	const TileResizeArgs &x = la.r.x;
	const uint32_t tid = threadIdx.x, n_rungs = la.n_factors;
	const bool oklab = a.mode == 0u;
	const bool nearest = a.filter == 0u;
	const ReshrinkLadderLds l = reshrink_ladder_lds(a.mode, a.bw, a.bh, (uint32_t)C, x.wdw);
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint8_t *s_p0 = reinterpret_cast<uint8_t *>(lds) + l.p0;
	uint8_t *s_p1 = reinterpret_cast<uint8_t *>(lds) + l.p1;
	uint32_t *s_wx = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(lds) + l.wx), *s_wy = s_wx + x.wdw * a.bw;
	if (oklab) {
		oklab_fill_tables(s_lms, s_alpha, s_scale, tid);
		__syncthreads();
	}

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		// ---- 1. the tile's owner, its full size and its stored size
		const uint32_t owner = owner_of(a.images, a.n_images, tile_g, &VariedImage::tile0);
		const VariedImage im = a.images[owner];
		const uint32_t t = tile_g - im.tile0;
		const uint32_t ty = t / im.cols, tx = t - ty * im.cols;
		const uint32_t w = tx + 1u == im.cols ? im.edge_w : a.bw;  // split.rs:18
		const uint32_t h = ty + 1u == im.rows ? im.edge_h : a.bh;  // split.rs:19
		const uint32_t n = w * h;
		const uint32_t tw = x.tile_w[tile_g], th = x.tile_h[tile_g];
		const uint8_t *src = x.slots + (size_t)tile_g * x.slot_bytes;

		// ---- 2. a stored size that cannot be (bad_stored_size, pxz_device.h): flagged, empty at every rung, every slot left alone
		if (tw == 0u || th == 0u || tw > w || th > h) {
			if (tid == 0u) {
				atomicOr(x.status, 1u);
				if (la.r.image_flags) la.r.image_flags[owner] = 1u;
			}
			if (tid < n_rungs) {
				const size_t at = (size_t)tid * a.n_tiles + tile_g;
				a.value[at] = 0.0f;
				a.out_w[at] = 0u;
				a.out_h[at] = 0u;
			}
			continue;
		}

		uint8_t *s_x, *s_o;  // the tile image X, tightly packed, and the plane the expand leaves free
		if (tw == w && th == h) {
			// ---- 3. clone in: the slot's bytes are the tile image (as varied_kernel stages a tile whose pitch is one row)
			const uint32_t bytes = n * (uint32_t)C;
			uint32_t head = 0;
			if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
				head = bytes & ~15u;
				uint4 *d = reinterpret_cast<uint4 *>(s_p0);
				for (uint32_t i = tid; i < head / 16u; i += kVariedThreads) d[i] = reinterpret_cast<const uint4 *>(src)[i];
			} else if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0u) {
				head = bytes & ~3u;
				uint32_t *d = reinterpret_cast<uint32_t *>(s_p0);
				for (uint32_t i = tid; i < head / 4u; i += kVariedThreads) d[i] = reinterpret_cast<const uint32_t *>(src)[i];
			}
			for (uint32_t i = head + tid; i < bytes; i += kVariedThreads) s_p0[i] = src[i];
			s_x = s_p0;
			s_o = s_p1;
			__syncthreads();
		} else {
			// ---- 4. expand: varied_resize_tile (pxz_device.h) by the whole block.  Stored pixels -> one dword per pixel in P0
			// (RGBA under a convolution alpha-premultiplied as fir does); the windows of both axis tables -- directory entry
			// (full size, stored size) -- per output sample wdw dwords: first | count << 16, then the weights as i16 pairs
			uint32_t *s_src = reinterpret_cast<uint32_t *>(s_p0), *s_tmp = reinterpret_cast<uint32_t *>(s_p1);
			const bool conv = x.filter != 0u;
			for (uint32_t i = tid; i < tw * th; i += kVariedThreads) {
				uint32_t px;
				if constexpr (C == 4) {
					px = reinterpret_cast<const uint32_t *>(src)[i];
					if (conv) px = premultiply(px);  // fir: U8x4 is alpha-premultiplied before a convolution
				} else {
					px = (uint32_t)src[3u * i] | ((uint32_t)src[3u * i + 1u] << 8) | ((uint32_t)src[3u * i + 2u] << 16) | 0xff000000u;
				}
				s_src[i] = px;
			}
			ExpandTab tab_x{0, 0, 0, 0}, tab_y{0, 0, 0, 0};
			auto stage_windows = [&](uint32_t *wd, const ExpandTab &tab, uint32_t outs) {
				for (uint32_t o = tid; o < outs; o += kVariedThreads) {
					uint32_t *d = wd + x.wdw * o;
					const uint32_t first = x.starts[tab.start_off + o];
					const uint32_t cnt = conv ? x.sizes[tab.start_off + o] : 1u;
					d[0] = first | (cnt << 16);
					if (conv) {
						const int16_t *k = x.coeffs + tab.coeff_off + o * tab.window;
						for (uint32_t j = 0; j < cnt; j += 2u)
							d[1u + (j >> 1)] = (uint32_t)(uint16_t)k[j] | (j + 1u < cnt ? (uint32_t)(uint16_t)k[j + 1u] << 16 : 0u);
					}
				}
			};
			if (tw != w) {
				tab_x = x.dir[(size_t)x.slot[w] * x.stride + tw];
				stage_windows(s_wx, tab_x, w);
			}
			if (th != h) {
				tab_y = x.dir[(size_t)x.slot[h] * x.stride + th];
				stage_windows(s_wy, tab_y, h);
			}
			__syncthreads();

			uint32_t *out;
			if (!conv) {  // ResizeAlg::Nearest
				RowWalker rw(tid, kVariedThreads, w);
				for (uint32_t i = tid; i < n; i += kVariedThreads, rw.next()) {
					const uint32_t sx = tw == w ? rw.col : (s_wx[x.wdw * rw.col] & 0xffffu), sy = th == h ? rw.row : (s_wy[x.wdw * rw.row] & 0xffffu);
					s_tmp[i] = s_src[sy * tw + sx];
				}
				out = s_tmp;
				__syncthreads();
			} else {
				const bool need_h = tw != w, need_v = th != h;
				out = s_src;
				if (need_h) {
					// horizontal pass: item = (ox, y) of the th stored rows
					const int prec = tab_x.precision;
					const int32_t init = 1 << (prec - 1);
					RowWalker rw(tid, kVariedThreads, w);
					for (uint32_t i = tid; i < w * th; i += kVariedThreads, rw.next()) {
						const uint32_t *wd = s_wx + x.wdw * rw.col;
						const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
						const uint32_t *row = s_src + rw.row * tw + first;
						int32_t acc[4] = {init, init, init, init};
						// two taps per v_dot2_i32_i16 (an odd count has a zero weight for the pixel read past the window, which is
						// still inside the plane: tw < w)
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
					__syncthreads();
				}
				if (need_v) {
					// vertical pass: item = (ox, oy); the rows it reads are w wide (w == tw when only this pass runs; the row an odd
					// count reads past the window is still inside the plane: th < h)
					const uint32_t *cur = need_h ? s_tmp : s_src;
					uint32_t *o = need_h ? s_src : s_tmp;
					const int prec = tab_y.precision;
					const int32_t init = 1 << (prec - 1);
					RowWalker rw(tid, kVariedThreads, w);
					for (uint32_t i = tid; i < n; i += kVariedThreads, rw.next()) {
						const uint32_t *wd = s_wy + x.wdw * rw.row;
						const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
						const uint32_t *col = cur + first * w + rw.col;
						int32_t acc[4] = {init, init, init, init};
						for (uint32_t j = 0; j < cnt; j += 2u) {
							const uint32_t w2 = wd[1u + (j >> 1)], p0 = col[j * w], p1 = col[(j + 1u) * w];
#pragma unroll
							for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
						}
						uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
						px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
						if constexpr (C == 4) px = unpremultiply(px);
						o[i] = px;
					}
					out = o;
					__syncthreads();
				}
			}
			uint32_t *other = out == s_src ? s_tmp : s_src;
			if constexpr (C == 4) {
				s_x = reinterpret_cast<uint8_t *>(out);
				s_o = reinterpret_cast<uint8_t *>(other);
			} else {
				// RGB: the dwords packed to 3 bytes in the other plane (four pixels as three dwords, bytes at the tail)
				const uint32_t n4 = n >> 2;
				for (uint32_t q = tid; q < n4; q += kVariedThreads) {
					const uint32_t p0 = out[4u * q], p1 = out[4u * q + 1u], p2 = out[4u * q + 2u], p3 = out[4u * q + 3u];
					other[3u * q] = (p0 & 0xffffffu) | (p1 << 24);
					other[3u * q + 1u] = ((p1 >> 8) & 0xffffu) | (p2 << 16);
					other[3u * q + 2u] = ((p2 >> 16) & 0xffu) | (p3 << 8);
				}
				uint8_t *ob = reinterpret_cast<uint8_t *>(other);
				for (uint32_t i = 4u * n4 + tid; i < n; i += kVariedThreads) {
					const uint32_t px = out[i];
					ob[3u * i] = (uint8_t)px;
					ob[3u * i + 1u] = (uint8_t)(px >> 8);
					ob[3u * i + 2u] = (uint8_t)(px >> 16);
				}
				s_x = ob;
				s_o = reinterpret_cast<uint8_t *>(out);
				__syncthreads();
			}
		}
		uint8_t *s_a = l.own != 0u ? reinterpret_cast<uint8_t *>(lds) + l.own : s_o;  // I, or a vertical-only result
		uint8_t *s_f = s_a + l.f;                                                       // F
		float *s_plane = reinterpret_cast<float *>(s_a);                                // [4][kVariedChunk] (the detector, before A holds a pass)

		// ---- 5. the detector up to what the factor has not entered, once
		float xr = 0.0f;
		uint32_t shz = 0, svr = 0;
		if (oklab) xr = varied_oklab_raw<C>(s_x, n, s_lms, s_alpha, s_scale, s_plane, s_acc, tid);
		else varied_sobel_sums<C>(s_x, w, h, s_red, tid, shz, svr);

		// ---- 6. (varied_ladder_kernel 3) every rung's decision: thread r decides rung r
		if (tid < n_rungs) {
			const float k = la.factors[tid];
			float v0, v1;
			if (oklab) {
				v0 = v1 = parse_value((xr * k) * 10.0f);  // pixlzr.rs:162 (BASE_FACTOR, :15), :177-178
			} else {
				const uint64_t fac = (uint64_t)(w - 2u) * (uint64_t)(h - 2u) * 4096ull;  // operations.rs:253-254
				if (fac == 0ull || w < 2u || h < 2u) {
					v0 = v1 = 0.0f;  // 0/0: the negative default NaN, which parse_value turns into 0 (finish_tile)
				} else {
					const double dfac = (double)fac;
					v0 = parse_value((float)((double)shz / dfac) * k);  // :256-257, pixlzr.rs:199
					v1 = parse_value((float)((double)svr / dfac) * k);
				}
			}
			// level_count against the thresholds (round(log2f(v)) >= -k), as the single-geometry call decides it
			uint32_t mx = 0, my = 0;
#pragma unroll
			for (int j = 0; j < kMaxLevel; ++j) {
				mx += v0 < a.thresholds[j] ? 1u : 0u;
				my += v1 < a.thresholds[j] ? 1u : 0u;
			}
			const uint32_t nw = reduced_size(w, mx), nh = reduced_size(h, my);  // operations.rs:150-151
			const size_t at = (size_t)tid * a.n_tiles + tile_g;
			a.value[at] = hypot_f32(v0, v1);  // operations.rs:154
			a.out_w[at] = nw;
			a.out_h[at] = nh;
			s_key[tid] = (nw != w ? mx : 0u) | ((nh != h ? my : 0u) << 8);
		}
		__syncthreads();  // the keys: the same in every wave from here on

		if (a.out_px != nullptr) {
			auto slot_of = [&](uint32_t r) { return a.out_px + ((uint64_t)r * a.n_tiles + tile_g) * (uint64_t)a.slot_bytes; };
			// ---- (4) the clones (block.rs:279-281), while X still holds the tile's bytes
			bool shrinks = false;
			for (uint32_t r = 0; r < n_rungs; ++r) {
				if (s_key[r] == 0u) varied_store(slot_of(r), s_x, n * (uint32_t)C, tid);
				else shrinks = true;
			}
			if (shrinks) {
				__syncthreads();  // the clones have read X
				// ---- (5) ResizeAlg::Convolution, default options: U8x4 is alpha-premultiplied first
				if (C == 4 && !nearest) {
					uint32_t *p32 = reinterpret_cast<uint32_t *>(s_x);
					for (uint32_t i = tid; i < n; i += kVariedThreads) p32[i] = premultiply(p32[i]);
					__syncthreads();
				}
				// ---- (6) one resample per distinct pair of levels; X is only read
				for (uint32_t r = 0; r < n_rungs; ++r) {
					const uint32_t key = s_key[r];
					if (key == 0u) continue;
					bool done = false;
					for (uint32_t q = 0; q < r; ++q) done = done || s_key[q] == key;
					if (done) continue;
					const uint32_t mx = key & 255u, my = key >> 8;
					const bool need_h = mx != 0u, need_v = my != 0u;
					const uint32_t nw = need_h ? reduced_size(w, mx) : w, nh = need_v ? reduced_size(h, my) : h;
					const uint32_t lx = mx < (uint32_t)kMaxLevel ? mx : (uint32_t)kMaxLevel - 1u;
					const uint32_t ly = my < (uint32_t)kMaxLevel ? my : (uint32_t)kMaxLevel - 1u;
					const uint8_t *cur = s_x;
					if (need_h) {
						const TreeAxisEntry ex = a.dir[w * (uint32_t)kMaxLevel + lx];
						varied_pass<C>(a, ex, nearest, s_x, (uint32_t)C, w * (uint32_t)C, s_a, (uint32_t)C, nw * (uint32_t)C, h, tid);
						__syncthreads();
						cur = s_a;
					}
					if (need_v) {
						const TreeAxisEntry ey = a.dir[h * (uint32_t)kMaxLevel + ly];
						uint8_t *o = need_h ? s_f : s_a;
						// one "line" per column of the nw-wide image, samples a row apart
						varied_pass<C>(a, ey, nearest, cur, nw * (uint32_t)C, (uint32_t)C, o, nw * (uint32_t)C, (uint32_t)C, nw, tid);
						__syncthreads();
						cur = o;
					}
					if (C == 4 && !nearest) {
						varied_unpremultiply(reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(cur)), nw * nh, tid);
						__syncthreads();
					}
					for (uint32_t q = r; q < n_rungs; ++q)
						if (s_key[q] == key) varied_store(slot_of(q), cur, nw * nh * (uint32_t)C, tid);
					__syncthreads();  // the next pair reuses I and F
				}
			}
		}
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_reshrink_ladder(const ReshrinkLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.r.v.n_tiles == 0u || a.n_factors == 0u) return hipSuccess;
	const uint32_t lds = reshrink_ladder_lds(a.r.v.mode, a.r.v.bw, a.r.v.bh, channels, a.r.x.wdw).total;
	if (lds > 160u * 1024u) return hipErrorInvalidValue;
	// as many blocks as the CUs' LDS holds (at most eight of four waves per CU); the rest walk the grid-stride loop
	uint32_t per_cu = (160u * 1024u) / lds;
	per_cu = per_cu < 1u ? 1u : (per_cu > 8u ? 8u : per_cu);
	const uint64_t cap = (uint64_t)n_cus * per_cu;
	const uint32_t blocks = (uint32_t)(a.r.v.n_tiles < cap ? a.r.v.n_tiles : cap);
	auto go = [&](auto kernel) { return launch_with_lds(kernel, blocks, kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(reshrink_ladder_kernel<4>) : go(reshrink_ladder_kernel<3>);
}

uint32_t reshrink_ladder_lds_bytes(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t channels, uint32_t wdw)
{
	return reshrink_ladder_lds(mode, bw, bh, channels, wdw).total;
}

}  // namespace pxz
