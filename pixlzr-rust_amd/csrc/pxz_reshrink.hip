// pxz_reshrink.hip -- stored tiles of a varied batch shrunk again without their images (pxz_reshrink_varied_frames_device):
// the reference CLI's pix_to_pix (src/bin/main.rs:233-265: open a .pixlzr file, to_image(filter), from_image, shrink, save)
// for a block size that stays the same.  Tile t of the rebuilt image is then exactly the expansion of stored tile t, so the
// flow is per-tile work and nothing of image size touches HBM: stored bytes in, stored bytes out.
//
// reshrink_kernel: one tile per block of 256 threads, grid-stride over the flat tile space of pxz_varied_layout, owners by
// owner_of (pxz_device.h), the grid of tile_blocks (pxz_launch.h).  A tile
//   1. reads     its stored size (tw, th) and, from its owner's grid, its full size (fw, fh);
//   2. is flagged and skipped when its stored size cannot be (zero, or beyond its place), as bad_stored_size does it: status
//                bit 0, the image's flag, outputs 0 x 0 with value bits 0, its slot left as it was;
//   3. is cloned in when it is stored at full size (block.rs:279-281): the slot's bytes go straight into the tile image;
//   4. is expanded otherwise: the arithmetic of varied_resize_tile step 3 (pxz_device.h), done by the whole block -- stride
//                256, __syncthreads() where the wave form has wsync.  THIS KERNEL KEEPS ITS OWN COPY of steps 3 and 4
//                (reshrink_tile_image, pxz_varied_tile.h, is the text the re-shrink ladder runs) and of the detectors: on the
//                shared functions its shrink_by rows measured 0.5-1 % slower than before, outside the rule of DESIGN.md 8g, and
//                on the shared tile image alone 4-7 %.  A FIX TO THE ARITHMETIC THERE BELONGS HERE TOO, and the
//                other way round.  The result is one dword per pixel; RGB is then packed to 3 bytes, so that what follows reads
//                the tile image varied_kernel reads;
//   5. is measured, decided, resampled and stored: steps 2 and 3 of varied_kernel (pxz_varied.hip), unchanged in arithmetic
//                (copied, not called; the pass and the store are pxz_varied_tile.h's).
// In place: tile t's stored size and slot are read only by the block that writes tile t's outputs, into registers and LDS
// and before its first store (barriers lie between), so out_w / out_h / out_px may be the input arrays.
//
// LDS of one block (reshrink_lds with no rung channels, pxz_varied_tile.h: the launch and the host take it from there; the kernel
// derives the same offsets from v.tile_bytes = one plane, the pointer arithmetic it was measured with):
//   [oklab tables, shrink_by only: 14 336 B] [P0: plane] [P1: plane] [windows of both axes: (bw + bh) * wdw dwords]
//   [the detector's planes, shrink_by with planes below 16 KB only: 16 KB]
// A plane is bw * bh dwords (the expand works on one dword per pixel for both channel counts), so the call's limit is
// block_w * block_h * 4 <= 65536 for RGB and RGBA alike: 128 KB + 14 KB + 5 KB (wdw <= 5: an up-scaling window has at most
// 7 taps) at 128x128, under the CU's 160 KB.  Beyond a 64 KB plane reshrink_lds answers "does not fit"; within it only
// the windows of a very oblong block (bw + bh above about 900) can still exceed the CU.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(kVariedThreads) reshrink_kernel(const ReshrinkArgs r)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	const VariedArgs &a = r.v;
	const TileResizeArgs &x = r.x;
	const uint32_t tid = threadIdx.x;
	const bool oklab = a.mode == 0u;
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint8_t *s_p0 = reinterpret_cast<uint8_t *>(lds) + (oklab ? kVariedTables * 4u : 0u);
	uint8_t *s_p1 = s_p0 + a.tile_bytes;
	uint32_t *s_wx = reinterpret_cast<uint32_t *>(s_p1 + a.tile_bytes), *s_wy = s_wx + x.wdw * a.bw;
	float *s_own = reinterpret_cast<float *>(s_wx + (((a.bw + a.bh) * x.wdw + 3u) & ~3u));  // (there only when the planes are small)
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

		// ---- 2. a stored size that cannot be (bad_stored_size, pxz_device.h): flagged, its outputs empty, its slot left alone
		if (tw == 0u || th == 0u || tw > w || th > h) {
			if (tid == 0u) {
				atomicOr(x.status, 1u);
				if (r.image_flags) r.image_flags[owner] = 1u;
				a.value[tile_g] = 0.0f;
				a.out_w[tile_g] = 0u;
				a.out_h[tile_g] = 0u;
			}
			continue;
		}

		uint8_t *s_x, *s_a;  // the tile image, tightly packed, and the other plane
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
			s_a = s_p1;
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
				s_a = reinterpret_cast<uint8_t *>(other);
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
				s_a = reinterpret_cast<uint8_t *>(out);
				__syncthreads();
			}
		}
		float *s_plane = a.tile_bytes < kVariedPlaneBytes ? s_own : reinterpret_cast<float *>(s_a);  // [4][kVariedChunk]

		// ---- 5a. the detector (varied_kernel step 2)
		float v0, v1;
		if (oklab) {
			const float count = (float)n;  // operations.rs:51
			float mean = 0.0f;
			for (int pass = 0; pass < 2; ++pass) {
				float acc = 0.0f;
				for (uint32_t base = 0; base < n; base += kVariedChunk) {
					const uint32_t first = base + tid * 4u;
					uint32_t px[4];
#pragma unroll
					for (int j = 0; j < 4; ++j) px[j] = first + (uint32_t)j < n ? varied_pixel(s_x, first + (uint32_t)j, C) : 0u;
#pragma unroll
					for (int j = 0; j < 4; j += 2) {
						float o0[3], o1[3];
						oklab_pair(px[j], px[j + 1], s_lms, s_scale, o0, o1);
						const uint32_t k = tid * 4u + (uint32_t)j;
#pragma unroll
						for (int c = 0; c < 3; ++c) {
							s_plane[c * kVariedChunk + k] = o0[c];
							s_plane[c * kVariedChunk + k + 1u] = o1[c];
						}
						s_plane[3 * kVariedChunk + k] = s_alpha[px[j] >> 24];
						s_plane[3 * kVariedChunk + k + 1u] = s_alpha[px[j + 1] >> 24];
					}
					__syncthreads();
					if (tid < 4u) {
						// chains a, b, l, alpha: one lane each, in pixel order (operations.rs:60-63, :80-83)
						const uint32_t m = n - base < kVariedChunk ? n - base : kVariedChunk;
						const float *v = s_plane + tid * kVariedChunk;
						const uint32_t m4 = m & ~3u;
						if (pass == 0) {
							for (uint32_t i = 0; i < m4; i += 4u) {
								const float4 q = *reinterpret_cast<const float4 *>(v + i);
								acc += q.x; acc += q.y; acc += q.z; acc += q.w;
							}
							for (uint32_t i = m4; i < m; ++i) acc += v[i];
						} else {
							for (uint32_t i = 0; i < m4; i += 4u) {
								const float4 q = *reinterpret_cast<const float4 *>(v + i);
								acc += fabsf(q.x - mean); acc += fabsf(q.y - mean); acc += fabsf(q.z - mean); acc += fabsf(q.w - mean);
							}
							for (uint32_t i = m4; i < m; ++i) acc += fabsf(v[i] - mean);
						}
					}
					__syncthreads();
				}
				if (tid < 4u) {
					if (pass == 0) mean = __fdiv_rn(acc, count);  // :65-68
					else s_acc[tid] = acc;
				}
			}
			__syncthreads();
			const float total = C == 4 ? ((s_acc[0] + s_acc[1]) + s_acc[2]) + s_acc[3] : (s_acc[0] + s_acc[1]) + s_acc[2];  // :89 / :124
			const float xv = __fdiv_rn(total, count);
			v0 = v1 = parse_value((xv * a.factor) * 10.0f);  // pixlzr.rs:162 (BASE_FACTOR, :15), :177-178
		} else {
			// get_block_variance_directionally (operations.rs:192-259): Sobel-like sums over the (w - 2) x (h - 2) interior
			uint32_t shz = 0, svr = 0;
			if (w > 2u && h > 2u) {
				const uint32_t iw = w - 2u, rb = w * (uint32_t)C;
				for (uint32_t i = tid; i < iw * (h - 2u); i += kVariedThreads) {
					const uint32_t y = i / iw, xx = i - y * iw;
					const uint8_t *p0 = s_x + y * rb + xx * (uint32_t)C, *p1 = p0 + rb, *p2 = p1 + rb;
#pragma unroll
					for (int c = 0; c < 3; ++c) {
						const int32_t hz = -(int32_t)p0[c] - 2 * (int32_t)p0[C + c] - (int32_t)p0[2 * C + c] + (int32_t)p2[c] +
						                   2 * (int32_t)p2[C + c] + (int32_t)p2[2 * C + c];
						const int32_t vr = -(int32_t)p0[c] - 2 * (int32_t)p1[c] - (int32_t)p2[c] + (int32_t)p0[2 * C + c] +
						                   2 * (int32_t)p1[2 * C + c] + (int32_t)p2[2 * C + c];
						shz += (uint32_t)(hz < 0 ? -hz : hz);
						svr += (uint32_t)(vr < 0 ? -vr : vr);
					}
				}
			}
			for (int d = 32; d >= 1; d >>= 1) {
				shz += (uint32_t)__shfl_xor((int)shz, d, 64);
				svr += (uint32_t)__shfl_xor((int)svr, d, 64);
			}
			if ((tid & 63u) == 0u) {
				s_red[2u * (tid >> 6)] = shz;
				s_red[2u * (tid >> 6) + 1u] = svr;
			}
			__syncthreads();
			shz = svr = 0;
#pragma unroll
			for (uint32_t q = 0; q < kVariedThreads / 64u; ++q) {
				shz += s_red[2u * q];
				svr += s_red[2u * q + 1u];
			}
			const uint64_t fac = (uint64_t)(w - 2u) * (uint64_t)(h - 2u) * 4096ull;  // operations.rs:253-254
			if (fac == 0ull || w < 2u || h < 2u) {
				v0 = v1 = 0.0f;  // 0/0: the negative default NaN, which parse_value turns into 0 (finish_tile)
			} else {
				const double dfac = (double)fac;
				v0 = parse_value((float)((double)shz / dfac) * a.factor);  // :256-257, pixlzr.rs:199
				v1 = parse_value((float)((double)svr / dfac) * a.factor);
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
		if (tid == 0u) {
			a.value[tile_g] = hypot_f32(v0, v1);  // operations.rs:154
			a.out_w[tile_g] = nw;
			a.out_h[tile_g] = nh;
		}

		// ---- 5b. the resample into the tile's slot (varied_kernel step 3)
		if (a.out_px != nullptr) {
			uint8_t *slot = a.out_px + (uint64_t)tile_g * a.slot_bytes;
			if (nw == w && nh == h) {
				varied_store(slot, s_x, n * (uint32_t)C, tid);  // block.rs:279-281: a clone
			} else {
				const bool nearest = a.filter == 0u;
				const bool need_h = nw != w, need_v = nh != h;
				const uint32_t lx = mx < (uint32_t)kMaxLevel ? mx : (uint32_t)kMaxLevel - 1u;
				const uint32_t ly = my < (uint32_t)kMaxLevel ? my : (uint32_t)kMaxLevel - 1u;
				if (C == 4 && !nearest) {
					// ResizeAlg::Convolution, default options: U8x4 is alpha-premultiplied first
					uint32_t *p32 = reinterpret_cast<uint32_t *>(s_x);
					for (uint32_t i = tid; i < n; i += kVariedThreads) p32[i] = premultiply(p32[i]);
					__syncthreads();
				}
				uint8_t *cur = s_x;
				if (need_h) {
					const TreeAxisEntry ex = a.dir[w * (uint32_t)kMaxLevel + lx];
					varied_pass<C>(a, ex, nearest, s_x, (uint32_t)C, w * (uint32_t)C, s_a, (uint32_t)C, nw * (uint32_t)C, h, tid);
					__syncthreads();
					cur = s_a;
				}
				if (need_v) {
					const TreeAxisEntry ey = a.dir[h * (uint32_t)kMaxLevel + ly];
					uint8_t *o = cur == s_x ? s_a : s_x;
					// one "line" per column of the nw-wide image, samples a row apart
					varied_pass<C>(a, ey, nearest, cur, nw * (uint32_t)C, (uint32_t)C, o, nw * (uint32_t)C, (uint32_t)C, nw, tid);
					__syncthreads();
					cur = o;
				}
				if (C == 4 && !nearest) {
					uint32_t *p32 = reinterpret_cast<uint32_t *>(cur);
					for (uint32_t i = tid; i < nw * nh; i += kVariedThreads) {
						const uint32_t px = p32[i], al = px >> 24;
						const uint32_t rc = kRecipAlpha.v[al];
						uint32_t rr = ((px & 255u) * rc + 128u) >> 8, g = (((px >> 8) & 255u) * rc + 128u) >> 8, b = (((px >> 16) & 255u) * rc + 128u) >> 8;
						rr = rr > 255u ? 255u : rr;
						g = g > 255u ? 255u : g;
						b = b > 255u ? 255u : b;
						p32[i] = rr | (g << 8) | (b << 16) | (al << 24);
					}
					__syncthreads();
				}
				varied_store(slot, cur, nw * nh * (uint32_t)C, tid);
			}
		}
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_reshrink(const ReshrinkArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.v.n_tiles == 0u) return hipSuccess;
	const uint32_t lds = reshrink_lds(a.v.mode, a.v.bw, a.v.bh, 0u, a.x.wdw).total;
	if (lds > kLdsPerCu) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.v.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(reshrink_kernel<4>) : go(reshrink_kernel<3>);
}

uint32_t reshrink_lds_bytes(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t rung_channels, uint32_t wdw)
{
	return reshrink_lds(mode, bw, bh, rung_channels, wdw).total;
}

}  // namespace pxz
