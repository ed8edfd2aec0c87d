// pxz_retile.hip -- stored tiles of a varied batch brought to another block size without their images
// (pxz_retile_varied_frames_device): the reference CLI's pix_to_pix (src/bin/main.rs:233-265: open a .pixlzr file,
// to_image(filter), from_image, shrink, save) with -b, a block size that CHANGES.  A tile of the rebuilt image's new grid is
// then no longer the expansion of one stored tile: it is put together from the parts of the stored tiles that cover it.  That
// is still per-tile work, so nothing of image size touches HBM: stored bytes in, stored bytes out.
//
// retile_kernel: one DESTINATION tile per block of 256 threads, grid-stride over the flat tile space of the destination layout
// (pxz_varied_layout at the new block), owners by owner_of (pxz_device.h), the grid of tile_blocks (pxz_launch.h).  Image i is
// entry i of both per-image tables, the destination layout's (v.images) and the source layout's (src_images).  A tile
//   1. is the rectangle [X0, X1) x [Y0, Y1) of its image; the source tiles that cover it are the columns X0 / sbw ..
//                (X1 - 1) / sbw and the rows Y0 / sbh .. (Y1 - 1) / sbh of the source grid: at most ceil(dbw / sbw) + 1 by
//                ceil(dbh / sbh) + 1 tiles, all of them inside the grid (the rectangle lies inside the image);
//   2. is assembled in X (one dword per pixel, rows w apart), covering tile by covering tile.  Of each the kernel reads the stored
//                size (tw, th) and, from the source grid, its full size (fw, fh) -- a source edge tile has its own -- and wants
//                the part [cx0, cx1) x [cy0, cy1) of it (tile coordinates).
//                A stored size that cannot be (zero, or beyond the tile's place in the SOURCE grid) is handled as
//                bad_stored_size handles it (pxz_device.h): status bit 0, the image's flag; the destination tile gets 0 x 0
//                and value bits 0, its slot is left as it was, and the assembly stops there.
//                A tile stored at full size is cloned in (block.rs:279-281): the wanted part straight from its slot.
//                Otherwise the stored pixels that the part's windows read -- a rectangle of the stored tile -- are staged as one
//                dword per pixel (RGBA under a convolution premultiplied as fir does) and the part is expanded INTO ITS PLACE in
//                X with the arithmetic of varied_resize_tile step 3
//                (pxz_device.h) as reshrink_kernel step 4 has it (pxz_reshrink.hip) -- COPIED from there, by the whole block:
//                the Nearest pick; or the horizontal pass, the vertical pass with clip8_med3 and the un-premultiply; one pass
//                where only one axis differs.  A FIX TO THE ARITHMETIC THERE BELONGS HERE TOO, and the other way round.
//                Only the wanted columns of the horizontal pass are computed (over the staged rows) and only the wanted rows of
//                the vertical pass: an output sample depends on
//                its own window alone and the intermediate is clipped per sample, so the part has the bits of the whole
//                tile's expansion.  The tables are the (full size, stored size) directory of put_varied_expand_tables for the
//                source geometry; only the wanted samples' windows are staged.  (Expanding the tile whole with varied_resize_tile
//                and copying the part gives the same bits; it was measured and lost in every row);
//   3. is packed: RGB to 3 bytes per pixel, in place, so that what follows reads the tile image varied_kernel reads;
//   4. is measured, decided, resampled and stored: steps 2 and 3 of varied_kernel (pxz_varied.hip) as reshrink_kernel step 5
//                runs them, unchanged in arithmetic (copied from there, not called, for the reason given there: DESIGN.md 8k;
//                the pass and the store are pxz_varied_tile.h's).
// Source and destination layouts differ, so there is no in-place form.
// Steps 1 to 3 stand a second time as retile_assemble (pxz_varied_tile.h), which retile_ladder_kernel (pxz_retile_ladder.hip)
// calls; THIS KERNEL KEEPS ITS INLINE TEXT -- its timing is pinned in DESIGN.md 8o, and folding it onto the function is a change
// with its own A/B.  A FIX TO STEPS 1 TO 3 HERE BELONGS THERE TOO, and the other way round.
//
// LDS of one block: retile_lds (pxz_varied_tile.h), where the layout and its limit are described; the kernel, this launch and
// the host take it from there.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(kVariedThreads) retile_kernel(const RetileArgs r)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	const VariedArgs &a = r.v;
	const TileResizeArgs &x = r.x;
	const uint32_t tid = threadIdx.x;
	const bool oklab = a.mode == 0u;
	const RetileLds L = retile_lds(a.mode, x.bw, x.bh, a.bw, a.bh, x.wdw);
	uint8_t *const s_base = reinterpret_cast<uint8_t *>(lds);
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint32_t *s_img = reinterpret_cast<uint32_t *>(s_base + L.x);
	uint32_t *s_src = reinterpret_cast<uint32_t *>(s_base + L.u), *s_tmp = reinterpret_cast<uint32_t *>(s_base + L.inter);
	uint32_t *s_wx = reinterpret_cast<uint32_t *>(s_base + L.wx), *s_wy = s_wx + x.wdw * x.bw;
	if (oklab) {
		oklab_fill_tables(s_lms, s_alpha, s_scale, tid);
		__syncthreads();
	}
	const bool conv = x.filter != 0u;

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		// ---- 1. the tile's owner, its rectangle, and the source tiles that cover it
		const uint32_t owner = owner_of(a.images, a.n_images, tile_g, &VariedImage::tile0);
		const VariedImage im = a.images[owner];
		const VariedImage sm = r.src_images[owner];
		const uint32_t t = tile_g - im.tile0;
		const uint32_t ty = t / im.cols, tx = t - ty * im.cols;
		const uint32_t w = tx + 1u == im.cols ? im.edge_w : a.bw;  // split.rs:18
		const uint32_t h = ty + 1u == im.rows ? im.edge_h : a.bh;  // split.rs:19
		const uint32_t n = w * h;
		const uint32_t X0 = tx * a.bw, Y0 = ty * a.bh, X1 = X0 + w, Y1 = Y0 + h;
		const uint32_t sc0 = X0 / x.bw, sr0 = Y0 / x.bh;
		const uint32_t ncx = (X1 - 1u) / x.bw - sc0 + 1u, ncy = (Y1 - 1u) / x.bh - sr0 + 1u;

		// ---- 2. the tile image, covering tile by covering tile (every value that steers the loop is the same in all threads)
		bool bad = false;
		for (uint32_t k = 0; k < ncx * ncy; ++k) {
			const uint32_t ky = k / ncx;
			const uint32_t sty = sr0 + ky, stx = sc0 + (k - ky * ncx);
			const uint32_t fw = stx + 1u == sm.cols ? sm.edge_w : x.bw, fh = sty + 1u == sm.rows ? sm.edge_h : x.bh;
			const uint32_t st = sm.tile0 + sty * sm.cols + stx;
			const uint32_t tw = x.tile_w[st], th = x.tile_h[st];
			if (tw == 0u || th == 0u || tw > fw || th > fh) {  // (bad_stored_size, pxz_device.h)
				bad = true;
				break;
			}
			const uint8_t *src = x.slots + (size_t)st * x.slot_bytes;
			// the wanted part in the source tile's coordinates, and its place in X
			const uint32_t ox = stx * x.bw, oy = sty * x.bh;
			const uint32_t cx0 = X0 > ox ? X0 - ox : 0u, cy0 = Y0 > oy ? Y0 - oy : 0u;
			const uint32_t cx1 = (X1 < ox + fw ? X1 : ox + fw) - ox, cy1 = (Y1 < oy + fh ? Y1 : oy + fh) - oy;
			const uint32_t cw = cx1 - cx0, chh = cy1 - cy0;
			uint32_t *dst = s_img + (oy + cy0 - Y0) * w + (ox + cx0 - X0);

			if (tw == fw && th == fh) {
				// clone in: the part's pixels from the slot (no LDS but X is touched: no barrier between two clones)
				RowWalker rw(tid, kVariedThreads, cw);
				for (uint32_t i = tid; i < cw * chh; i += kVariedThreads, rw.next()) {
					const uint32_t at = (cy0 + rw.row) * fw + cx0 + rw.col;
					uint32_t px;
					if constexpr (C == 4) px = reinterpret_cast<const uint32_t *>(src)[at];
					else px = (uint32_t)src[3u * at] | ((uint32_t)src[3u * at + 1u] << 8) | ((uint32_t)src[3u * at + 2u] << 16) | 0xff000000u;
					dst[rw.row * w + rw.col] = px;
				}
				continue;
			}
			ExpandTab tab_x{0, 0, 0, 0}, tab_y{0, 0, 0, 0};
			auto stage_windows = [&](uint32_t *wd, const ExpandTab &tab, uint32_t lo, uint32_t hi) {
				for (uint32_t o = lo + tid; o < hi; o += kVariedThreads) {
					uint32_t *d = wd + x.wdw * o;
					const uint32_t first = x.starts[tab.start_off + o];
					const uint32_t cnt = conv ? x.sizes[tab.start_off + o] : 1u;
					d[0] = first | (cnt << 16);
					if (conv) {
						const int16_t *kk = x.coeffs + tab.coeff_off + o * tab.window;
						for (uint32_t j = 0; j < cnt; j += 2u)
							d[1u + (j >> 1)] = (uint32_t)(uint16_t)kk[j] | (j + 1u < cnt ? (uint32_t)(uint16_t)kk[j + 1u] << 16 : 0u);
					}
				}
			};
			// expand (reshrink_kernel step 4, restricted to the part).  The windows of the wanted samples at their own indices:
			// first | count << 16, then the weights as i16 pairs
			const bool need_h = tw != fw, need_v = th != fh;
			// the stored samples the part's windows read: [rx0, rx1) x [ry0, ry1) -- window starts ascend with the sample, so the first
			// wanted sample's start and the last one's end bound them (an axis that keeps its size: the part itself)
			uint32_t rx0 = cx0, rx1 = cx1, ry0 = cy0, ry1 = cy1;
			if (need_h) {
				tab_x = x.dir[(size_t)x.slot[fw] * x.stride + tw];
				stage_windows(s_wx, tab_x, cx0, cx1);
				rx0 = x.starts[tab_x.start_off + cx0];
				rx1 = x.starts[tab_x.start_off + cx1 - 1u] + (conv ? x.sizes[tab_x.start_off + cx1 - 1u] : 1u);
			}
			if (need_v) {
				tab_y = x.dir[(size_t)x.slot[fh] * x.stride + th];
				stage_windows(s_wy, tab_y, cy0, cy1);
				ry0 = x.starts[tab_y.start_off + cy0];
				ry1 = x.starts[tab_y.start_off + cy1 - 1u] + (conv ? x.sizes[tab_y.start_off + cy1 - 1u] : 1u);
			}
			const uint32_t pw = rx1 - rx0, ph = ry1 - ry0;  // (within L.pw x L.ph: retile_lds, pxz_varied_tile.h)
			// those stored pixels -> one dword per pixel in s_src, rows pw apart (RGBA under a convolution alpha-premultiplied as fir does)
			{
				RowWalker rw(tid, kVariedThreads, pw);
				for (uint32_t i = tid; i < pw * ph; i += kVariedThreads, rw.next()) {
					const uint32_t at = (ry0 + rw.row) * tw + rx0 + rw.col;
					uint32_t px;
					if constexpr (C == 4) {
						px = reinterpret_cast<const uint32_t *>(src)[at];
						if (conv) px = premultiply(px);  // fir: U8x4 is alpha-premultiplied before a convolution
					} else {
						px = (uint32_t)src[3u * at] | ((uint32_t)src[3u * at + 1u] << 8) | ((uint32_t)src[3u * at + 2u] << 16) | 0xff000000u;
					}
					s_src[i] = px;
				}
			}
			__syncthreads();

			if (!conv) {  // ResizeAlg::Nearest
				RowWalker rw(tid, kVariedThreads, cw);
				for (uint32_t i = tid; i < cw * chh; i += kVariedThreads, rw.next()) {
					const uint32_t ux = cx0 + rw.col, uy = cy0 + rw.row;
					const uint32_t sx = need_h ? (s_wx[x.wdw * ux] & 0xffffu) : ux, sy = need_v ? (s_wy[x.wdw * uy] & 0xffffu) : uy;
					dst[rw.row * w + rw.col] = s_src[(sy - ry0) * pw + (sx - rx0)];
				}
			} else {
				if (need_h) {
					// horizontal pass: item = (wanted column, row) -- of the ph staged rows (into the intermediate, cw wide, when the
					// vertical pass follows; th == fh otherwise: the staged rows are the wanted rows, into X)
					const int prec = tab_x.precision;
					const int32_t init = 1 << (prec - 1);
					RowWalker rw(tid, kVariedThreads, cw);
					for (uint32_t i = tid; i < cw * ph; i += kVariedThreads, rw.next()) {
						const uint32_t *wd = s_wx + x.wdw * (cx0 + rw.col);
						const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
						const uint32_t *row = s_src + rw.row * pw + (first - rx0);
						int32_t acc[4] = {init, init, init, init};
						// two taps per v_dot2_i32_i16 (an odd count has a zero weight for the pixel read past the window: at the end of
						// the staged rectangle's last row that is the first dword of the intermediate, inside the block's LDS)
						for (uint32_t j = 0; j < cnt; j += 2u) {
							const uint32_t w2 = wd[1u + (j >> 1)], p0 = row[j], p1 = row[j + 1u];
#pragma unroll
							for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
						}
						uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
						px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
						if (need_v) {
							s_tmp[i] = px;
						} else {
							if constexpr (C == 4) px = unpremultiply(px);
							dst[rw.row * w + rw.col] = px;
						}
					}
					if (need_v) __syncthreads();
				}
				if (need_v) {
					// vertical pass: item = (wanted column, wanted row); the rows it reads are cw wide behind a horizontal pass, the
					// staged rows otherwise (pw == cw then).  The row an odd count reads past the window lies behind the rectangle:
					// in the intermediate or in the staged windows, inside the block's LDS, and has a zero weight
					const uint32_t *cur = need_h ? s_tmp : s_src;
					const uint32_t pitch = need_h ? cw : pw;
					const int prec = tab_y.precision;
					const int32_t init = 1 << (prec - 1);
					RowWalker rw(tid, kVariedThreads, cw);
					for (uint32_t i = tid; i < cw * chh; i += kVariedThreads, rw.next()) {
						const uint32_t *wd = s_wy + x.wdw * (cy0 + rw.row);
						const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
						const uint32_t *col = cur + (first - ry0) * pitch + rw.col;
						int32_t acc[4] = {init, init, init, init};
						for (uint32_t j = 0; j < cnt; j += 2u) {
							const uint32_t w2 = wd[1u + (j >> 1)], p0 = col[j * pitch], p1 = col[(j + 1u) * pitch];
#pragma unroll
							for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
						}
						uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
						px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
						if constexpr (C == 4) px = unpremultiply(px);
						dst[rw.row * w + rw.col] = px;
					}
				}
			}
			__syncthreads();  // the next covering tile reuses the staging
		}
		if (bad) {
			if (tid == 0u) {
				atomicOr(x.status, 1u);
				if (r.image_flags) r.image_flags[owner] = 1u;
				a.value[tile_g] = 0.0f;
				a.out_w[tile_g] = 0u;
				a.out_h[tile_g] = 0u;
			}
			__syncthreads();  // the next tile writes X, which threads still behind may be cloning into
			continue;
		}
		__syncthreads();

		// ---- 3. the tile image as varied_kernel stages it: C bytes per pixel, tightly packed, in X; U is the other plane
		uint8_t *s_x = reinterpret_cast<uint8_t *>(s_img), *s_a = reinterpret_cast<uint8_t *>(s_src);
		if constexpr (C == 3) {
			// RGB: the dwords packed to 3 bytes in place, 1024 pixels a round (four per thread as three dwords, bytes at the tail): a
			// round writes below what later rounds read, and the barrier keeps its own reads ahead of its writes
			for (uint32_t base = 0; base < n; base += 4u * kVariedThreads) {
				const uint32_t q = (base >> 2) + tid, i0 = 4u * q;
				uint32_t p[4];
#pragma unroll
				for (uint32_t j = 0; j < 4u; ++j) p[j] = i0 + j < n ? s_img[i0 + j] : 0u;
				__syncthreads();
				if (i0 + 4u <= n) {
					s_img[3u * q] = (p[0] & 0xffffffu) | (p[1] << 24);
					s_img[3u * q + 1u] = ((p[1] >> 8) & 0xffffu) | (p[2] << 16);
					s_img[3u * q + 2u] = ((p[2] >> 16) & 0xffu) | (p[3] << 8);
				} else {
					for (uint32_t j = 0; i0 + j < n; ++j) {
						s_x[3u * (i0 + j)] = (uint8_t)p[j];
						s_x[3u * (i0 + j) + 1u] = (uint8_t)(p[j] >> 8);
						s_x[3u * (i0 + j) + 2u] = (uint8_t)(p[j] >> 16);
					}
				}
				__syncthreads();
			}
		}
		float *s_plane = reinterpret_cast<float *>(s_a);  // [4][kVariedChunk]: U has room for them in shrink_by mode

		// ---- 4a. the detector (varied_kernel step 2, as reshrink_kernel step 5a)
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

		// ---- 4b. the resample into the tile's slot (varied_kernel step 3, as reshrink_kernel step 5b)
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
					varied_unpremultiply(reinterpret_cast<uint32_t *>(cur), nw * nh, tid);
					__syncthreads();
				}
				varied_store(slot, cur, nw * nh * (uint32_t)C, tid);
			}
		}
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_retile(const RetileArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.v.n_tiles == 0u) return hipSuccess;
	const uint32_t lds = retile_lds(a.v.mode, a.x.bw, a.x.bh, a.v.bw, a.v.bh, a.x.wdw).total;
	if (lds > kLdsPerCu) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.v.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(retile_kernel<4>) : go(retile_kernel<3>);
}

uint32_t retile_lds_bytes(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t wdw)
{
	return retile_lds(mode, sbw, sbh, dbw, dbh, wdw).total;
}

}  // namespace pxz
