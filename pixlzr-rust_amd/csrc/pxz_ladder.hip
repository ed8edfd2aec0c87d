// pxz_ladder.hip -- the factor ladder's second stage (pxz_shrink_ladder_frames_device, shrink_by): every tile is staged in
// LDS once and written out for all K rungs, with one resample per DISTINCT level among them.  The first stage is the
// ordinary detector in its identity form (pxz_api.cpp), which leaves the raw x = sum of deviations / count of every tile.
//
// The resample is the generic kernel's (pxz_shrink_generic.hip, process_tile): the same LDS image (four planes of u16 pairs,
// transposed planes for the vertical pass), the same dot2 convolutions over the same tables, the same alpha handling
// (fir's premultiply / un-premultiply for tiles with alpha < 255, the weight-sum shortcut for opaque ones) -- so a rung is
// bit-identical to a single-factor call, which every kernel of that flow is to the generic kernel.
//
// Compiled with -ffp-contract=off: (x * k) * 10 must be two f32 roundings, as the reference's x * factor * BASE_FACTOR.
#include "pxz_device.h"
#include "pxz_launch.h"

namespace pxz {

// The level of one rung (one lane per rung): shrink_by's closure (pixlzr.rs:160-162) on the raw value, parse_value
// (pixlzr.rs:177-178), then level_count's comparison against the thresholds' bit patterns -- lane by lane here, where
// level_count makes its key tile-uniform.
__device__ __forceinline__ uint32_t ladder_level(float x, float k, const uint32_t *breaks, uint32_t asc, float &v)
{
	v = parse_value((x * k) * 10.0f);  // BASE_FACTOR, pixlzr.rs:15
	const uint32_t key = __float_as_uint(v);
	uint32_t m = 0;
#pragma unroll
	for (int j = 0; j < kMaxLevel; ++j) m += ((key < breaks[j]) != (asc != 0u)) ? 1u : 0u;
	return m;
}

template <int NW, int C>
__device__ __forceinline__ void ladder_tile(const LadderArgs &a, const uint32_t tile_g, uint32_t *s_pl, uint32_t *s_red,
                                            const uint32_t tid)
{
	constexpr uint32_t TPT = 64u * NW;
	const uint32_t lane = tid & 63u;
	const uint32_t frame = fastdiv(tile_g, a.div_tpf);
	const uint32_t t = tile_g - frame * a.tiles_per_frame;
	const uint32_t ty = fastdiv(t, a.div_cols), tx = t - ty * a.cols;
	const uint32_t w = (tx == a.cols - 1) ? a.edge_w : a.bw;  // split.rs:18
	const uint32_t h = (ty == a.rows - 1) ? a.edge_h : a.bh;  // split.rs:19
	const uint32_t n = w * h;
	const uint32_t cls = (w != a.bw ? 1u : 0u) | (h != a.bh ? 2u : 0u);

	// ---- the rungs: lane r decides rung r (every wave of the block the same, so that the masks below are block-uniform) ----
	const bool live = lane < a.n_rungs;
	const float x = a.x[tile_g];
	uint32_t m = 0, nw = w, nh = h;
	if (live) {
		float v;
		m = ladder_level(x, a.factors[lane], a.breaks[cls], a.breaks_asc[cls], v);
		nw = reduced_size(w, m);  // operations.rs:150
		nh = reduced_size(h, m);  // :151
		if (tid < 64u) {
			const size_t o = (size_t)lane * a.n_tiles + tile_g;
			a.value[o] = hypot_f32(v, v);  // operations.rs:154
			a.out_w[o] = nw;
			a.out_h[o] = nh;
		}
	}
	if (a.out_px == nullptr) return;
	const uint64_t live_mask = __builtin_amdgcn_ballot_w64(live);
	const uint64_t clone_mask = __builtin_amdgcn_ballot_w64(live && nw == w && nh == h);
	uint64_t pending = live_mask & ~clone_mask;
	const uint64_t slot_bytes = a.slot_bytes;
	auto slot_of = [&](uint32_t r) { return a.out_px + ((uint64_t)r * a.n_tiles + tile_g) * slot_bytes; };

	const uint8_t *src = a.src + (size_t)frame * a.frame_stride + (size_t)(ty * a.bh) * a.pitch + (size_t)(tx * a.bw) * C;
	const uint32_t rs = a.rs, PD = a.plane_dw;
	uint32_t *s_tmp = s_pl + 4 * PD;
	uint16_t *pl16 = reinterpret_cast<uint16_t *>(s_pl);

	// ---- stage the tile: 16-B loads along image rows where they are aligned -> planar u16 pairs ----
	uint32_t alpha_and = 0xffu;
	const uint32_t qpr = w >> 2, nquad = qpr * h;
	const bool vec = C == 4 && ((w & 3u) == 0) && ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) && ((a.pitch & 15u) == 0);
	if (vec) {
		for (uint32_t i0 = 0; i0 < nquad; i0 += 4u * TPT) {
			uint4 v[4];
#pragma unroll
			for (uint32_t k = 0; k < 4; ++k) {
				const uint32_t i = i0 + tid + k * TPT;
				if (i < nquad) {
					const uint32_t row = small_div(i, qpr), col = i - row * qpr;
					v[k] = *reinterpret_cast<const uint4 *>(src + (size_t)row * a.pitch + col * 16u);
				}
			}
#pragma unroll
			for (uint32_t k = 0; k < 4; ++k) {
				const uint32_t i = i0 + tid + k * TPT;
				if (i < nquad) {
					const uint32_t row = small_div(i, qpr), col = i - row * qpr;
					alpha_and &= (v[k].x & v[k].y & v[k].z & v[k].w) >> 24;
					uint32_t *d = s_pl + row * rs + col * 2u;
#pragma unroll
					for (uint32_t c = 0; c < 4; ++c) {
						const uint32_t sel = c | 0x0c000c00u | ((4u + c) << 16);
						uint2 pr;
						pr.x = __builtin_amdgcn_perm(v[k].y, v[k].x, sel);
						pr.y = __builtin_amdgcn_perm(v[k].w, v[k].z, sel);
						*reinterpret_cast<uint2 *>(d + c * PD) = pr;
					}
				}
			}
		}
	} else {
		RowWalker rw(tid, TPT, w);
		for (uint32_t i = tid; i < n; i += TPT, rw.next()) {
			const uint8_t *p = src + (size_t)rw.row * a.pitch + rw.col * (uint32_t)C;
			const uint32_t idx = rw.row * rs * 2u + rw.col;
			pl16[idx] = p[0];
			pl16[idx + 2u * PD] = p[1];
			pl16[idx + 4u * PD] = p[2];
			const uint32_t al = C == 4 ? p[3] : 255u;
			pl16[idx + 6u * PD] = (uint16_t)al;
			alpha_and &= al;
		}
	}
	tile_sync<NW>();

	auto gather_px = [&](uint32_t gx, uint32_t gy) -> uint32_t {
		const uint32_t idx = gy * rs * 2u + gx;
		return (uint32_t)pl16[idx] | ((uint32_t)pl16[idx + 2u * PD] << 8) | ((uint32_t)pl16[idx + 4u * PD] << 16) |
		       ((uint32_t)pl16[idx + 6u * PD] << 24);
	};
	// one output pixel into the slot of every rung of `mask`
	auto store_all = [&](uint64_t mask, uint32_t index, uint32_t px) {
		for (uint64_t mm = mask; mm != 0ull; mm &= mm - 1ull) store_pixel<C>(slot_of((uint32_t)__builtin_ctzll(mm)), index, px);
	};

	// ---- level 0 (and every level that keeps both sides): block.rs:279-281, a clone -- before the planes are premultiplied ----
	if (clone_mask != 0ull) {
		bool aligned8 = true;
		for (uint64_t mm = clone_mask; mm != 0ull; mm &= mm - 1ull)
			aligned8 = aligned8 && (reinterpret_cast<uintptr_t>(slot_of((uint32_t)__builtin_ctzll(mm))) & 7u) == 0;
		if (C == 4 && (w & 1u) == 0 && aligned8) {
			const uint32_t P2 = w >> 1;
			RowWalker rw(tid, TPT, P2);
			for (uint32_t i = tid; i < P2 * h; i += TPT, rw.next()) {
				const uint32_t *p = s_pl + rw.row * rs + rw.col;
				const uint32_t rg = __builtin_amdgcn_perm(p[PD], p[0], 0x06020400u);          // r0 g0 r1 g1
				const uint32_t ba = __builtin_amdgcn_perm(p[3 * PD], p[2 * PD], 0x06020400u);  // b0 a0 b1 a1
				uint2 o;
				o.x = __builtin_amdgcn_perm(ba, rg, 0x05040100u);
				o.y = __builtin_amdgcn_perm(ba, rg, 0x07060302u);
				for (uint64_t mm = clone_mask; mm != 0ull; mm &= mm - 1ull)
					reinterpret_cast<uint2 *>(slot_of((uint32_t)__builtin_ctzll(mm)))[i] = o;
			}
		} else {
			RowWalker rw(tid, TPT, w);
			for (uint32_t i = tid; i < n; i += TPT, rw.next()) store_all(clone_mask, i, gather_px(rw.col, rw.row));
		}
	}
	if (pending == 0ull) return;

	// ResizeAlg::Convolution, default ResizeOptions: U8x4 is alpha-premultiplied first (once for all levels; the clones above
	// read the planes as they came).  Opaque tiles take the weight-sum shortcut for alpha instead.
	bool opaque = true;
	if (a.filter != 0) {
		if constexpr (C == 4) {
			alpha_and = wave_and_sgpr(alpha_and);
			if constexpr (NW > 1) {
				const uint32_t wv = threadIdx.x / 64u;
				if ((threadIdx.x & 63u) == 0) s_red[wv] = alpha_and;
				__syncthreads();
#pragma unroll
				for (int q = 0; q < NW; ++q) alpha_and &= s_red[q];
			}
			opaque = alpha_and == 0xffu;
			if (!opaque) {
				const uint32_t P2 = (w + 1) >> 1;
				RowWalker rw(tid, TPT, P2);
				for (uint32_t i = tid; i < P2 * h; i += TPT, rw.next()) {
					uint32_t *p = s_pl + rw.row * rs + rw.col;
					const uint32_t al = p[3 * PD];
#pragma unroll
					for (int c = 0; c < 3; ++c) {
						const uint32_t v = p[c * PD];
						p[c * PD] = mul_div_255(v & 0xffffu, al & 0xffffu) | (mul_div_255(v >> 16, al >> 16) << 16);
					}
				}
				tile_sync<NW>();
			}
		}
	}
	const uint32_t nch = opaque ? 3u : 4u;  // channels that need taps

	// ---- one resample per distinct level, stored to every rung at that level ----
	while (pending != 0ull) {
		const uint32_t r0 = (uint32_t)__builtin_ctzll(pending);
		const uint32_t lm = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)r0);
		const uint64_t mask = __builtin_amdgcn_ballot_w64(live && m == lm) & pending;
		pending &= ~mask;
		const uint32_t ow = reduced_size(w, lm), oh = reduced_size(h, lm);
		const uint32_t lx = lm < (uint32_t)kMaxLevel ? lm : (uint32_t)kMaxLevel - 1;
		const AxisTab tab_x = a.tabs[(0 * 2 + (w == a.bw ? 0 : 1)) * kMaxLevel + lx];
		const AxisTab tab_y = a.tabs[(1 * 2 + (h == a.bh ? 0 : 1)) * kMaxLevel + lx];

		if (a.filter == 0) {  // ResizeAlg::Nearest (mod.rs:277): pick, no alpha handling
			const uint16_t *sx = a.bounds + tab_x.bounds_off;
			const uint16_t *sy = a.bounds + tab_y.bounds_off;
			RowWalker rw(tid, TPT, ow);
			for (uint32_t i = tid; i < ow * oh; i += TPT, rw.next()) {
				const uint32_t gx = ow == w ? rw.col : sx[rw.col];
				const uint32_t gy = oh == h ? rw.row : sy[rw.row];
				store_all(mask, i, gather_px(gx, gy));
			}
			continue;  // (the planes are only read: no barrier between levels)
		}

		const bool need_h = ow != w, need_v = oh != h;
		const int prec_x = tab_x.precision, prec_y = tab_y.precision;
		const int32_t init_x = 1 << (prec_x - 1), init_y = 1 << (prec_y - 1);
		const uint16_t *bnd_x = a.bounds + tab_x.bounds_off, *bnd_y = a.bounds + tab_y.bounds_off;
		const uint32_t *cf_x = a.coeffs + tab_x.coeff_off, *cf_y = a.coeffs + tab_y.coeff_off;
		const int32_t *ks_x = a.ksums + tab_x.ksum_off, *ks_y = a.ksums + tab_y.ksum_off;
		const uint32_t hps = a.hps, TD = a.tmp_dw;

		if (need_h) {
			// horizontal pass: item = (output column, pair of rows); u8 results kept transposed
			const uint32_t HP = (h + 1) >> 1;
			RowWalker rw(tid, TPT, ow);
			for (uint32_t i = tid; i < ow * HP; i += TPT, rw.next()) {
				const uint32_t ox = rw.col, yp = rw.row;
				const uint32_t fq = bnd_x[2 * ox], nq = bnd_x[2 * ox + 1];
				const uint32_t *k = cf_x + ox * tab_x.wquads * 2u;
				const uint32_t *row = s_pl + (2 * yp) * rs + fq * 2u;
				int32_t acc[4][2];
#pragma unroll
				for (int c = 0; c < 4; ++c) acc[c][0] = acc[c][1] = init_x;
				for (uint32_t q = 0; q < nq; ++q) {
					const uint32_t k01 = k[2 * q], k23 = k[2 * q + 1];
#pragma unroll
					for (uint32_t c = 0; c < 4; ++c) {
						if (c < nch) {
							const uint2 da = *reinterpret_cast<const uint2 *>(row + c * PD + q * 2u);
							const uint2 db = *reinterpret_cast<const uint2 *>(row + c * PD + rs + q * 2u);
							acc[c][0] = dot2(da.y, k23, dot2(da.x, k01, acc[c][0]));
							acc[c][1] = dot2(db.y, k23, dot2(db.x, k01, acc[c][1]));
						}
					}
				}
				uint32_t o[4][2];
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					o[c][0] = clip8(acc[c][0], prec_x);
					o[c][1] = clip8(acc[c][1], prec_x);
				}
				if (opaque) o[3][0] = o[3][1] = clip8(init_x + 255 * ks_x[ox], prec_x);
				if (need_v) {
#pragma unroll
					for (uint32_t c = 0; c < 4; ++c)
						if (c < nch) s_tmp[c * TD + ox * hps + yp] = o[c][0] | (o[c][1] << 16);
				} else {
#pragma unroll
					for (uint32_t r = 0; r < 2; ++r) {
						const uint32_t y = 2 * yp + r;
						if (y < h) {
							uint32_t px = o[0][r] | (o[1][r] << 8) | (o[2][r] << 16) | (o[3][r] << 24);
							if constexpr (C == 4) px = unpremultiply(px);
							store_all(mask, y * ow + ox, px);
						}
					}
				}
			}
			if (need_v) {
				tile_sync<NW>();
				// vertical pass over the transposed planes: item = (output column, output row)
				RowWalker rv(tid, TPT, ow);
				for (uint32_t i = tid; i < ow * oh; i += TPT, rv.next()) {
					const uint32_t ox = rv.col, oy = rv.row;
					const uint32_t fq = bnd_y[2 * oy], nq = bnd_y[2 * oy + 1];
					const uint32_t *k = cf_y + oy * tab_y.wquads * 2u;
					const uint32_t *colp = s_tmp + ox * hps + fq * 2u;
					int32_t acc[4] = {init_y, init_y, init_y, init_y};
					for (uint32_t q = 0; q < nq; ++q) {
						const uint32_t k01 = k[2 * q], k23 = k[2 * q + 1];
#pragma unroll
						for (uint32_t c = 0; c < 4; ++c) {
							if (c < nch) {
								const uint2 d = *reinterpret_cast<const uint2 *>(colp + c * TD + q * 2u);
								acc[c] = dot2(d.y, k23, dot2(d.x, k01, acc[c]));
							}
						}
					}
					uint32_t al = clip8(acc[3], prec_y);
					if (opaque) {
						const int32_t ah = (int32_t)clip8(init_x + 255 * ks_x[ox], prec_x);
						al = clip8(init_y + ah * ks_y[oy], prec_y);
					}
					uint32_t px = clip8(acc[0], prec_y) | (clip8(acc[1], prec_y) << 8) | (clip8(acc[2], prec_y) << 16) | (al << 24);
					if constexpr (C == 4) px = unpremultiply(px);
					store_all(mask, i, px);
				}
				tile_sync<NW>();  // the next level writes the transposed planes again
			}
			continue;
		}
		{
			// vertical pass only (width kept): item = (pair of columns, output row) on the [y][x] planes
			const uint32_t P2 = (w + 1) >> 1;
			RowWalker rv(tid, TPT, P2);
			for (uint32_t i = tid; i < P2 * oh; i += TPT, rv.next()) {
				const uint32_t qx = rv.col, oy = rv.row;
				const uint32_t fq = bnd_y[2 * oy], nq = bnd_y[2 * oy + 1];
				const uint32_t *k = cf_y + oy * tab_y.wquads * 2u;
				const uint32_t *colp = s_pl + (fq * 4u) * rs + qx;
				int32_t acc[4][2];
#pragma unroll
				for (int c = 0; c < 4; ++c) acc[c][0] = acc[c][1] = init_y;
				for (uint32_t q = 0; q < nq; ++q) {
					const uint32_t k01 = k[2 * q], k23 = k[2 * q + 1];
#pragma unroll
					for (uint32_t c = 0; c < 4; ++c) {
						if (c < nch) {
							const uint32_t *p = colp + c * PD + (q * 4u) * rs;
							const uint32_t q0 = p[0], q1 = p[rs], q2 = p[2 * rs], q3 = p[3 * rs];
							// (row j, row j+1) pairs of the left / right column
							const uint32_t l01 = __builtin_amdgcn_perm(q1, q0, 0x05040100u), l23 = __builtin_amdgcn_perm(q3, q2, 0x05040100u);
							const uint32_t h01 = __builtin_amdgcn_perm(q1, q0, 0x07060302u), h23 = __builtin_amdgcn_perm(q3, q2, 0x07060302u);
							acc[c][0] = dot2(l23, k23, dot2(l01, k01, acc[c][0]));
							acc[c][1] = dot2(h23, k23, dot2(h01, k01, acc[c][1]));
						}
					}
				}
				uint32_t al0 = clip8(acc[3][0], prec_y), al1 = clip8(acc[3][1], prec_y);
				if (opaque) al0 = al1 = clip8(init_y + 255 * ks_y[oy], prec_y);
#pragma unroll
				for (uint32_t r = 0; r < 2; ++r) {
					const uint32_t gx = 2 * qx + r;
					if (gx < w) {
						uint32_t px = clip8(acc[0][r], prec_y) | (clip8(acc[1][r], prec_y) << 8) | (clip8(acc[2][r], prec_y) << 16) |
						              ((r ? al1 : al0) << 24);
						if constexpr (C == 4) px = unpremultiply(px);
						store_all(mask, oy * w + gx, px);
					}
				}
			}
		}
	}
}

// One tile per block (NW waves), grid-stride over the batch.
template <int NW, int C>
__global__ void __launch_bounds__(64 * NW) ladder_kernel(const LadderArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		ladder_tile<NW, C>(a, tile_g, lds, lds + a.tile_dw, threadIdx.x);
		__syncthreads();  // the next tile reuses the LDS image
	}
}

template <int NW, int C>
static hipError_t launch_ladder_nw(const LadderArgs &a, uint32_t n_cus, hipStream_t stream)
{
	auto kernel = ladder_kernel<NW, C>;
	const uint32_t lds_bytes = (a.out_px ? a.tile_dw * 4u : 0u) + 16u * NW;  // (values and sizes only: no tile image)
	if (lds_bytes > 64u * 1024u) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
		if (e != hipSuccess) return e;
	}
	// as many blocks as fit the CUs' LDS four times over (the rest walk the grid-stride loop)
	const uint32_t per_cu = (160u * 1024u) / lds_bytes > 0 ? (160u * 1024u) / lds_bytes : 1u;
	const uint64_t cap = (uint64_t)n_cus * per_cu * 4u;
	const uint32_t blocks = (uint32_t)(a.n_tiles < cap ? a.n_tiles : cap);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * NW), lds_bytes, stream, a);
	return hipGetLastError();
}

template <int NW>
static hipError_t launch_ladder_c(const LadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	return channels == 4 ? launch_ladder_nw<NW, 4>(a, n_cus, stream) : launch_ladder_nw<NW, 3>(a, n_cus, stream);
}

// waves per tile as the generic kernel picks them (waves_per_tile)
hipError_t launch_ladder(const LadderArgs &a, uint32_t channels, uint32_t nw, uint32_t n_cus, hipStream_t stream)
{
	switch (nw) {
	case 1: return launch_ladder_c<1>(a, channels, n_cus, stream);
	case 2: return launch_ladder_c<2>(a, channels, n_cus, stream);
	case 4: return launch_ladder_c<4>(a, channels, n_cus, stream);
	case 8: return launch_ladder_c<8>(a, channels, n_cus, stream);
	default: return launch_ladder_c<16>(a, channels, n_cus, stream);
	}
}

}  // namespace pxz
