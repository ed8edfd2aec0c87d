// pxz_reshrink_ladder.hip -- stored tiles of a varied batch shrunk again at several factors in one launch
// (pxz_reshrink_varied_ladder_frames_device): reshrink_kernel (pxz_reshrink.hip) up to the detector's raw result, then
// varied_ladder_kernel (pxz_varied_ladder.hip) from the rungs' decisions on.  The expand and the detector do not depend on the
// factor, so a stored tile is expanded once and measured once; each rung only decides its levels, and the tile is resampled once
// per distinct pair of levels among its rungs.
//
// reshrink_ladder_kernel: one tile per block of 256 threads, grid-stride over the flat tile space of pxz_varied_layout, owners by
// owner_of (pxz_device.h), the grid of tile_blocks (pxz_launch.h).  A tile
//   1. reads      its stored size (tw, th) and, from its owner's grid, its full size (fw, fh);
//   2. is flagged and skipped when its stored size cannot be (zero, or beyond its place), as reshrink_kernel does it: status bit
//                 0, the image's flag, and for EVERY rung outputs 0 x 0 with value bits 0; every rung's slot is left as it was;
//   3., 4. is cloned in when it is stored at full size, or expanded otherwise: reshrink_tile_image (pxz_varied_tile.h).
//                 reshrink_kernel has an inline copy of these two steps (pxz_reshrink.hip says why).  X is the plane the result lies in;
//   5. is measured once: x = total / count, or the two integer sums (varied_oklab_raw, varied_sobel_sums);
//   6. is decided per rung, by thread r for rung r, cloned, premultiplied once and resampled once per distinct pair of levels:
//                 steps 3 to 6 of varied_ladder_kernel.  THIS KERNEL KEEPS ITS OWN COPY of varied_ladder_tail (pxz_varied_tile.h),
//                 unchanged in arithmetic: with the tile image and the tail both called as functions its shrink_by rows measured
//                 2-3.5 % slower, with either one alone they do not.  A fix to the tail there belongs here too.
// In place: tile t's stored size and slot are read only by the block of tile t, into registers and LDS and before its first store
// (barriers lie between), and rungs of 1 and above lie beyond the inputs, so rung 0 of out_w / out_h / out_px may be the input
// arrays.
//
// LDS of one block (reshrink_lds with the tile's channel count, pxz_varied_tile.h):
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
	const ReshrinkLds l = reshrink_lds(a.mode, a.bw, a.bh, (uint32_t)C, x.wdw);
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

		// ---- 3., 4. the tile image X, tightly packed, and the plane the expand leaves free: cloned in, or expanded
		const ReshrinkTileImage ti = reshrink_tile_image<C>(x, src, tw, th, w, h, s_p0, s_p1, s_wx, s_wy, tid);
		uint8_t *s_x = ti.x, *s_o = ti.free;
		uint8_t *s_a = l.own != 0u ? reinterpret_cast<uint8_t *>(lds) + l.own : s_o;  // I, or a vertical-only result
		uint8_t *s_f = s_a + l.f;                                                         // F
		float *s_plane = reinterpret_cast<float *>(s_a);                                  // [4][kVariedChunk] (the detector, before A holds a pass)

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
	const uint32_t lds = reshrink_lds(a.r.v.mode, a.r.v.bw, a.r.v.bh, channels, a.r.x.wdw).total;
	if (lds > kLdsPerCu) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.r.v.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(reshrink_ladder_kernel<4>) : go(reshrink_ladder_kernel<3>);
}

}  // namespace pxz
