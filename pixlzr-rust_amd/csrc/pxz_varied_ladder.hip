// pxz_varied_ladder.hip -- a batch of differently sized images at several factors in one launch
// (pxz_shrink_varied_ladder_frames_device).  The flat tile space, the owner search and the per-tile arithmetic are those of
// varied_kernel (pxz_varied.hip); what changes is how often each step runs.  The detector's raw result does not depend on the
// factor -- shrink_by decides on parse_value((x * k) * 10), shrink_directionally on parse_value((float)(sum / dfac) * k) --
// so a tile is staged and measured once and only the decision runs per rung.
//
// varied_ladder_kernel: one tile per block of 256 threads (grid-stride over the batch).  A tile is
//   1. staged      as in varied_kernel;
//   2. measured    once: x = total / count, or the two integer sums and their divisor;
//   3. decided     per rung, by thread r for rung r: levels, sizes and value go to index r * n_tiles + tile, and the pair of
//                  levels that shrink (0 for an axis that keeps its size) goes to LDS, where every wave reads the same keys;
//   4. cloned      to the slot of every rung that keeps both sizes -- before the tile is premultiplied;
//   5. premultiplied once, in place (RGBA under a convolution, and only when some rung shrinks);
//   6. resampled   once per distinct pair of levels: horizontal pass X -> I, vertical pass I -> F (or X -> I alone, or X -> A
//                  alone), un-premultiplied where it ends and stored to the slot of every rung with that pair.
// X is never written after step 5, so it serves every pair.  LDS of one block (varied_ladder_lds):
//   [oklab tables, shrink_by only] [X: the tile] [A: the detector's planes, then I at its start and F behind I]
// with I = ceil(bw/2) * bh * C bytes (the widest horizontal result: reduced_size(w, m >= 1) <= ceil(w/2)), F = ceil(bw/2) *
// ceil(bh/2) * C, and a vertical-only result of at most bw * ceil(bh/2) * C bytes at the start of A.  A side of 1 is never
// resampled and takes no room.  Rung r of a tile equals varied_kernel at factors[r] bit for bit.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

// Where a block of varied_ladder_kernel keeps its images: byte offsets into its dynamic LDS, and their sum.  The kernel, its
// launcher and the host's limit check all take the layout from here.
struct VariedLadderLds {
	uint32_t x, a, f, total;
};

__host__ __device__ inline VariedLadderLds varied_ladder_lds(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t channels)
{
	auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
	const uint32_t hw = bw > 1u ? (bw + 1u) / 2u : 0u, hh = bh > 1u ? (bh + 1u) / 2u : 0u;
	const uint32_t i_bytes = up16(hw * bh * channels);
	const uint32_t hv = i_bytes + up16(hw * hh * channels), v_only = up16(bw * hh * channels);
	uint32_t a_bytes = hv > v_only ? hv : v_only;
	if (mode == 0u && a_bytes < kVariedPlaneBytes) a_bytes = kVariedPlaneBytes;
	if (a_bytes < 16u) a_bytes = 16u;
	VariedLadderLds l;
	l.x = mode == 0u ? kVariedTables * 4u : 0u;
	l.a = l.x + up16(bw * bh * channels);
	l.f = l.a + i_bytes;
	l.total = l.a + a_bytes;
	return l;
}

// ---- this kernel's copy of varied_kernel's staging (pxz_varied_tile.h says why; the detectors up to their raw results and the
// un-premultiply loop, which the re-shrink ladder runs too, are there)

// A tile of w x h pixels at src (rows pitch bytes apart) into LDS, tightly packed: 16-byte loads where its rows are
// aligned, dwords or bytes otherwise.
template <int C>
__device__ __forceinline__ void varied_stage(uint8_t *s_x, const uint8_t *src, uint32_t pitch, uint32_t w, uint32_t h, uint32_t tid)
{
	const uint32_t n = w * h;
	if (C == 4 && (w & 3u) == 0u && ((reinterpret_cast<uintptr_t>(src) | pitch) & 15u) == 0u) {
		const uint32_t qpr = w >> 2;
		uint4 *d = reinterpret_cast<uint4 *>(s_x);
		for (uint32_t i = tid; i < qpr * h; i += kVariedThreads) {
			const uint32_t row = i / qpr, col = i - row * qpr;
			d[i] = *reinterpret_cast<const uint4 *>(src + (size_t)row * pitch + col * 16u);
		}
	} else if (C == 4 && ((reinterpret_cast<uintptr_t>(src) | pitch) & 3u) == 0u) {
		uint32_t *d = reinterpret_cast<uint32_t *>(s_x);
		for (uint32_t i = tid; i < n; i += kVariedThreads) {
			const uint32_t row = i / w, col = i - row * w;
			d[i] = *reinterpret_cast<const uint32_t *>(src + (size_t)row * pitch + col * 4u);
		}
	} else {
		const uint32_t rb = w * (uint32_t)C;
		for (uint32_t i = tid; i < n * (uint32_t)C; i += kVariedThreads) {
			const uint32_t row = i / rb, col = i - row * rb;
			s_x[i] = src[(size_t)row * pitch + col];
		}
	}
}

template <int C>
__global__ void __launch_bounds__(kVariedThreads) varied_ladder_kernel(const VariedLadderArgs la)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	__shared__ uint32_t s_key[kVariedLadderMaxRungs];  // per rung: mx | my << 8 of the axes that shrink (0: a clone)
	const VariedArgs &a = la.v;
	const uint32_t tid = threadIdx.x, n_rungs = la.n_factors;
	const bool oklab = a.mode == 0u;
	const bool nearest = a.filter == 0u;
	const VariedLadderLds l = varied_ladder_lds(a.mode, a.bw, a.bh, (uint32_t)C);
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint8_t *s_x = reinterpret_cast<uint8_t *>(lds) + l.x;
	uint8_t *s_a = reinterpret_cast<uint8_t *>(lds) + l.a;  // I, or a vertical-only result
	uint8_t *s_f = reinterpret_cast<uint8_t *>(lds) + l.f;  // F
	float *s_plane = reinterpret_cast<float *>(s_a);        // [4][kVariedChunk] (the detector, before A holds a pass)
	if (oklab) {
		oklab_fill_tables(s_lms, s_alpha, s_scale, tid);
		__syncthreads();
	}

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		const VariedImage im = a.images[owner_of(a.images, a.n_images, tile_g, &VariedImage::tile0)];
		const uint32_t t = tile_g - im.tile0;
		const uint32_t ty = t / im.cols, tx = t - ty * im.cols;
		const uint32_t w = tx + 1u == im.cols ? im.edge_w : a.bw;  // split.rs:18
		const uint32_t h = ty + 1u == im.rows ? im.edge_h : a.bh;  // split.rs:19
		const uint32_t n = w * h;
		const uint8_t *src = a.base + im.offset + (size_t)(ty * a.bh) * im.pitch + (size_t)(tx * a.bw) * (uint32_t)C;

		// ---- 1. the tile into LDS, once
		varied_stage<C>(s_x, src, im.pitch, w, h, tid);
		__syncthreads();

		// ---- 2. the detector up to what the factor has not entered, once
		float x = 0.0f;
		uint32_t shz = 0, svr = 0;
		if (oklab) x = varied_oklab_raw<C>(s_x, n, s_lms, s_alpha, s_scale, s_plane, s_acc, tid);
		else varied_sobel_sums<C>(s_x, w, h, s_red, tid, shz, svr);

		// ---- 3. every rung's decision: thread r decides rung r
		if (tid < n_rungs) {
			const float k = la.factors[tid];
			float v0, v1;
			if (oklab) {
				v0 = v1 = parse_value((x * k) * 10.0f);  // pixlzr.rs:162 (BASE_FACTOR, :15), :177-178
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
			// ---- 4. the clones (block.rs:279-281), while X still holds the staged bytes
			bool shrinks = false;
			for (uint32_t r = 0; r < n_rungs; ++r) {
				if (s_key[r] == 0u) varied_store(slot_of(r), s_x, n * (uint32_t)C, tid);
				else shrinks = true;
			}
			if (shrinks) {
				__syncthreads();  // the clones have read X
				// ---- 5. ResizeAlg::Convolution, default options: U8x4 is alpha-premultiplied first
				if (C == 4 && !nearest) {
					uint32_t *p32 = reinterpret_cast<uint32_t *>(s_x);
					for (uint32_t i = tid; i < n; i += kVariedThreads) p32[i] = premultiply(p32[i]);
					__syncthreads();
				}
				// ---- 6. one resample per distinct pair of levels; X is only read
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

hipError_t launch_varied_ladder(const VariedLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.v.n_tiles == 0u || a.n_factors == 0u) return hipSuccess;
	const uint32_t lds = varied_ladder_lds(a.v.mode, a.v.bw, a.v.bh, channels).total;
	// as many blocks as the CUs' LDS holds (at most eight of four waves per CU); the rest walk the grid-stride loop
	uint32_t per_cu = (160u * 1024u) / lds;
	per_cu = per_cu < 1u ? 1u : (per_cu > 8u ? 8u : per_cu);
	const uint64_t cap = (uint64_t)n_cus * per_cu;
	const uint32_t blocks = (uint32_t)(a.v.n_tiles < cap ? a.v.n_tiles : cap);
	auto go = [&](auto kernel) { return launch_with_lds(kernel, blocks, kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(varied_ladder_kernel<4>) : go(varied_ladder_kernel<3>);
}

uint32_t varied_ladder_lds_limit_bytes(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t channels)
{
	return varied_ladder_lds(mode, bw, bh, channels).total;
}

}  // namespace pxz
