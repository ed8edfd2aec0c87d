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
// Steps 3 to 6 are varied_ladder_tail (pxz_varied_tile.h), which reshrink_ladder_kernel runs too.
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

// ---- this kernel's copy of varied_kernel's staging (pxz_varied_tile.h says why)

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

		// ---- 3.-6. the rungs: decisions, clones, the premultiply, resamples, stores (pxz_varied_tile.h)
		varied_ladder_tail<C>(a, la.factors, n_rungs, tile_g, w, h, x, shz, svr, s_key, s_x, s_a, s_f, tid);
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_varied_ladder(const VariedLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.v.n_tiles == 0u || a.n_factors == 0u) return hipSuccess;
	const uint32_t lds = varied_ladder_lds(a.v.mode, a.v.bw, a.v.bh, channels).total;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.v.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(varied_ladder_kernel<4>) : go(varied_ladder_kernel<3>);
}

uint32_t varied_ladder_lds_limit_bytes(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t channels)
{
	return varied_ladder_lds(mode, bw, bh, channels).total;
}

}  // namespace pxz
