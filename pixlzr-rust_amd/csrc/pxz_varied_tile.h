// pxz_varied_tile.h -- one tile's work in a block of 256 threads, written once for the four tile-per-block kernels of the flat
// tile space: varied_kernel (pxz_varied.hip), varied_ladder_kernel (pxz_varied_ladder.hip), reshrink_kernel (pxz_reshrink.hip)
// and reshrink_ladder_kernel (pxz_reshrink_ladder.hip).
//   all four:          the detector's LDS constants, varied_pixel, varied_pass (one resample pass along one axis), varied_store;
//   the two ladders:   the detectors up to their raw results (varied_oklab_raw, varied_sobel_sums) and varied_unpremultiply;
//   the re-shrinks:    the block's LDS layout (reshrink_lds: both kernels' launches and the host's limit check);
//   retile_kernel (pxz_retile.hip): its LDS layout (retile_lds), and of the above varied_pixel, varied_pass, varied_store and
//                      varied_unpremultiply; its partial tile expand and its detectors are copies of reshrink_kernel's;
//   retile_ladder_kernel (pxz_retile_ladder.hip): its LDS layout (retile_ladder_lds), the assembly of a destination tile
//                      (retile_assemble: retile_kernel's steps 1 to 3, which that kernel keeps inline), the two ladders' detectors
//                      and varied_ladder_tail;
//   retile_distortion_kernel (pxz_retile_distortion.hip): its LDS layout (retile_distortion_lds) and retile_assemble, twice;
//   reshrink_ladder_kernel: the tile image of a stored tile (reshrink_tile_image: clone-in, or varied_resize_tile of pxz_device.h
//                      by the whole block, and the RGB pack);
//   varied_ladder_kernel: everything behind the detector (varied_ladder_tail: the rungs' decisions, clones, resamples and
//                      stores).
// Every function is called by all 256 threads of the block.  What is still copied, and why (each copy says so where it stands):
// varied_kernel keeps its staging, the two detectors and the un-premultiply loop inline -- 101 -> 124 VGPRs as functions
// (DESIGN.md 8h); reshrink_kernel keeps the tile image and the detectors inline, and reshrink_ladder_kernel the ladder's tail --
// same registers, but measurably slower on the shared text.  A fix to the arithmetic here belongs there too.
#pragma once
#include "pxz_device.h"
#include "pxz_oklab_math.h"

namespace pxz {

constexpr uint32_t kVariedThreads = 256;
constexpr uint32_t kVariedTables = 3072u + 256u + 2u * 128u;  // dwords: matrix-column products, alpha / 255, scale factors
constexpr uint32_t kVariedChunk = 1024;                       // pixels the Oklab detector converts per round
constexpr uint32_t kVariedPlaneBytes = 4u * kVariedChunk * 4u;

__device__ __forceinline__ uint32_t varied_pixel(const uint8_t *s_x, uint32_t i, int C)
{
	if (C == 4) return reinterpret_cast<const uint32_t *>(s_x)[i];
	const uint8_t *p = s_x + i * 3u;
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | 0xff000000u;
}

// One pass of fir's convolution (or the nearest pick) along one axis of an image in LDS: `lines` lines of e.in samples of C
// bytes (sample stride sstep, line stride lstep) -> e.out samples per line (dst_ostep, dst_lstep).
template <int C>
__device__ __forceinline__ void varied_pass(const VariedArgs &a, const TreeAxisEntry &e, bool nearest, const uint8_t *src, uint32_t sstep,
                                            uint32_t lstep, uint8_t *dst, uint32_t dst_ostep, uint32_t dst_lstep, uint32_t lines, uint32_t tid)
{
	const uint32_t out = e.out;
	for (uint32_t i = tid; i < lines * out; i += kVariedThreads) {
		const uint32_t line = i / out, o = i - line * out;
		const uint8_t *s = src + line * lstep;
		uint8_t *d = dst + line * dst_lstep + o * dst_ostep;
		if (nearest) {
			const uint8_t *p = s + (uint32_t)a.starts[e.starts_off + o] * sstep;
#pragma unroll
			for (int c = 0; c < C; ++c) d[c] = p[c];
			continue;
		}
		const int32_t first = a.starts[e.starts_off + o], n = a.sizes[e.starts_off + o];
		const int16_t *k = a.coeffs + e.coeff_off + (size_t)o * e.window;
		int32_t acc[C];
#pragma unroll
		for (int c = 0; c < C; ++c) acc[c] = 1 << (e.precision - 1u);
		for (int32_t j = 0; j < n; ++j) {
			const uint8_t *p = s + (uint32_t)(first + j) * sstep;
			const int32_t kj = k[j];
#pragma unroll
			for (int c = 0; c < C; ++c) acc[c] += (int32_t)p[c] * kj;
		}
#pragma unroll
		for (int c = 0; c < C; ++c) d[c] = (uint8_t)clip8(acc[c], (int)e.precision);
	}
}

// LDS -> a tile's slot (bytes; dwords where the slot is 4-byte aligned)
__device__ __forceinline__ void varied_store(uint8_t *slot, const uint8_t *s, uint32_t bytes, uint32_t tid)
{
	uint32_t head = 0;
	if ((reinterpret_cast<uintptr_t>(slot) & 3u) == 0u) {
		head = bytes & ~3u;
		const uint32_t *s32 = reinterpret_cast<const uint32_t *>(s);
		uint32_t *d32 = reinterpret_cast<uint32_t *>(slot);
		for (uint32_t i = tid; i < head / 4u; i += kVariedThreads) d32[i] = s32[i];
	}
	for (uint32_t i = head + tid; i < bytes; i += kVariedThreads) slot[i] = s[i];
}

// ---- a tile measured up to what the factor has not entered, and the un-premultiply of a resampled image

// get_block_variance with |x - avg| (operations.rs:26-126) up to its raw result x = total / count, the same in every thread:
// the detector kernels' own colour conversion (pxz_oklab_math.h), 1024 pixels at a time into s_plane ([4][kVariedChunk]),
// and four lanes that add them up in pixel order, twice -- the two sequential f32 sums of the reference.  s_acc: 4 floats.
template <int C>
__device__ __forceinline__ float varied_oklab_raw(const uint8_t *s_x, uint32_t n, const float4 *s_lms, const float *s_alpha,
                                                  const double *s_scale, float *s_plane, float *s_acc, uint32_t tid)
{
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
	return __fdiv_rn(total, count);
}

// get_block_variance_directionally (operations.rs:192-259): the Sobel-like integer sums over the (w - 2) x (h - 2) interior,
// the same in every thread.  s_red: 2 dwords per wave.
template <int C>
__device__ __forceinline__ void varied_sobel_sums(const uint8_t *s_x, uint32_t w, uint32_t h, uint32_t *s_red, uint32_t tid, uint32_t &shz,
                                                  uint32_t &svr)
{
	shz = svr = 0;
	if (w > 2u && h > 2u) {
		const uint32_t iw = w - 2u, rb = w * (uint32_t)C;
		for (uint32_t i = tid; i < iw * (h - 2u); i += kVariedThreads) {
			const uint32_t y = i / iw, x = i - y * iw;
			const uint8_t *p0 = s_x + y * rb + x * (uint32_t)C, *p1 = p0 + rb, *p2 = p1 + rb;
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
}

// fir's un-premultiply of `count` RGBA pixels in LDS, in place (the reciprocal table's division)
__device__ __forceinline__ void varied_unpremultiply(uint32_t *p32, uint32_t count, uint32_t tid)
{
	for (uint32_t i = tid; i < count; i += kVariedThreads) {
		const uint32_t px = p32[i], al = px >> 24;
		const uint32_t rc = kRecipAlpha.v[al];
		uint32_t r = ((px & 255u) * rc + 128u) >> 8, g = (((px >> 8) & 255u) * rc + 128u) >> 8, b = (((px >> 16) & 255u) * rc + 128u) >> 8;
		r = r > 255u ? 255u : r;
		g = g > 255u ? 255u : g;
		b = b > 255u ? 255u : b;
		p32[i] = r | (g << 8) | (b << 16) | (al << 24);
	}
}

// ---- the re-shrinks: a stored tile back at its full size in LDS

// Where a block of reshrink_kernel or reshrink_ladder_kernel keeps its images: byte offsets into its dynamic LDS, and their sum
// (0xffffffff: a plane beyond the calls' limit).  The kernels, their launchers and the host's limit check all take the layout
// from here.  After reshrink_tile_image the tile image X is P0 or P1 and the other plane is free; it serves as A -- the
// detector's planes [4][kVariedChunk], then, in the ladder, the passes' I at its start and F behind I (varied_ladder_lds' sizes)
// -- unless A is larger than a plane: then A has a region of its own behind the windows.  rung_channels: the ladder's channel
// count, or 0 for reshrink_kernel, whose passes go from plane to plane and whose A holds the detector's planes only.
constexpr uint32_t kReshrinkMaxPlaneBytes = 65536;
struct ReshrinkLds {
	uint32_t p0, p1, wx;  // the two planes and the staged windows
	uint32_t own;         // A's own region, or 0: A is the plane the expand leaves free
	uint32_t f;           // F, from the start of A (= the room of I)
	uint32_t total;
};

__host__ __device__ inline ReshrinkLds reshrink_lds(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t rung_channels, uint32_t wdw)
{
	auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
	ReshrinkLds l{0, 0, 0, 0, 0, 0xffffffffu};
	const uint64_t plane64 = ((uint64_t)bw * bh * 4u + 15u) & ~(uint64_t)15u;
	if (bw == 0u || bh == 0u || plane64 > kReshrinkMaxPlaneBytes) return l;
	const uint32_t plane = (uint32_t)plane64;
	// A: the widest horizontal result I and the result F behind it, or a vertical-only result (varied_ladder_lds)
	const uint32_t hw = bw > 1u ? (bw + 1u) / 2u : 0u, hh = bh > 1u ? (bh + 1u) / 2u : 0u;
	const uint32_t i_bytes = up16(hw * bh * rung_channels);
	const uint32_t hv = i_bytes + up16(hw * hh * rung_channels), v_only = up16(bw * hh * rung_channels);
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

// ---- the re-tile: a destination tile's image assembled from parts of source tiles (retile_kernel, pxz_retile.hip)
//
// Where a block of retile_kernel keeps its images: byte offsets into its dynamic LDS, and their sum (0xffffffff: a plane beyond
// the limit below).  The kernel, its launch and the host's limit check (pxz_retile_lds_bytes, the entry point, the host form)
// all take the layout from here.
//   [oklab tables, shrink_by only: 14 336 B] [X: D = dbw * dbh * 4, rounded up to 16] [U]
// X is the destination tile image: one dword per pixel while it is assembled, then C bytes per pixel (RGB is packed in place).
// U is one region with two lives.  During the assembly it holds, for one covering source tile at a time,
//   [the staged stored pixels: pw x ph dwords] [the horizontal pass's intermediate: cwmax x ph dwords]
//   [the windows of both SOURCE axes: (sbw + sbh) * wdw dwords]
// Only the stored pixels that the wanted part's windows read are staged -- a rectangle of the stored tile -- so the staging is
// bounded by the part, not by the source block: a part is at most cwmax = min(sbw, dbw) by chmax = min(sbh, dbh) samples, the
// windows of n consecutive samples of an up-scaling table span at most n + (widest window) stored samples (a window starts at
// most one sample after its neighbour's), and the widest window has at most 2 (wdw - 1) taps; with two samples to spare
//   pw = min(sbw, cwmax + 2 (wdw - 1) + 2),  ph = min(sbh, chmax + 2 (wdw - 1) + 2).
// After the assembly U is X's other plane (D bytes: what the shrink's passes alternate with) and, in shrink_by mode, the
// detector's planes (16 KB), one over the other as in reshrink_kernel with large planes: the detector is done before the first
// pass writes.  So U = max(assembly, D, 16 KB in shrink_by mode).  The shrink's windows are not staged: varied_pass reads them
// from the tables, as in the re-shrink.
// Limit: D <= 65536 and sbw * sbh * 4 <= 65536 (either beyond: 0xffffffff), and the sum within the CU's 160 KB.  With Lanczos3
// (wdw = 5) that admits equal square blocks up to 109x109 on both sides in shrink_by mode, and a 128x128 block on one side with
// a square block of up to 99x99 on the other; 128x128 <-> 128x127 does not fit (a part can then be nearly the whole source
// tile: 64 KB staged, 64 KB of intermediate), nor does a one-row block of 16384 (its windows alone).  Destination blocks of
// 32x32 and 48x20 take 34-35 KB in shrink_by mode whatever the source block up to 64x64: four blocks per CU, as varied_kernel.
constexpr uint32_t kRetileMaxPlaneBytes = 65536;
struct RetileLds {
	uint32_t x, u;       // the destination tile image; the region of the assembly / of the other plane and the detector's planes
	uint32_t pw, ph;     // the staged rectangle's bounds (samples)
	uint32_t inter;      // the intermediate, from the start of the dynamic LDS
	uint32_t wx;         // the staged windows: x's sbw entries, then y's sbh entries, wdw dwords each
	uint32_t total;
};

__host__ __device__ inline RetileLds retile_lds(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t wdw)
{
	auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
	auto lesser = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
	RetileLds l{0, 0, 0, 0, 0, 0, 0xffffffffu};
	const uint64_t d64 = ((uint64_t)dbw * dbh * 4u + 15u) & ~(uint64_t)15u, s64 = (uint64_t)sbw * sbh * 4u;
	if (sbw == 0u || sbh == 0u || dbw == 0u || dbh == 0u || wdw == 0u || wdw > 64u || d64 > kRetileMaxPlaneBytes || s64 > kRetileMaxPlaneBytes) return l;
	const uint32_t d = (uint32_t)d64;
	const uint32_t cwmax = lesser(sbw, dbw), chmax = lesser(sbh, dbh);
	l.pw = lesser(sbw, cwmax + 2u * (wdw - 1u) + 2u);
	l.ph = lesser(sbh, chmax + 2u * (wdw - 1u) + 2u);
	l.x = mode == 0u ? kVariedTables * 4u : 0u;
	l.u = l.x + d;
	l.inter = l.u + up16(l.pw * l.ph * 4u);
	l.wx = l.inter + up16(cwmax * l.ph * 4u);
	uint32_t u_bytes = l.wx + (((sbw + sbh) * wdw + 3u) & ~3u) * 4u - l.u;  // (sides of at most 16384, wdw of at most 64)
	if (u_bytes < d) u_bytes = d;
	if (mode == 0u && u_bytes < kVariedPlaneBytes) u_bytes = kVariedPlaneBytes;
	l.total = l.u + u_bytes;
	return l;
}

// ---- the re-tile ladder: the same assembly, then the ladder's tail (retile_ladder_kernel, pxz_retile_ladder.hip)
//
// Where a block of retile_ladder_kernel keeps its images: byte offsets into its dynamic LDS, and their sum (0xffffffff beyond
// retile_lds' own limits: D or sbw * sbh * 4 above 65536).  The kernel, its launch and the host's limit check
// (pxz_retile_ladder_lds_bytes, the entry point, the host form) all take the layout from here.
//   [oklab tables, shrink_by only: 14 336 B] [X: D = dbw * dbh * 4, rounded up to 16] [U]
// X is the destination tile image as in retile_lds.  During the assembly U is what retile_lds lays out (staged pixels,
// intermediate, windows of both source axes, at the same offsets).  Afterwards U is the ladder's A: the detector's planes
// [4][kVariedChunk] (16 KB, shrink_by only), then the passes' I at its start and F behind I -- reshrink_lds' sizes for the
// destination block and the channel count.  varied_ladder_tail goes X -> I -> F and never writes X after the premultiply, so
// X's other plane is not needed: U = max(assembly, A).  Wherever A <= D that is at most the one-factor re-tile's footprint;
// only tiny blocks have A > D (a 3x5 RGBA block: I + F = 48 + 32 bytes beside D = 64).
struct RetileLadderLds {
	uint32_t x, u;       // the destination tile image; the region of the assembly, then A
	uint32_t pw, ph;     // the staged rectangle's bounds (samples)
	uint32_t inter;      // the intermediate, from the start of the dynamic LDS
	uint32_t wx;         // the staged windows: x's sbw entries, then y's sbh entries, wdw dwords each
	uint32_t f;          // F, from the start of U (= the room of I)
	uint32_t total;
};

__host__ __device__ inline RetileLadderLds retile_ladder_lds(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t channels,
                                                             uint32_t wdw)
{
	auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
	const RetileLds r = retile_lds(mode, sbw, sbh, dbw, dbh, wdw);
	RetileLadderLds l{r.x, r.u, r.pw, r.ph, r.inter, r.wx, 0, 0xffffffffu};
	if (r.total == 0xffffffffu) return l;
	// A: the widest horizontal result I and the result F behind it, or a vertical-only result (reshrink_lds, varied_ladder_lds)
	const uint32_t hw = dbw > 1u ? (dbw + 1u) / 2u : 0u, hh = dbh > 1u ? (dbh + 1u) / 2u : 0u;
	const uint32_t i_bytes = up16(hw * dbh * channels);
	const uint32_t hv = i_bytes + up16(hw * hh * channels), v_only = up16(dbw * hh * channels);
	uint32_t a_bytes = hv > v_only ? hv : v_only;
	if (mode == 0u && a_bytes < kVariedPlaneBytes) a_bytes = kVariedPlaneBytes;  // the detector's planes
	uint32_t u_bytes = r.wx + (((sbw + sbh) * wdw + 3u) & ~3u) * 4u - r.u;  // the assembly (retile_lds)
	if (u_bytes < a_bytes) u_bytes = a_bytes;
	l.f = i_bytes;
	l.total = l.u + u_bytes;
	return l;
}

// ---- the re-tile distortion: two assemblies of one destination tile, compared (retile_distortion_kernel, pxz_retile_distortion.hip)
//
// Where a block of retile_distortion_kernel keeps its images: byte offsets into its dynamic LDS, and their sum (0xffffffff beyond
// retile_lds' own limits: D or sbw * sbh * 4 above 65536).  The kernel, its launch and the host's limit check
// (pxz_retile_distortion_lds_bytes, the entry point, the host forms) all take the layout from here.
//   [R: D = dbw * dbh * 4, rounded up to 16] [E: D] [S]
// R is the reference -- the destination tile of what the archive decodes to, assembled from the SOURCE tiles that cover it -- and E
// one set's stored tile of the destination layout at its full size; each is a dword per pixel while it is assembled and C bytes
// per pixel, tightly packed, when it is compared.  S is the staging of retile_assemble, one region for both sides, laid out as
// retile_lds lays out the assembly (staged pixels, intermediate, windows of both axes) for
//   the source side: source blocks sbw x sbh -> parts of a dbw x dbh tile, windows of wdw_src dwords (expand_filter's tables);
//   the set side:    "source" blocks dbw x dbh -> the whole dbw x dbh tile, windows of wdw_set dwords (filter_up's tables);
// each side at its own offsets and its own window stride, S as large as the larger of the two needs.
// Limit: the sum within the CU's 160 KB.  The set side stages a whole stored tile (up to D), its intermediate (up to D) and the
// windows of both axes, so equal square blocks of side n with Lanczos3 on both sides (both strides 5) take 16 n^2 + 40 n bytes
// and what rounds each region up to 16: up to 99x99 (160 832 bytes); 100x100 is beyond (164 000), and fits only with Nearest on
// both sides (161 600).  Destination blocks of 32x32 take 16.5-22.6 KB whatever the source block up to 64x64 (seven blocks a CU
// and more), 64x64 ones 65-66.5 KB (two).
struct RetileDistortionLds {
	uint32_t r, e, s;                      // the two planes and the staging
	uint32_t src_inter, src_wx;            // the source side's intermediate and windows, from the start of the dynamic LDS
	uint32_t set_inter, set_wx;            // the set side's
	uint32_t total;
};

__host__ __device__ inline RetileDistortionLds retile_distortion_lds(uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t wdw_src,
                                                                     uint32_t wdw_set)
{
	RetileDistortionLds l{0, 0, 0, 0, 0, 0, 0, 0xffffffffu};
	const RetileLds a = retile_lds(1u, sbw, sbh, dbw, dbh, wdw_src), b = retile_lds(1u, dbw, dbh, dbw, dbh, wdw_set);
	if (a.total == 0xffffffffu || b.total == 0xffffffffu) return l;
	const uint32_t d = a.u;  // (mode 1: X stands at 0 and U behind it, D bytes on)
	const uint32_t need_a = a.wx + (((sbw + sbh) * wdw_src + 3u) & ~3u) * 4u - a.u;
	const uint32_t need_b = b.wx + (((dbw + dbh) * wdw_set + 3u) & ~3u) * 4u - b.u;
	l.r = 0u;
	l.e = d;
	l.s = 2u * d;
	l.src_inter = l.s + (a.inter - a.u);
	l.src_wx = l.s + (a.wx - a.u);
	l.set_inter = l.s + (b.inter - b.u);
	l.set_wx = l.s + (b.wx - b.u);
	l.total = l.s + (need_a > need_b ? need_a : need_b);
	return l;
}

// retile_kernel's steps 1 to 3 (pxz_retile.hip, where they are described) for the destination tile whose rectangle is
// [X0, X0 + w) x [Y0, Y0 + h) of an image whose SOURCE grid is sm: the covering source tiles, the assembly in s_img (one dword per
// pixel, rows w apart; s_src, s_tmp, s_wx, s_wy: the staging of retile_lds), and the pack to C bytes per pixel in place.  Returns
// true ("bad") when a covering tile's stored size cannot be: the assembly stops there and s_img holds nothing of use.  Ends in a
// barrier either way.  retile_kernel KEEPS ITS OWN INLINE TEXT of these steps (its timing is pinned in DESIGN.md 8o; 8k showed
// what a call can cost): A FIX HERE BELONGS THERE TOO, and the other way round -- and to the expand arithmetic of
// varied_resize_tile (pxz_device.h) and reshrink_kernel step 4, from which both are copied.
template <int C>
__device__ __forceinline__ bool retile_assemble(const TileResizeArgs &x, const VariedImage &sm, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                                                uint32_t *s_img, uint32_t *s_src, uint32_t *s_tmp, uint32_t *s_wx, uint32_t *s_wy, uint32_t tid)
{
	const bool conv = x.filter != 0u;
	const uint32_t n = w * h;
	// ---- 1. the source tiles that cover the rectangle
	const uint32_t X1 = X0 + w, Y1 = Y0 + h;
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
		const uint32_t pw = rx1 - rx0, ph = ry1 - ry0;  // (within the layout's pw x ph: retile_lds)
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
	__syncthreads();  // X is whole -- or, bad: threads still behind may be cloning into X, which the next tile writes
	if (bad) return true;

	// ---- 3. the tile image as varied_kernel stages it: C bytes per pixel, tightly packed, in X
	if constexpr (C == 3) {
		// RGB: the dwords packed to 3 bytes in place, 1024 pixels a round (four per thread as three dwords, bytes at the tail): a
		// round writes below what later rounds read, and the barrier keeps its own reads ahead of its writes
		uint8_t *s_x = reinterpret_cast<uint8_t *>(s_img);
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
	return false;
}

// The tile image of stored tile (tw x th at src, tightly packed) of full size w x h, in the planes p0 / p1 of the block's LDS:
// C bytes per pixel, tightly packed, as varied_kernel stages a tile.  Stored at full size it is cloned in (block.rs:279-281; 16-,
// 4- or 1-byte loads by the slot's alignment); otherwise varied_resize_tile (pxz_device.h) expands it, by the whole block, to one
// dword per pixel, and RGB is packed to 3 bytes into the other plane.  x: the image; free: the other plane.  Ends in a barrier.
struct ReshrinkTileImage {
	uint8_t *x, *free;
};

template <int C>
__device__ __forceinline__ ReshrinkTileImage reshrink_tile_image(const TileResizeArgs &x, const uint8_t *src, uint32_t tw, uint32_t th, uint32_t w,
                                                                 uint32_t h, uint8_t *s_p0, uint8_t *s_p1, uint32_t *s_wx, uint32_t *s_wy, uint32_t tid)
{
	const uint32_t n = w * h;
	if (tw == w && th == h) {
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
		__syncthreads();
		return {s_p0, s_p1};
	}
	uint32_t *s_src = reinterpret_cast<uint32_t *>(s_p0), *s_tmp = reinterpret_cast<uint32_t *>(s_p1);
	uint32_t *out = const_cast<uint32_t *>(
		varied_resize_tile<C, kVariedThreads>(x, tid, src, tw, th, w, h, s_src, s_tmp, s_wx, s_wy, true, true, [] { __syncthreads(); }));
	uint32_t *other = out == s_src ? s_tmp : s_src;
	if constexpr (C == 4) {
		return {reinterpret_cast<uint8_t *>(out), reinterpret_cast<uint8_t *>(other)};
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
		__syncthreads();
		return {ob, reinterpret_cast<uint8_t *>(out)};
	}
}

// ---- the ladders: everything behind the detector (steps 3 to 6 of varied_ladder_kernel, pxz_varied_ladder.hip)
// Tile tile_g of w x h pixels, its image in X and its raw detector result in x (shrink_by) or shz / svr (directional), the same in
// every thread.  Thread r decides rung r with factors[r]: value and sizes go to index r * n_tiles + tile_g, the pair of levels
// that shrink (0 for an axis that keeps its size) to s_key[r], where every wave reads the same keys.  Then the clones, to the slot
// of every rung that keeps both sizes, before X is premultiplied; the premultiply, once and in place (RGBA under a convolution,
// and only when some rung shrinks); and one resample per distinct pair of levels -- X -> I -> F, or X -> I alone, or X -> A alone,
// with I at the start of A -- un-premultiplied where it ends and stored to the slot of every rung with that pair.  X is never
// written after the premultiply, so it serves every pair.  Does not end in a barrier.
template <int C>
__device__ __forceinline__ void varied_ladder_tail(const VariedArgs &a, const float *factors, uint32_t n_rungs, uint32_t tile_g, uint32_t w,
                                                   uint32_t h, float x, uint32_t shz, uint32_t svr, uint32_t *s_key, uint8_t *s_x, uint8_t *s_a,
                                                   uint8_t *s_f, uint32_t tid)
{
	const uint32_t n = w * h;
	const bool nearest = a.filter == 0u;
	// ---- 3. every rung's decision: thread r decides rung r
	if (tid < n_rungs) {
		const float k = factors[tid];
		float v0, v1;
		if (a.mode == 0u) {
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
	if (a.out_px == nullptr) return;

	auto slot_of = [&](uint32_t r) { return a.out_px + ((uint64_t)r * a.n_tiles + tile_g) * (uint64_t)a.slot_bytes; };
	// ---- 4. the clones (block.rs:279-281), while X still holds the tile's bytes
	bool shrinks = false;
	for (uint32_t r = 0; r < n_rungs; ++r) {
		if (s_key[r] == 0u) varied_store(slot_of(r), s_x, n * (uint32_t)C, tid);
		else shrinks = true;
	}
	if (!shrinks) return;
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

}  // namespace pxz
