// pxz_fit.h -- which rung of a ladder an image takes under a budget (pxz_fit_select, pxz_fit_varied_ladder_device): the rule,
// written once for the host export (pxz_api.cpp) and fit_select_kernel (pxz_fit.hip).
//
// An image has n_factors rungs; rung r has a file length bytes(r) and a squared error sse(r) (the sum over its channels), both
// uint64_t.  One of the two is the CONSTRAINED quantity, the other the one to make small:
//   PXZ_FIT_BYTES  constrained: bytes   minimised: sse     ("at most `target` bytes, as good as they allow")
//   PXZ_FIT_SSE    constrained: sse     minimised: bytes   ("an error of at most `target`, as small as that allows")
// A rung is eligible when its constrained quantity is <= target.  Among the eligible rungs the choice is the smallest
// (minimised, constrained, r), compared in that order; when no rung is eligible it is the smallest (constrained, minimised, r)
// -- the rung that misses the target by the least -- and bit 0 of the flags is set.  The index r is the last key both times:
// neighbouring factors often give a tile the same pair of levels, hence the same length and error, so "the lower index" decides
// in ordinary use.  Integer comparisons only: the result does not depend on who computes it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PXZ_FIT_HD __host__ __device__
#else
#define PXZ_FIT_HD
#endif

namespace pxz {

constexpr uint32_t kFitBytes = 0;  // PXZ_FIT_BYTES
constexpr uint32_t kFitSse = 1;    // PXZ_FIT_SSE
constexpr uint32_t kFitMissed = 1; // bit 0 of an image's fit flags: no rung met the target

struct FitPick {
	uint32_t choice, flags;
};

// bytes_of(r), sse_of(r): the two quantities of rung r (each called once per rung).  n_factors >= 1.
template <class BytesOf, class SseOf>
PXZ_FIT_HD inline FitPick fit_pick(uint32_t n_factors, uint32_t criterion, uint64_t target, BytesOf bytes_of, SseOf sse_of)
{
	bool any = false;
	uint32_t in_r = 0, out_r = 0;          // the best eligible rung, and the best of all by the fallback's order
	uint64_t in_c = 0, in_m = 0, out_c = 0, out_m = 0;  // their constrained and minimised quantities
	for (uint32_t r = 0; r < n_factors; ++r) {
		const uint64_t b = bytes_of(r), s = sse_of(r);
		const uint64_t c = criterion == kFitBytes ? b : s, m = criterion == kFitBytes ? s : b;
		if (r == 0u || c < out_c || (c == out_c && m < out_m)) {
			out_r = r;
			out_c = c;
			out_m = m;
		}
		if (c <= target && (!any || m < in_m || (m == in_m && c < in_c))) {
			any = true;
			in_r = r;
			in_c = c;
			in_m = m;
		}
	}
	return any ? FitPick{in_r, 0u} : FitPick{out_r, kFitMissed};
}

// ---- the copy of one tile's valid bytes by the 64 lanes of a wave (gather_rungs_kernel, pxz_fit.hip)
// `bytes` bytes from s to d; lane = 0 .. 63, every lane of the wave calls it (on the host: once per lane, in any order --
// pxz_fit_check.cpp does, for every pair of alignments).  Every access is naturally aligned, and exactly [0, bytes) is written:
//   s and d congruent mod 16: bytes up to a dword, dwords up to a 16-byte line, 16-byte lines, then dwords and bytes;
//   congruent mod 4 only:     bytes, dwords, bytes;
//   otherwise:                bytes.
struct alignas(16) FitLine {
	uint32_t v[4];
};

// How gather_copy cuts [0, bytes): `at` bytes, n4a dwords, n16 16-byte lines, n4b dwords, then the bytes that are left (fewer
// than 4 unless wide is false: then everything moves as bytes and the counts are 0).  The dwords start at a multiple of 4 of
// both addresses and the lines at a multiple of 16 of both; pxz_fit_check.cpp holds every case against that.
struct GatherSplit {
	bool wide;
	uint32_t at, n4a, n16, n4b;
};

PXZ_FIT_HD inline GatherSplit gather_split(uintptr_t da, uintptr_t sa, uint32_t bytes)
{
	const uintptr_t rel = da ^ sa;
	GatherSplit g{(rel & 3u) == 0u, 0, 0, 0, 0};
	if (!g.wide) return g;
	// bytes up to the next dword of both
	g.at = (0u - (uint32_t)da) & 3u;
	g.at = g.at < bytes ? g.at : bytes;
	// dwords: all that is left, or, where both share their place in a 16-byte line, those up to the line (n4a), the lines
	// (n16) and the dwords behind them (n4b)
	g.n4a = (bytes - g.at) / 4u;
	if ((rel & 15u) == 0u) {
		const uint32_t lead = ((0u - ((uint32_t)da + g.at)) & 15u) / 4u;
		if (lead <= g.n4a) {
			g.n16 = (g.n4a - lead) / 4u;
			g.n4b = (g.n4a - lead) % 4u;
			g.n4a = lead;
		}
	}
	return g;
}

PXZ_FIT_HD inline void gather_copy(uint8_t *d, const uint8_t *s, uint32_t bytes, uint32_t lane)
{
	const GatherSplit g = gather_split(reinterpret_cast<uintptr_t>(d), reinterpret_cast<uintptr_t>(s), bytes);
	if (!g.wide) {
		for (uint32_t i = lane; i < bytes; i += 64u) d[i] = s[i];
		return;
	}
	if (lane < g.at) d[lane] = s[lane];
	const uint32_t *s4 = reinterpret_cast<const uint32_t *>(s + g.at);
	uint32_t *d4 = reinterpret_cast<uint32_t *>(d + g.at);
	for (uint32_t i = lane; i < g.n4a; i += 64u) d4[i] = s4[i];
	const FitLine *s16 = reinterpret_cast<const FitLine *>(s4 + g.n4a);
	FitLine *d16 = reinterpret_cast<FitLine *>(d4 + g.n4a);
	for (uint32_t i = lane; i < g.n16; i += 64u) d16[i] = s16[i];
	const uint32_t *s4b = reinterpret_cast<const uint32_t *>(s16 + g.n16);
	uint32_t *d4b = reinterpret_cast<uint32_t *>(d16 + g.n16);
	if (lane < g.n4b) d4b[lane] = s4b[lane];
	// the bytes behind the last dword (fewer than 4)
	const uint32_t done = g.at + 4u * (g.n4a + 4u * g.n16 + g.n4b);
	if (lane < bytes - done) d[done + lane] = s[done + lane];
}

}  // namespace pxz
