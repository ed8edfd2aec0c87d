// pxz_tilefit.h -- which rung of a ladder each TILE takes under a budget of its group (pxz_fit_tiles_select,
// pxz_fit_varied_tiles_device): the rule, written once for the host export (pxz_api.cpp), the kernels of pxz_tilefit.hip and
// the stand-alone check (pxz_tilefit_check.cpp).
//
// A group is a run of flat tiles (the tiles of consecutive images) with `fixed` bytes of headers and line tables and one target.
// Tile t has n_factors candidates; candidate (t, r) has b = its record's bytes (u32) and s = the sum over its channels of its
// squared error.  It is USABLE when no channel sum is all-ones, s < 2^32 and b < 2^24 (tilefit_pack: such a candidate is one
// u64, s in bits 24..55 and b in bits 0..23; every other is kTileFitUnusable).  Unusable candidates are skipped; a tile without a
// usable one gets choice 0, counts in no total and sets kTileFitNoCandidate.
//
//   pick(t, lambda) = the usable r with the smallest (s + lambda * b, b, r), lambda an integer in [0, kTileFitLambdaMax = 2^32]
//   B(lambda) = fixed + sum over the group's tiles of b(pick),   S(lambda) = the sum of s(pick)
// All arithmetic is u64: s + lambda * b < 2^32 + 2^32 * 2^24 < 2^57.  At lambda = 2^32 a byte outweighs any error, so every
// tile takes its fewest bytes; at lambda = 0 its least error.
//
// B never increases with lambda and S never decreases, whatever the ties: for lambda1 < lambda2 let tile t pick (s1, b1) at
// lambda1 and (s2, b2) at lambda2.  Each is optimal where it was picked: s1 + lambda1 b1 <= s2 + lambda1 b2 and
// s2 + lambda2 b2 <= s1 + lambda2 b1.  Added up: (lambda2 - lambda1) (b2 - b1) <= 0, so b2 <= b1 -- and then the first
// inequality gives s1 - s2 <= lambda1 (b2 - b1) <= 0, so s1 <= s2.  (With equal costs the second key, b, and the third, r, make
// the pick a function of lambda; the two inequalities hold for any minimiser.)  Tile by tile, hence for the sums.  The
// bisections below, and the tests, lean on that.
//
//   PXZ_FIT_BYTES  lambda* = the smallest lambda with B(lambda) <= target; B(2^32) > target: lambda* = 2^32 and kTileFitMissed --
//                  no assignment of rungs fits then, for B(2^32) is every tile's fewest bytes.
//   PXZ_FIT_SSE    lambda* = the largest lambda with S(lambda) <= target; S(0) > target: lambda* = 0 and kTileFitMissed.
// Either is found by kTileFitSteps = 33 halvings of [0, 2^32] (tilefit_mid, tilefit_advance), each of which needs one total of
// the group at one lambda: on the device one launch, with the interval in device memory.
//
// A Lagrangian pick is optimal for the bytes it uses, but it can lose to one rung for the whole group that sits closer under
// the target.  So, when the target was not missed, the uniform totals (B_u(r), S_u(r)) over the rungs usable for EVERY tile of
// the group go through fit_pick (pxz_fit.h), and the uniform rung is taken when it is eligible and its (minimised, constrained)
// pair is strictly smaller than the Lagrangian's: every tile of the group then takes that rung and kTileFitUniform is set
// (tilefit_decide).  Integer comparisons only: the host and the device cannot disagree.
#pragma once
#include <cstdint>

#include "pxz_fit.h"

namespace pxz {

constexpr uint64_t kTileFitLambdaMax = 1ull << 32;  // PXZ_TILEFIT_LAMBDA_MAX
constexpr uint32_t kTileFitSteps = 33;              // halvings that bring [0, 2^32] down to one value
constexpr uint64_t kTileFitUnusable = ~0ull;        // a packed candidate that is skipped
constexpr uint32_t kTileFitNoCandidate = 2;         // bit 1 of a group's flags: a tile of it has no usable candidate
constexpr uint32_t kTileFitUniform = 4;             // bit 2: the group took one rung for all its tiles
// (bit 0 is kFitMissed of pxz_fit.h)

// candidate (t, r) as one u64; sse: the candidate's `channels` sums
PXZ_FIT_HD inline uint64_t tilefit_pack(uint32_t bytes, const uint64_t *sse, uint32_t channels)
{
	uint64_t s = 0;
	for (uint32_t c = 0; c < channels; ++c) {
		if (sse[c] >= (1ull << 32)) return kTileFitUnusable;  // (all-ones among them; the sum below cannot wrap)
		s += sse[c];
	}
	if (s >= (1ull << 32) || bytes >= (1u << 24)) return kTileFitUnusable;
	return (s << 24) | bytes;
}
PXZ_FIT_HD inline uint64_t tilefit_s(uint64_t cand) { return cand >> 24; }
PXZ_FIT_HD inline uint64_t tilefit_b(uint64_t cand) { return cand & 0xffffffull; }

struct TilePick {
	bool any;      // false: no usable candidate (choice 0, s = b = 0)
	uint32_t r;
	uint64_t s, b;
};

// cand_of(r): the packed candidate of rung r of one tile (called once per rung)
template <class CandOf>
PXZ_FIT_HD inline TilePick tilefit_pick(uint32_t n_factors, uint64_t lambda, CandOf cand_of)
{
	TilePick p{false, 0u, 0u, 0u};
	uint64_t best = 0;
	for (uint32_t r = 0; r < n_factors; ++r) {
		const uint64_t cand = cand_of(r);
		if (cand == kTileFitUnusable) continue;
		const uint64_t s = tilefit_s(cand), b = tilefit_b(cand), cost = s + lambda * b;
		if (!p.any || cost < best || (cost == best && b < p.b)) {  // (equal cost and bytes: the lower r stays)
			p = TilePick{true, r, s, b};
			best = cost;
		}
	}
	return p;
}

// One halving of a group's interval [lo, hi] (lo <= hi): the lambda whose total decides it, and the interval behind it.
// PXZ_FIT_BYTES looks for the smallest lambda whose B fits, PXZ_FIT_SSE for the largest whose S does; total is B (fixed bytes
// included) or S at tilefit_mid.  An interval of one value stays as it is.
PXZ_FIT_HD inline uint64_t tilefit_mid(uint32_t criterion, uint64_t lo, uint64_t hi)
{
	return criterion == kFitBytes ? lo + (hi - lo) / 2u : lo + (hi - lo + 1u) / 2u;
}
PXZ_FIT_HD inline void tilefit_advance(uint32_t criterion, uint64_t target, uint64_t total, uint64_t *lo, uint64_t *hi)
{
	if (*lo >= *hi) return;
	const uint64_t mid = tilefit_mid(criterion, *lo, *hi);
	if (criterion == kFitBytes) {
		if (total <= target) *hi = mid;
		else *lo = mid + 1u;
	} else {
		if (total <= target) *lo = mid;
		else *hi = mid - 1u;
	}
}

struct TileFitDecision {
	uint32_t flags;     // kFitMissed | kTileFitNoCandidate | kTileFitUniform
	uint32_t uniform;   // the rung every tile takes when kTileFitUniform is set
	uint64_t bytes, sse;  // the totals of the final choice, fixed bytes included
};

// What a group ends with.  bytes_l, sse_l: the totals at lambda* (fixed bytes included); uni_bytes(r), uni_sse(r): the uniform
// totals of rung r (fixed bytes included) over its usable candidates and uni_bad(r) how many of the group's tiles have none
// at r; no_candidate: a tile of the group has no usable candidate at all.
template <class UniBytes, class UniSse, class UniBad>
PXZ_FIT_HD inline TileFitDecision tilefit_decide(uint32_t n_factors, uint32_t criterion, uint64_t target, uint64_t bytes_l, uint64_t sse_l,
                                                 bool no_candidate, UniBytes uni_bytes, UniSse uni_sse, UniBad uni_bad)
{
	TileFitDecision d{no_candidate ? kTileFitNoCandidate : 0u, 0u, bytes_l, sse_l};
	if ((criterion == kFitBytes ? bytes_l : sse_l) > target) {
		d.flags |= kFitMissed;
		return d;
	}
	// a rung that some tile cannot take goes in as (all-ones, all-ones): it is never strictly smaller than the Lagrangian pair
	const FitPick u = fit_pick(
		n_factors, criterion, target, [&](uint32_t r) -> uint64_t { return uni_bad(r) ? ~0ull : uni_bytes(r); },
		[&](uint32_t r) -> uint64_t { return uni_bad(r) ? ~0ull : uni_sse(r); });
	if (u.flags != 0u || uni_bad(u.choice)) return d;
	const uint64_t ub = uni_bytes(u.choice), us = uni_sse(u.choice);
	const uint64_t um = criterion == kFitBytes ? us : ub, uc = criterion == kFitBytes ? ub : us;
	const uint64_t lm = criterion == kFitBytes ? sse_l : bytes_l, lc = criterion == kFitBytes ? bytes_l : sse_l;
	if (um < lm || (um == lm && uc < lc)) {
		d.flags |= kTileFitUniform;
		d.uniform = u.choice;
		d.bytes = ub;
		d.sse = us;
	}
	return d;
}

// ---- one group on the host (pxz_fit_tiles_select, pxz_tilefit_check.cpp): the same steps the kernels take, in one loop
// cand(r, t): the packed candidate of rung r of the group's tile t = 0 .. n_tiles-1; choice: n_tiles entries
struct TileFitGroup {
	uint64_t lambda, bytes, sse;
	uint32_t flags;
};

template <class Cand>
inline void tilefit_totals(uint32_t n_factors, uint64_t n_tiles, uint64_t lambda, Cand cand, uint64_t *bytes, uint64_t *sse, bool *no_candidate,
                           uint32_t *choice)
{
	*bytes = *sse = 0;
	*no_candidate = false;
	for (uint64_t t = 0; t < n_tiles; ++t) {
		const TilePick p = tilefit_pick(n_factors, lambda, [&](uint32_t r) { return cand(r, t); });
		*bytes += p.b;
		*sse += p.s;
		if (!p.any) *no_candidate = true;
		if (choice) choice[t] = p.r;
	}
}

template <class Cand>
inline TileFitGroup tilefit_group(uint32_t n_factors, uint32_t criterion, uint64_t target, uint64_t fixed, uint64_t n_tiles, Cand cand,
                                  uint32_t *choice)
{
	uint64_t lo = 0, hi = kTileFitLambdaMax, b = 0, s = 0;
	bool none = false;
	for (uint32_t step = 0; step < kTileFitSteps; ++step) {
		tilefit_totals(n_factors, n_tiles, tilefit_mid(criterion, lo, hi), cand, &b, &s, &none, nullptr);
		tilefit_advance(criterion, target, criterion == kFitBytes ? fixed + b : s, &lo, &hi);
	}
	tilefit_totals(n_factors, n_tiles, lo, cand, &b, &s, &none, choice);
	auto uni = [&](uint32_t r, int what) -> uint64_t {  // 0: bytes, 1: sse, 2: tiles without the rung
		uint64_t ub = fixed, us = 0, bad = 0;
		for (uint64_t t = 0; t < n_tiles; ++t) {
			const uint64_t c = cand(r, t);
			if (c == kTileFitUnusable) ++bad;
			else ub += tilefit_b(c), us += tilefit_s(c);
		}
		return what == 0 ? ub : what == 1 ? us : bad;
	};
	const TileFitDecision d = tilefit_decide(
		n_factors, criterion, target, fixed + b, s, none, [&](uint32_t r) { return uni(r, 0); }, [&](uint32_t r) { return uni(r, 1); },
		[&](uint32_t r) { return uni(r, 2) != 0u; });
	if (d.flags & kTileFitUniform)
		for (uint64_t t = 0; t < n_tiles; ++t) choice[t] = d.uniform;
	return TileFitGroup{lo, d.bytes, d.sse, d.flags};
}

}  // namespace pxz
