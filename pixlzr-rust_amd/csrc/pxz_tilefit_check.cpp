// pxz_tilefit_check — the per-tile rule of pxz_tilefit.h run on the host, one group at a time, against an exhaustive search
// over all n_factors^tiles assignments of small random tables (up to 5 tiles, up to 4 rungs; small values, so ties are
// everywhere; a tenth of the candidates unusable).  Checked for both criteria and a sweep of targets:
//   the totals are those of the returned choices, and a tile without a usable candidate is flagged and has choice 0;
//   missed <=> no assignment of usable candidates meets the target;
//   the pick at lambda* kept: no assignment whose constrained total is at most the chosen one has a smaller minimised total;
//   one rung for all taken: it is what fit_pick gives on the uniform totals, and strictly better than the pick at lambda*;
//   either way the result is never worse than fit_pick on the uniform totals;
//   B(lambda) never increases and S(lambda) never decreases over a sweep of lambda, and lambda* is where the header says.
// Being stand-alone it can be built with -fsanitize=address,undefined and run as it is.  Prints "ok <cases>"
// (tests/test_tilefit_host.py runs it).
#include <cstdio>
#include <vector>

#include "pxz_tilefit.h"

using namespace pxz;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)((rng_state >> 11) % n);
}

#define CHECK(cond, what)                                                                                     \
	do {                                                                                                      \
		if (!(cond)) {                                                                                        \
			printf("FAIL table %d criterion %u target %llu: %s\n", table, criterion, (unsigned long long)target, what); \
			return 1;                                                                                         \
		}                                                                                                     \
	} while (0)

int main()
{
	long cases = 0;
	for (int table = 0; table < 400; ++table) {
		const uint32_t K = 1u + rnd(4), T = 1u + rnd(5);
		const uint64_t fixed = rnd(3) * 7u;
		std::vector<uint64_t> cand((size_t)K * T);
		for (auto &c : cand) {
			const uint64_t sse[3] = {rnd(4), rnd(3), rnd(2)};
			c = rnd(10) == 0 ? kTileFitUnusable : tilefit_pack(rnd(6), sse, 3);
		}
		auto at = [&](uint32_t r, uint64_t t) { return cand[(size_t)r * T + t]; };
		std::vector<bool> has(T, false);
		bool all_have = true;
		for (uint32_t t = 0; t < T; ++t) {
			for (uint32_t r = 0; r < K; ++r) has[t] = has[t] || at(r, t) != kTileFitUnusable;
			all_have = all_have && has[t];
		}
		// every assignment of usable candidates (tiles without one stay out): its totals
		std::vector<std::pair<uint64_t, uint64_t>> all;  // (bytes with the fixed ones, sse)
		std::vector<uint32_t> pick(T, 0);
		for (;;) {
			uint64_t b = fixed, s = 0;
			bool usable = true;
			for (uint32_t t = 0; t < T && usable; ++t) {
				if (!has[t]) continue;
				if (at(pick[t], t) == kTileFitUnusable) usable = false;
				else b += tilefit_b(at(pick[t], t)), s += tilefit_s(at(pick[t], t));
			}
			if (usable) all.emplace_back(b, s);
			uint32_t t = 0;
			while (t < T && ++pick[t] == K) pick[t++] = 0;
			if (t == T) break;
		}
		// monotone totals over a sweep of lambda
		{
			const uint32_t criterion = 0;
			const uint64_t target = 0;
			uint64_t pb = ~0ull, ps = 0;
			const uint64_t sweep[] = {0, 1, 2, 3, 5, 8, 100, 1ull << 16, (1ull << 32) - 1, 1ull << 32};
			for (uint64_t lambda : sweep) {
				uint64_t b, s;
				bool none;
				tilefit_totals(K, T, lambda, at, &b, &s, &none, nullptr);
				CHECK(b <= pb && s >= ps, "B or S is not monotone in lambda");
				CHECK(none == !all_have, "no_candidate");
				pb = b;
				ps = s;
			}
		}
		for (uint32_t criterion = 0; criterion < 2; ++criterion)
			for (uint64_t target : {0ull, 1ull, 3ull, 5ull, 8ull, 11ull, 14ull, 18ull, 25ull, 40ull, ~0ull}) {
				std::vector<uint32_t> choice(T, 99u);
				const TileFitGroup g = tilefit_group(K, criterion, target, fixed, T, at, choice.data());
				uint64_t b = fixed, s = 0;
				for (uint32_t t = 0; t < T; ++t) {
					if (!has[t]) {
						CHECK(choice[t] == 0u, "a tile without a usable candidate has another choice than 0");
						continue;
					}
					CHECK(choice[t] < K && at(choice[t], t) != kTileFitUnusable, "an unusable candidate was chosen");
					b += tilefit_b(at(choice[t], t));
					s += tilefit_s(at(choice[t], t));
				}
				CHECK(b == g.bytes && s == g.sse, "the totals are not those of the choices");
				CHECK(((g.flags & kTileFitNoCandidate) != 0u) == !all_have, "bit 1");
				CHECK(g.lambda <= kTileFitLambdaMax, "lambda beyond its range");
				auto con = [&](const std::pair<uint64_t, uint64_t> &a) { return criterion == kFitBytes ? a.first : a.second; };
				auto mini = [&](const std::pair<uint64_t, uint64_t> &a) { return criterion == kFitBytes ? a.second : a.first; };
				bool fits = false;
				for (const auto &a : all) fits = fits || con(a) <= target;
				CHECK(((g.flags & kFitMissed) != 0u) == !fits, "missed <=> no assignment fits");
				const std::pair<uint64_t, uint64_t> mine(g.bytes, g.sse);
				if (g.flags & kFitMissed) {
					CHECK(g.lambda == (criterion == kFitBytes ? kTileFitLambdaMax : 0u) && !(g.flags & kTileFitUniform), "a missed group's lambda");
					++cases;
					continue;
				}
				CHECK(con(mine) <= target, "the target is not met");
				// lambda* is the first (last) lambda whose total fits
				{
					uint64_t lb, ls;
					bool none;
					if (criterion == kFitBytes && g.lambda > 0u) {
						tilefit_totals(K, T, g.lambda - 1u, at, &lb, &ls, &none, nullptr);
						CHECK(fixed + lb > target, "a smaller lambda fits too");
					}
					if (criterion == kFitSse && g.lambda < kTileFitLambdaMax) {
						tilefit_totals(K, T, g.lambda + 1u, at, &lb, &ls, &none, nullptr);
						CHECK(ls > target, "a larger lambda fits too");
					}
				}
				if (!(g.flags & kTileFitUniform))
					for (const auto &a : all) CHECK(!(con(a) <= con(mine) && mini(a) < mini(mine)), "an assignment within the chosen total is better");
				// against fit_pick on the uniform totals
				std::vector<std::pair<uint64_t, uint64_t>> uni;
				for (uint32_t r = 0; r < K; ++r) {
					std::pair<uint64_t, uint64_t> u(fixed, 0);
					bool whole = true;
					for (uint32_t t = 0; t < T; ++t) {
						if (at(r, t) == kTileFitUnusable) whole = false;
						else u.first += tilefit_b(at(r, t)), u.second += tilefit_s(at(r, t));
					}
					if (whole) uni.push_back(u);
				}
				if (!uni.empty()) {
					const FitPick p = fit_pick((uint32_t)uni.size(), criterion, target, [&](uint32_t r) { return uni[r].first; },
					                           [&](uint32_t r) { return uni[r].second; });
					if (p.flags == 0u) {
						const auto &u = uni[p.choice];
						CHECK(mini(mine) < mini(u) || (mini(mine) == mini(u) && con(mine) <= con(u)), "worse than one factor for the group");
						if (g.flags & kTileFitUniform) CHECK(mine == u, "one rung for all, but not fit_pick's");
					} else {
						CHECK(!(g.flags & kTileFitUniform), "one rung for all though none is eligible");
					}
				} else {
					CHECK(!(g.flags & kTileFitUniform), "one rung for all though no rung is usable for every tile");
				}
				++cases;
			}
	}
	printf("ok %ld\n", cases);
	return 0;
}
