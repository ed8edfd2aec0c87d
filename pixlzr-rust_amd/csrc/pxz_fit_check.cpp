// pxz_fit_check — gather_copy (pxz_fit.h), the tile copy of gather_rungs_kernel, run on the host: the 64 lanes one after the
// other, for every pair of source and destination alignments mod 16 and lengths from 0 to beyond several 16-byte lines, the odd
// slot sizes of the tests among them (45, 6771).  Checked: exactly the bytes [0, bytes) of the destination are written, with the
// source's bytes -- the destination is poisoned with a byte the source does not hold at that place, before, inside and behind.
// And gather_split, which says how the copy is cut, is held against its promise: dwords start at a multiple of 4 of both
// addresses, 16-byte lines at a multiple of 16 of both, the counts add up, and the wide forms are taken whenever the two
// addresses allow them.  Prints "ok <cases>" (tests/test_fit_host.py runs it).
#include <cstdio>
#include <cstring>

#include "pxz_fit.h"

int main()
{
	constexpr uint32_t kMax = 8192, kLead = 32;
	alignas(16) static uint8_t src[kMax + 64], dst[kMax + 128];
	const uint32_t lengths[] = {0, 1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 19, 20, 31, 32, 33, 45, 47, 48, 63, 64, 65, 100, 255, 256, 257,
	                            1023, 1024, 1029, 4096, 6771, 8191, 8192};
	long cases = 0;
	for (uint32_t so = 0; so < 16; ++so)
		for (uint32_t dofs = 0; dofs < 16; ++dofs)
			for (uint32_t bytes : lengths) {
				for (uint32_t i = 0; i < sizeof src; ++i) src[i] = (uint8_t)(i * 7u + so);
				// the destination's poison differs from what the source holds at the same place, also behind the valid bytes
				for (uint32_t i = 0; i < sizeof dst; ++i) dst[i] = (uint8_t)~src[(i + so + sizeof src - kLead - dofs) % sizeof src];
				alignas(16) static uint8_t before[sizeof dst];
				memcpy(before, dst, sizeof dst);
				const uintptr_t da = reinterpret_cast<uintptr_t>(dst + kLead + dofs), sa = reinterpret_cast<uintptr_t>(src + so);
				const pxz::GatherSplit g = pxz::gather_split(da, sa, bytes);
				const uint32_t rest = bytes - (g.at + 4u * (g.n4a + 4u * g.n16 + g.n4b));
				bool good = g.wide == ((da & 3u) == (sa & 3u)) && g.at + 4u * (g.n4a + 4u * g.n16 + g.n4b) <= bytes;
				if (g.wide) {
					const uintptr_t d4 = da + g.at, s4 = sa + g.at, d16 = d4 + 4u * g.n4a, s16 = s4 + 4u * g.n4a;
					good = good && g.at < 4u && rest < 4u && g.n4b < 4u;
					good = good && (g.n4a + g.n4b == 0u || ((d4 & 3u) == 0u && (s4 & 3u) == 0u));
					good = good && (g.n16 == 0u || ((d16 & 15u) == 0u && (s16 & 15u) == 0u));
					// lines whenever both addresses share their place in one and a whole line lies inside
					const bool same16 = (da & 15u) == (sa & 15u);
					const uintptr_t line = (da + 15u) & ~(uintptr_t)15u;
					good = good && (g.n16 != 0u) == (same16 && line + 16u <= da + bytes);
					good = good && (same16 || g.n4b == 0u) && (g.n16 != 0u || same16 == false || g.n4a <= 6u);
				} else {
					good = good && g.at + g.n4a + g.n16 + g.n4b == 0u;
				}
				if (!good) {
					printf("FAIL source %u destination %u bytes %u: the split %u %u %u %u\n", so, dofs, bytes, g.at, g.n4a, g.n16, g.n4b);
					return 1;
				}
				for (uint32_t lane = 64; lane-- > 0;) pxz::gather_copy(dst + kLead + dofs, src + so, bytes, lane);
				for (uint32_t i = 0; i < sizeof dst; ++i) {
					const bool in = i >= kLead + dofs && i < kLead + dofs + bytes;
					const uint8_t want = in ? src[so + (i - kLead - dofs)] : before[i];
					if (dst[i] != want) {
						printf("FAIL source %u destination %u bytes %u: byte %d of the destination\n", so, dofs, bytes, (int)i - (int)(kLead + dofs));
						return 1;
					}
				}
				++cases;
			}
	printf("ok %ld\n", cases);
	return 0;
}
