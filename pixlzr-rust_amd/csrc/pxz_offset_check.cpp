// pxz_offset_check — the host's decision about the 32-bit lane offsets of shrink32_kernel / shrink32a_kernel
// (fast32_lane_offset_fits, pxz_internal.h), held against 64-bit arithmetic written out here: for a pitch, the largest offset a
// lane forms is 7 rows + 7 pixel quads of 16 bytes; the fast path may be taken iff that fits 32 bits.  Checked at the boundary
// (the last pitch that fits, the first that does not, and their 16-byte-aligned neighbours), at the ends of the range and over a
// sweep.  Prints "ok <last fitting pitch> <cases>" (tests/test_gpu_shrink32_staging.py runs it).
#include <cstdio>

#include "pxz_internal.h"

int main()
{
	// the largest pitch with 7 * pitch + 112 <= 2^32 - 1
	const uint64_t last = (0xffffffffull - 112ull) / 7ull;
	long cases = 0;
	auto check = [&](uint64_t pitch) -> bool {
		if (pitch > 0xffffffffull) return true;
		uint64_t worst = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) {
			const uint64_t off = (uint64_t)(lane >> 3) * pitch + (uint64_t)(lane & 7u) * 16ull;
			if (off > worst) worst = off;
		}
		const bool want = worst <= 0xffffffffull;
		++cases;
		if (pxz::fast32_lane_offset_fits((uint32_t)pitch) != want) {
			printf("FAIL pitch %llu: largest lane offset %llu, the host says %d\n", (unsigned long long)pitch, (unsigned long long)worst,
			       (int)pxz::fast32_lane_offset_fits((uint32_t)pitch));
			return false;
		}
		// and what the kernel computes in 32 bits is the true offset whenever the host lets the batch through
		if (want) {
			const uint32_t p32 = (uint32_t)pitch;
			for (uint32_t lane = 0; lane < 64; ++lane) {
				const uint32_t off32 = (lane >> 3) * p32 + (lane & 7u) * 16u;
				if ((uint64_t)off32 != (uint64_t)(lane >> 3) * pitch + (uint64_t)(lane & 7u) * 16ull) {
					printf("FAIL pitch %llu lane %u: the 32-bit offset wraps\n", (unsigned long long)pitch, lane);
					return false;
				}
			}
		}
		return true;
	};
	const uint64_t directed[] = {0, 16, 128, 30720, 32768, 1ull << 20, 1ull << 29, last - 16, last - 1, last, last + 1, last + 2, last + 16,
	                             (last & ~15ull), (last & ~15ull) + 16, 1ull << 30, 1ull << 31, 0xfffffff0ull, 0xffffffffull};
	for (uint64_t p : directed)
		if (!check(p)) return 1;
	if (!pxz::fast32_lane_offset_fits((uint32_t)last) || pxz::fast32_lane_offset_fits((uint32_t)(last + 1))) {
		printf("FAIL the boundary is not at %llu\n", (unsigned long long)last);
		return 1;
	}
	for (uint64_t p = 0; p <= 0xffffffffull; p += 1000003ull)
		if (!check(p)) return 1;
	printf("ok %llu %ld\n", (unsigned long long)last, cases);
	return 0;
}
