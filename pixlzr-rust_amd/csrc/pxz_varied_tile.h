// pxz_varied_tile.h -- what varied_kernel (pxz_varied.hip: one factor) and varied_ladder_kernel (pxz_varied_ladder.hip:
// several factors per staged tile) share of one tile's work in a block of 256 threads: the detector's LDS constants, the
// pixel read, one resample pass along one axis and the store to a slot.  Every function is called by all 256 threads of the
// block and none ends in a barrier.  (Staging, the detectors and the un-premultiply loop stay in each unit: varied_kernel
// gains registers when they are called as functions -- DESIGN.md 8h.)
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

}  // namespace pxz
