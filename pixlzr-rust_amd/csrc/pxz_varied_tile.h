// pxz_varied_tile.h -- what varied_kernel (pxz_varied.hip: one factor) and varied_ladder_kernel (pxz_varied_ladder.hip:
// several factors per staged tile) share of one tile's work in a block of 256 threads: the detector's LDS constants, the
// pixel read, one resample pass along one axis and the store to a slot.  Every function is called by all 256 threads of the
// block; the pass and the store do not end in a barrier.  (Staging, the detectors and the un-premultiply loop stay in the units
// of varied_kernel and reshrink_kernel: varied_kernel gains registers when they are called as functions -- DESIGN.md 8h.  The
// ladder kernels' forms of the detectors and of that loop are at the end of this header; the one-factor kernels never call
// them, and their instruction streams are the same with and without -- DESIGN.md 8j.)
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


// ---- what the two ladder kernels (pxz_varied_ladder.hip, pxz_reshrink_ladder.hip) share beyond that: a tile measured once,
// up to what the factor has not entered, and the un-premultiply of a resampled image

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

}  // namespace pxz
