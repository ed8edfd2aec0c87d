// pxz_device.h -- device-side helpers shared by the kernel files (gfx950 only): constant tables, index math,
// packed 16-bit / dot2 / matrix-core resample helpers of the fast paths, the worklist batching, finish_tile, and what the
// kernels of a flat tile space share: the owner search, the resize of a stored tile, the tile store.
// Included by every pxz_*.hip; everything here is __device__ __forceinline__ or a file-local table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "pxz_internal.h"

namespace pxz {

// ---------------------------------------------------------------------------
// constant tables
// ---------------------------------------------------------------------------

// sRGB u8 -> linear f32 (bits): the 256-entry table palette 0.7.6 / fast-srgb8
// 1.0.0 use for `Srgb<u8>::into_linear()` (reference operations.rs:56-59).
static __constant__ uint32_t kSrgbToLinearBits[256] = {
#include "srgb_lut.inc"
};

// fast_image_resize un-premultiply: recip[a] = ((255 << 9) / a + 1) >> 1
struct RecipAlphaTable {
	uint32_t v[256];
	constexpr RecipAlphaTable() : v{}
	{
		for (uint32_t a = 1; a < 256; ++a) v[a] = ((255u * 512u) / a + 1u) >> 1;
	}
};
static __constant__ RecipAlphaTable kRecipAlpha = RecipAlphaTable();

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------

// Walks i = first, first+step, ... while tracking (row, col) = (i / width, i % width)
// without a division per element.
// n / d for a host-prepared divisor (round-up magic number): stays on the scalar unit for
// wave-uniform n, where a plain `/` would expand to ~25 VALU instructions.
__device__ __forceinline__ uint32_t fastdiv(uint32_t n, const FastDiv &d)
{
	const uint32_t t = __umulhi(n, d.mul);
	return (t + ((n - t) >> d.sh1)) >> d.sh2;
}

// n / d for n < 2^20, d >= 1 in five instructions instead of the ~30 of a general 32-bit division:
// x = (n + 0.5) / d is at least 0.5/d away from every integer, and the float product with the 1-ulp
// reciprocal is within x * 2^-22 of it, which is below 0.5/d for every n < 2^21.
__device__ __forceinline__ uint32_t small_div(uint32_t n, uint32_t d)
{
	return (uint32_t)(((float)n + 0.5f) * __builtin_amdgcn_rcpf((float)d));
}

struct RowWalker {
	uint32_t row, col, drow, dcol, width;
	__device__ RowWalker(uint32_t first, uint32_t step, uint32_t width_) : width(width_)
	{
		// first and step are lane / thread counts (<= 1024 + a tile's pixel count < 2^20)
		row = small_div(first, width_);
		col = first - row * width_;
		drow = small_div(step, width_);
		dcol = step - drow * width_;
	}
	__device__ void next()
	{
		row += drow;
		col += dcol;
		if (col >= width) {
			col -= width;
			++row;
		}
	}
};

template <int NW>
__device__ __forceinline__ void tile_sync()
{
	if constexpr (NW == 1) {
		// one wave owns the tile: LDS operations of a wave execute in order,
		// only the compiler must not move them across this point
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	} else {
		__syncthreads();
	}
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}
__device__ __forceinline__ uint32_t wave_and_u32(uint32_t v)
{
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) v &= __shfl_xor(v, off, 64);
	return v;
}

// A 64-bit value (an address) made wave-uniform, i.e. a scalar: lane 0's two halves.  The builtin returns a signed int:
// without the casts a low half of 2^31 and more is sign-extended over the high one.
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
	return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
	       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}

__device__ __forceinline__ uint32_t fbits(float f) { return __float_as_uint(f); }

// reference operations.rs:128-138
__device__ __forceinline__ float parse_value(float value)
{
	if ((fbits(value) >> 31) == 0) return value;
	float t = 1.0f + value;
	// f32::max(t, 0.0): NaN -> 0.0
	float v = (t != t) ? 0.0f : (t > 0.0f ? t : 0.0f);
	return v;  // never negative-signed here, so the `else 1f32` arm is unreachable
}

// n = min(round(log2f(v)), 0) as the exponent m = -n in [0, 32]; thresholds[k] is
// the smallest float with round(log2f(v)) >= -k (host-built with the platform log2f).
__device__ __forceinline__ uint32_t level_exponent(float v, const float *thresholds)
{
	uint32_t m = 0;
#pragma unroll
	for (int k = 0; k < kNumThresholds; ++k) m += (v < thresholds[k]) ? 1u : 0u;
	return m;
}

// ceil(max(size * 2^-m, 1)) (operations.rs:150-151)
__device__ __forceinline__ uint32_t reduced_size(uint32_t size, uint32_t m)
{
	if (m >= 31) return 1;
	uint32_t r = (uint32_t)(((uint64_t)size + ((1ull << m) - 1ull)) >> m);
	return r < 1 ? 1 : r;
}

// f32::hypot as glibc computes it (double sqrt of the exact squares' sum)
__device__ __forceinline__ float hypot_f32(float x, float y)
{
	double dx = (double)x, dy = (double)y;
	return (float)__dsqrt_rn(dx * dx + dy * dy);
}

// f32::cbrt = glibc 2.35 cbrtf: frexp, quadratic seed and one Halley step in double.
__device__ __forceinline__ float cbrt_f32(float x)
{
	if (x == 0.0f) return x + x;
	int xe;
	float xm = frexpf(fabsf(x), &xe);
	float u = (float)(0.492659620528969547 +
	                  (0.697570460207922770 - 0.191502161678719066 * (double)xm) * (double)xm);
	float t2 = u * u * u;
	int r = xe % 3;  // C semantics, sign follows xe
	double scale = r == 0 ? 1.0
	             : r == 1 ? 1.2599210498948731648
	             : r == 2 ? 1.5874010519681994748
	             : r == -1 ? 1.0 / 1.2599210498948731648
	                       : 1.0 / 1.5874010519681994748;
	float ym = (float)((double)u * ((double)t2 + 2.0 * (double)xm) / (2.0 * (double)t2 + (double)xm) * scale);
	return ldexpf(x > 0.0f ? ym : -ym, xe / 3);
}

// palette 0.7.6 LinSrgb<f32> -> Oklab<f32> (Ottosson's matrices, left-to-right f32 sums)
__device__ __forceinline__ void oklab_from_rgba(uint32_t px, float &L, float &A, float &B)
{
	float r = __uint_as_float(kSrgbToLinearBits[px & 255u]);
	float g = __uint_as_float(kSrgbToLinearBits[(px >> 8) & 255u]);
	float b = __uint_as_float(kSrgbToLinearBits[(px >> 16) & 255u]);
	float l = 0.4122214708f * r + 0.5363325363f * g + 0.0514459929f * b;
	float m = 0.2119034982f * r + 0.6806995451f * g + 0.1073969566f * b;
	float s = 0.0883024619f * r + 0.2817188376f * g + 0.6299787005f * b;
	float l_ = cbrt_f32(l), m_ = cbrt_f32(m), s_ = cbrt_f32(s);
	L = 0.2104542553f * l_ + 0.7936177850f * m_ - 0.0040720468f * s_;
	A = 1.9779984951f * l_ - 2.4285922050f * m_ + 0.4505937099f * s_;
	B = 0.0259040371f * l_ + 0.7827717662f * m_ - 0.8086757660f * s_;
}

// fast_image_resize alpha premultiply: mul_div_255
__device__ __forceinline__ uint32_t mul_div_255(uint32_t a, uint32_t b)
{
	uint32_t t = a * b + 128u;
	return ((t >> 8) + t) >> 8;
}
__device__ __forceinline__ uint32_t premultiply(uint32_t px)
{
	uint32_t al = px >> 24;
	return mul_div_255(px & 255u, al) | (mul_div_255((px >> 8) & 255u, al) << 8) |
	       (mul_div_255((px >> 16) & 255u, al) << 16) | (al << 24);
}
__device__ __forceinline__ uint32_t unpremultiply(uint32_t px)
{
	uint32_t al = px >> 24;
	// the identity at alpha 255 (recip = 256): no table look-up when every lane that is here holds an opaque pixel
	if (__builtin_amdgcn_ballot_w64(al != 255u) == 0ull) return px;
	uint32_t rc = kRecipAlpha.v[al];
	uint32_t r = ((px & 255u) * rc + 128u) >> 8;
	uint32_t g = (((px >> 8) & 255u) * rc + 128u) >> 8;
	uint32_t b = (((px >> 16) & 255u) * rc + 128u) >> 8;
	r = r > 255u ? 255u : r;
	g = g > 255u ? 255u : g;
	b = b > 255u ? 255u : b;
	return r | (g << 8) | (b << 16) | (al << 24);
}

__device__ __forceinline__ uint32_t clip8(int32_t acc, int precision)
{
	int32_t v = acc >> precision;
	return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <int C>
__device__ __forceinline__ void store_pixel(uint8_t *dst, uint32_t index, uint32_t px)
{
	if constexpr (C == 4) {
		reinterpret_cast<uint32_t *>(dst)[index] = px;
	} else {
		uint8_t *p = dst + (size_t)index * 3;
		p[0] = (uint8_t)px;
		p[1] = (uint8_t)(px >> 8);
		p[2] = (uint8_t)(px >> 16);
	}
}

// ---------------------------------------------------------------------------
// packed-math helpers
// ---------------------------------------------------------------------------
typedef short short2v __attribute__((ext_vector_type(2)));
typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ ushort2v us2(uint32_t v) { return __builtin_bit_cast(ushort2v, v); }
__device__ __forceinline__ uint32_t u32(ushort2v v) { return __builtin_bit_cast(uint32_t, v); }

// acc + a.lo*b.lo + a.hi*b.hi on i16 halves (v_dot2_i32_i16)
__device__ __forceinline__ int32_t dot2(uint32_t a, uint32_t b, int32_t acc)
{
	return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), acc, false);
}
// acc + |a.lo-b.lo| + |a.hi-b.hi| on u16 halves (v_sad_u16)
__device__ __forceinline__ uint32_t sad16(uint32_t a, uint32_t b, uint32_t acc)
{
	return __builtin_amdgcn_sad_u16(a, b, acc);
}
// a + b on both u16 halves where the low halves cannot carry (sums of a few 8-bit samples): ONE plain 32-bit add.  Written
// as a packed add (v_pk_add_u16) it is a VOP3P instruction, and those -- like every three-source integer form, SDWA and DPP
// -- occupy the SIMD for 4.3 cycles against the 2 of a VOP2 add (profiles/r03_issue_probe.txt).
__device__ __forceinline__ uint32_t add2x16(uint32_t a, uint32_t b) { return a + b; }
// horizontal 1-2-1 smoothing of the pixel pairs D0=(x,x+1), D1=(x+2,x+3): (x+2(x+1)+(x+2), (x+1)+2(x+2)+(x+3))
__device__ __forceinline__ uint32_t smooth121(uint32_t d0, uint32_t d1)
{
	const uint32_t mid = __builtin_amdgcn_alignbit(d1, d0, 16);  // (x+1, x+2)
	return u32(us2(mid) * (ushort2v)(2) + (us2(d0) + us2(d1)));
}

// v_pk_mad_u16: a*b+c on both u16 halves (the compiler prefers shift+add, one VALU op more)
__device__ __forceinline__ uint32_t pk_mad_u16(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t d;
	asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
	return d;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// sum over the wave, result in an SGPR: butterfly inside each row of 16 lanes (DPP), then 4 readlanes
__device__ __forceinline__ uint32_t wave_sum_sgpr(uint32_t v)
{
	v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
	v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
	v += dpp_mov<0x124>(v);  // row_ror:4
	v += dpp_mov<0x128>(v);  // row_ror:8
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
	       (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
// the same with the four row sums joined on the vector unit: row_bcast15 hands lane 15 of a row to the next row (rows 1 and 3
// take it), row_bcast31 lane 31 to rows 2 and 3; lane 63 then holds the sum -- 2 DPP adds and 1 readlane for 4 readlanes and 3
// scalar adds
__device__ __forceinline__ uint32_t wave_sum_sgpr_bcast(uint32_t v)
{
	v += dpp_mov<0xB1>(v);
	v += dpp_mov<0x4E>(v);
	v += dpp_mov<0x124>(v);
	v += dpp_mov<0x128>(v);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_and_sgpr(uint32_t v)
{
	v &= dpp_mov<0xB1>(v);
	v &= dpp_mov<0x4E>(v);
	v &= dpp_mov<0x124>(v);
	v &= dpp_mov<0x128>(v);
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) & (uint32_t)__builtin_amdgcn_readlane((int)v, 16) &
	       (uint32_t)__builtin_amdgcn_readlane((int)v, 32) & (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

__device__ __forceinline__ uint32_t level_count(uint32_t key, const uint32_t *breaks, uint32_t asc)
{
	key = __builtin_amdgcn_readfirstlane(key);  // tile-uniform: keep the compares on the scalar unit
	uint32_t m = 0;
#pragma unroll
	for (int j = 0; j < kMaxLevel; ++j) m += ((key < breaks[j]) != (asc != 0)) ? 1u : 0u;
	return m;
}

// LDS accesses spelled one by one (base + 16-bit immediate): left to itself the compiler pairs neighbouring accesses
// into ds_read2 / ds_write2, whose 8-bit offsets cost a vector add per new base -- 16 of them per tile in the pair form of
// shrink32_kernel's detector (sobel32_quads below reads aligned 8-byte quads with lds_load2).
typedef const volatile __attribute__((address_space(3))) uint32_t *lds_cptr;
__device__ __forceinline__ uint32_t lds_dword(const uint32_t *p) { return *(lds_cptr)p; }
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 lds_load2(const uint32_t *p)
{
	const u32x2 v = *(const volatile __attribute__((address_space(3))) u32x2 *)p;
	return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void lds_store2(uint32_t *p, uint2 v)
{
	u32x2 w = {v.x, v.y};
	*(volatile __attribute__((address_space(3))) u32x2 *)p = w;
}

// ---------------------------------------------------------------------------
// resample fast path: full, opaque 32x32 RGBA tile, both passes needed.
// Compile-time geometry (plane row stride 18 dwords -- 16 + 2 of bank skew --, plane 576
// dwords, transposed plane [ox][18 dwords] = 288 dwords) turns every LDS address into
// base+immediate and keeps the row groups / output columns on distinct banks.
// Work items are spread over all 64 lanes: when there are fewer than 64 outputs the
// filter window itself is split over 2..8 lanes and summed with DPP.
// ---------------------------------------------------------------------------
constexpr uint32_t kRS32 = 18, kPD32 = 18 * 32, kHS32 = 18;
// transposed planes of the dot2 two-pass form: up to 8 output columns (16/8/4-px outputs on both axes go
// through the matrix cores; the rare 16 x (2|1) tile is handed to the worklist)
constexpr uint32_t kTD32 = 8 * 18;
constexpr uint32_t kOut32 = 512;  // dwords of the region after the planes: transposed planes / parked output pixels

// ---------------------------------------------------------------------------
// The directional detector of a staged 32x32 tile (three planes of u16 pairs, rows of kRS32 dwords) on pixel QUADS: per lane
// the integer sums of |hz| and |vr| over the 3x3 windows it owns; the caller sums them over the wave.
// Lane map: j = tid & 7 is the quad (columns 4j..4j+3 = dwords 2j, 2j+1 of a row: ONE aligned ds_read_b64 per row and
// channel -- 18 per tile where the pair form issues 60 ds_read_b32 and fetches every dword twice), G = tid >> 3 one of eight
// row groups with base row R = 8 (G & 3) + 4 (G >> 2).  The four groups of a 32-lane half lie 8 rows = 144 dwords = 16
// (mod 64) apart: disjoint 16-bank ranges, no conflicts.  A group reads rows R..R+5 and owns window rows R..R+3 (two steps
// of two rows; R = 28 owns 28 and 29 and runs one step -- rows 32, 33 are neither read nor counted).
// Pair A = windows x = 4j, 4j+1, pair B = x = 4j+2, 4j+3.  Pair B needs the next quad's first pixel pair (1-2-1 along x) and
// its pair-A column sum (|vr|): DPP row_shl:1.  Quad 7 has no pair-B window (x = 30, 31) and its DPP source is another
// group's lane or zero: pair B keeps accumulators of its own, cleared for j == 7 before they are added.
// The sums are integers: whatever the order, bit for bit those of the pair form.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sobel32_quads(const uint32_t *s_pl, uint32_t tid, uint32_t &sum_hz, uint32_t &sum_vr)
{
	const uint32_t j = tid & 7u, G = tid >> 3;
	const uint32_t *pq = s_pl + (8u * (G & 3u) + 4u * (G >> 2)) * kRS32 + 2u * j;
	const uint32_t two = 0x00020002u;
	// (compared afresh where it is used: hoisted out of the tile loop the lane mask would sit in two scalar registers, and
	// those are spilled -- two v_readlane per use instead of one v_cmp)
	auto second_step = [](uint32_t grp) -> bool {
		asm volatile("" : "+v"(grp));
		return grp != 7u;
	};
	// 1-2-1 along x of a row's quad: .x = pair A (p0 + 2 p1 + p2, p1 + 2 p2 + p3), .y = pair B (p2 + 2 p3 + p4, p3 + 2 p4 + p5)
	auto smooth_row = [&](uint2 d) -> uint2 {
		const uint32_t nx = dpp_mov<0x101>(d.x);  // row_shl:1 = (p4, p5), the quad to the right
		return make_uint2(pk_mad_u16(__builtin_amdgcn_alignbit(d.y, d.x, 16), two, add2x16(d.x, d.y)),
		                  pk_mad_u16(__builtin_amdgcn_alignbit(nx, d.y, 16), two, add2x16(d.y, nx)));
	};
	uint32_t hzA = 0, vrA = 0, hzB = 0, vrB = 0;
	uint2 rA[3], rB[3], tP[3], dP[3];
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const uint2 a = lds_load2(pq + c * kPD32), b = lds_load2(pq + c * kPD32 + kRS32);
		rA[c] = smooth_row(a);
		rB[c] = smooth_row(b);
		tP[c] = make_uint2(add2x16(a.x, b.x), add2x16(a.y, b.y));
		dP[c] = b;
	}
#pragma unroll
	for (int st = 0; st < 2; ++st) {
		if (st < 1 || second_step(G)) {
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				const uint32_t *pr = pq + c * kPD32 + (2 + 2 * st) * (int)kRS32;
				const uint2 n = lds_load2(pr), o = lds_load2(pr + kRS32);
				const uint2 rN = smooth_row(n);
				hzA = sad16(rN.x, rA[c].x, hzA);
				hzB = sad16(rN.y, rA[c].y, hzB);
				const uint2 tN = make_uint2(add2x16(dP[c].x, n.x), add2x16(dP[c].y, n.y));
				const uint2 c0 = make_uint2(add2x16(tP[c].x, tN.x), add2x16(tP[c].y, tN.y));
				vrA = sad16(c0.y, c0.x, vrA);                   // the neighbour columns are pair B's, in this lane
				vrB = sad16(dpp_mov<0x101>(c0.x), c0.y, vrB);  // pair A's of the quad to the right
				const uint2 rO = smooth_row(o);
				hzA = sad16(rO.x, rB[c].x, hzA);
				hzB = sad16(rO.y, rB[c].y, hzB);
				const uint2 tO = make_uint2(add2x16(n.x, o.x), add2x16(n.y, o.y));
				const uint2 e0 = make_uint2(add2x16(tN.x, tO.x), add2x16(tN.y, tO.y));
				vrA = sad16(e0.y, e0.x, vrA);
				vrB = sad16(dpp_mov<0x101>(e0.x), e0.y, vrB);
				rA[c] = rN;
				rB[c] = rO;
				tP[c] = tO;
				dP[c] = o;
			}
		}
	}
	{
		uint32_t jj = j;
		asm volatile("" : "+v"(jj));  // (a fresh compare, not a hoisted and spilled lane mask)
		if (jj == 7u) hzB = vrB = 0;  // quad 7 starts no pair-B window (x = 30, 31)
	}
	sum_hz = hzA + hzB;
	sum_vr = vrA + vrB;
}

template <int LPI>
__device__ __forceinline__ int32_t group_sum(int32_t v)
{
	if constexpr (LPI == 8) v += (int32_t)dpp_mov<0x141>((uint32_t)v);  // row_half_mirror: i <-> 7-i
	if constexpr (LPI >= 4) v += (int32_t)dpp_mov<0x4E>((uint32_t)v);   // quad_perm [2,3,0,1]
	if constexpr (LPI >= 2) v += (int32_t)dpp_mov<0xB1>((uint32_t)v);   // quad_perm [1,0,3,2]
	return v;
}

// A lane's table row: header {first quad, quads, weight sum} + up to 8 quads of packed weights,
// fetched as independent 16-byte loads (one memory latency instead of one per window step).
struct RowRegs {
	uint32_t fq, nq;
	int32_t ksum;
	uint32_t k[16];
};
__device__ __forceinline__ void load_row(const uint32_t *rowp, RowRegs &r)
{
	const uint4 h = *reinterpret_cast<const uint4 *>(rowp);
	const uint4 c0 = *reinterpret_cast<const uint4 *>(rowp + 4), c1 = *reinterpret_cast<const uint4 *>(rowp + 8);
	const uint4 c2 = *reinterpret_cast<const uint4 *>(rowp + 12), c3 = *reinterpret_cast<const uint4 *>(rowp + 16);
	r.fq = h.x;
	r.nq = h.y;
	r.ksum = (int32_t)h.z;
	r.k[0] = c0.x; r.k[1] = c0.y; r.k[2] = c0.z; r.k[3] = c0.w;
	r.k[4] = c1.x; r.k[5] = c1.y; r.k[6] = c1.z; r.k[7] = c1.w;
	r.k[8] = c2.x; r.k[9] = c2.y; r.k[10] = c2.z; r.k[11] = c2.w;
	r.k[12] = c3.x; r.k[13] = c3.y; r.k[14] = c3.z; r.k[15] = c3.w;
}

// horizontal pass, one source row per item: item = (ox, y), the window split over LPI lanes
// (each lane takes quads part, part+LPI, ...; weights beyond the window are zero in the table)
template <int LPI>
__device__ __forceinline__ void fast32_h_rows(const uint32_t *trows, const AxisTab &tx, const uint32_t *s_pl, uint32_t *s_tmp,
                                              uint32_t lane, uint32_t nw, uint32_t lgx, uint32_t in_rows = 32u)
{
	constexpr int QPL = 8 / LPI;  // quads per lane
	const uint32_t item = lane / LPI, part = lane % LPI;
	const bool live = item < nw * in_rows;
	const uint32_t ox = item & (nw - 1u), y = live ? item >> lgx : 0u;
	const uint32_t *rowp = trows + tx.rows_off + ox * tx.row_stride;
	const uint4 hdr = *reinterpret_cast<const uint4 *>(rowp);
	uint2 kk[QPL];  // table rows are zero-padded to 8 quads (get_tables): quads past the window carry no weight
#pragma unroll
	for (int j = 0; j < QPL; ++j) kk[j] = *reinterpret_cast<const uint2 *>(rowp + 4 + 2 * (part + j * LPI));
	const uint32_t *row = s_pl + y * kRS32 + hdr.x * 2u + part * 2u;
	int32_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
	for (int j = 0; j < QPL; ++j) {
		if (LPI > 1 || (uint32_t)j < tx.wquads) {  // LPI == 1: wave-uniform trim of the zero-weight tail
			const uint2 d0 = *reinterpret_cast<const uint2 *>(row + j * LPI * 2);
			const uint2 d1 = *reinterpret_cast<const uint2 *>(row + kPD32 + j * LPI * 2);
			const uint2 d2 = *reinterpret_cast<const uint2 *>(row + 2 * kPD32 + j * LPI * 2);
			a0 = dot2(d0.y, kk[j].y, dot2(d0.x, kk[j].x, a0));
			a1 = dot2(d1.y, kk[j].y, dot2(d1.x, kk[j].x, a1));
			a2 = dot2(d2.y, kk[j].y, dot2(d2.x, kk[j].x, a2));
		}
	}
	a0 = group_sum<LPI>(a0);
	a1 = group_sum<LPI>(a1);
	a2 = group_sum<LPI>(a2);
	if (live && part == 0) {
		const int prec = tx.precision;
		const int32_t init = 1 << (prec - 1);
		uint16_t *t16 = reinterpret_cast<uint16_t *>(s_tmp) + ox * (2 * kHS32) + y;
		t16[0] = (uint16_t)clip8(a0 + init, prec);
		t16[2 * kTD32] = (uint16_t)clip8(a1 + init, prec);
		t16[4 * kTD32] = (uint16_t)clip8(a2 + init, prec);
	}
}

// vertical pass over the transposed planes, window split over LPI lanes; item = (oy fastest, ox),
// so that a lane keeps the same output row (= the same table row) across iterations
// C = 3: out is a slot of 3-byte pixels (shrink16_kernel on RGB frames)
template <int LPI, int C = 4>
__device__ __forceinline__ void fast32_v(const uint32_t *trows, const AxisTab &tx, const AxisTab &ty, const uint32_t *s_tmp,
                                         uint32_t lane, uint32_t nw, uint32_t nh, uint32_t *out)
{
	constexpr int QPL = 8 / LPI;
	const uint32_t items = nw * nh;
	const uint32_t lgy = 31u - (uint32_t)__builtin_clz(nh);
	const uint32_t part = lane % LPI, item0 = lane / LPI;
	const uint32_t oy = item0 & (nh - 1u);  // invariant: the item step (64/LPI) is a multiple of nh
	const uint32_t *rowp = trows + ty.rows_off + oy * ty.row_stride;
	const uint4 hdr = *reinterpret_cast<const uint4 *>(rowp);
	const uint32_t wq = ty.wquads;
	uint2 kk[QPL];  // zero-padded rows: no guard
#pragma unroll
	for (int j = 0; j < QPL; ++j) kk[j] = *reinterpret_cast<const uint2 *>(rowp + 4 + 2 * (part + j * LPI));
	const int px_ = tx.precision, py = ty.precision;
	const int32_t ix = 1 << (px_ - 1), iy = 1 << (py - 1);
	for (uint32_t item = item0; item < ((items + 63u / LPI) & ~(64u / LPI - 1u)); item += 64u / LPI) {
		const bool live = item < items;
		const uint32_t ox = live ? item >> lgy : 0u;
		const uint32_t *colp = s_tmp + ox * kHS32 + hdr.x * 2u + part * 2u;
		int32_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
		for (int j = 0; j < QPL; ++j) {
			if (LPI > 1 || (uint32_t)j < wq) {  // LPI == 1: wave-uniform trim of the zero-weight tail
				const uint2 d0 = *reinterpret_cast<const uint2 *>(colp + j * LPI * 2);
				const uint2 d1 = *reinterpret_cast<const uint2 *>(colp + kTD32 + j * LPI * 2);
				const uint2 d2 = *reinterpret_cast<const uint2 *>(colp + 2 * kTD32 + j * LPI * 2);
				a0 = dot2(d0.y, kk[j].y, dot2(d0.x, kk[j].x, a0));
				a1 = dot2(d1.y, kk[j].y, dot2(d1.x, kk[j].x, a1));
				a2 = dot2(d2.y, kk[j].y, dot2(d2.x, kk[j].x, a2));
			}
		}
		a0 = group_sum<LPI>(a0);
		a1 = group_sum<LPI>(a1);
		a2 = group_sum<LPI>(a2);
		if (live && part == 0) {
			// opaque tile: alpha is the convolution of the constant 255 = the windows' weight sums
			const int32_t ksx = (int32_t)trows[tx.rows_off + ox * tx.row_stride + 2];
			const int32_t ah = (int32_t)clip8(ix + 255 * ksx, px_);
			const uint32_t al = clip8(iy + ah * (int32_t)hdr.z, py);
			uint32_t px = clip8(a0 + iy, py) | (clip8(a1 + iy, py) << 8) | (clip8(a2 + iy, py) << 16) | (al << 24);
			if (al != 255u) px = unpremultiply(px);
			if constexpr (C == 4) {
				out[oy * nw + ox] = px;
			} else {
				uint8_t *o3 = reinterpret_cast<uint8_t *>(out) + 3u * (oy * nw + ox);
				o3[0] = (uint8_t)px;
				o3[1] = (uint8_t)(px >> 8);
				o3[2] = (uint8_t)(px >> 16);
			}
		}
	}
}

// single-pass cases of the fast path (one axis keeps its 32 samples), opaque tile.
// Vertical only: item = (pair of columns, output row) straight on the [y][x] planes; the (row j,
// row j+1) sample pairs dot2 needs are built with two perms per column pair and row pair.
// T = 32: a whole 32x32 LDS image, pixels parked as dwords (out).  T = 16: a 16x16 tile somewhere inside the image (s_pl points at
// its first pixel pair), pixels stored straight to its slot (C bytes each).
template <int T = 32, int C = 4>
__device__ __forceinline__ void fast32_v_only(const uint32_t *trows, const AxisTab &ty, const uint32_t *s_pl, uint32_t lane,
                                              uint32_t nh, uint32_t *out)
{
	constexpr uint32_t kPairs = T / 2;  // column pairs of a row
	const uint32_t lgy = 31u - (uint32_t)__builtin_clz(nh);
	const uint32_t oy = lane & (nh - 1u);  // invariant per lane: 64 is a multiple of nh
	RowRegs r;
	load_row(trows + ty.rows_off + oy * ty.row_stride, r);
	const int prec = ty.precision;
	const int32_t init = 1 << (prec - 1);
	const uint32_t al = clip8(init + 255 * r.ksum, prec);  // constant-255 alpha through the same window
	const uint32_t wq = ty.wquads;
	for (uint32_t i = lane; i < kPairs * nh; i += 64u) {
		const uint32_t qx = i >> lgy;  // column pair
		const uint32_t *colp = s_pl + (r.fq * 4u) * kRS32 + qx;
		int32_t acc[3][2];
#pragma unroll
		for (int c = 0; c < 3; ++c) acc[c][0] = acc[c][1] = init;
#pragma unroll
		for (int q = 0; q < T / 4; ++q) {
			if ((uint32_t)q < wq) {
#pragma unroll
				for (int c = 0; c < 3; ++c) {
					const uint32_t *p = colp + c * kPD32 + (q * 4) * (int)kRS32;
					const uint32_t r0 = p[0], r1 = p[kRS32], r2 = p[2 * kRS32], r3 = p[3 * kRS32];
					const uint32_t l01 = __builtin_amdgcn_perm(r1, r0, 0x05040100u), l23 = __builtin_amdgcn_perm(r3, r2, 0x05040100u);
					const uint32_t h01 = __builtin_amdgcn_perm(r1, r0, 0x07060302u), h23 = __builtin_amdgcn_perm(r3, r2, 0x07060302u);
					acc[c][0] = dot2(l23, r.k[2 * q + 1], dot2(l01, r.k[2 * q], acc[c][0]));
					acc[c][1] = dot2(h23, r.k[2 * q + 1], dot2(h01, r.k[2 * q], acc[c][1]));
				}
			}
		}
		uint2 o;
		o.x = clip8(acc[0][0], prec) | (clip8(acc[1][0], prec) << 8) | (clip8(acc[2][0], prec) << 16) | (al << 24);
		o.y = clip8(acc[0][1], prec) | (clip8(acc[1][1], prec) << 8) | (clip8(acc[2][1], prec) << 16) | (al << 24);
		if (al != 255u) {
			o.x = unpremultiply(o.x);
			o.y = unpremultiply(o.y);
		}
		// pixels (2qx, 2qx+1) of output row oy, row length T
		if constexpr (C == 4) {
			*reinterpret_cast<uint2 *>(out + (oy * kPairs + qx) * 2u) = o;
		} else {
			store_pixel<3>(reinterpret_cast<uint8_t *>(out), (oy * kPairs + qx) * 2u, o.x);
			store_pixel<3>(reinterpret_cast<uint8_t *>(out), (oy * kPairs + qx) * 2u + 1u, o.y);
		}
	}
}

// Horizontal only: item = (output column, pair of rows), results go straight to the slot.
template <int T = 32, int C = 4>
__device__ __forceinline__ void fast32_h_only(const uint32_t *trows, const AxisTab &tx, const uint32_t *s_pl, uint32_t lane,
                                              uint32_t nw, uint32_t *out)
{
	const uint32_t lgx = 31u - (uint32_t)__builtin_clz(nw);
	const uint32_t ox = lane & (nw - 1u);
	RowRegs r;
	load_row(trows + tx.rows_off + ox * tx.row_stride, r);
	const int prec = tx.precision;
	const int32_t init = 1 << (prec - 1);
	const uint32_t al = clip8(init + 255 * r.ksum, prec);
	const uint32_t wq = tx.wquads;
	for (uint32_t i = lane; i < nw * (uint32_t)(T / 2); i += 64u) {  // T / 2 pairs of rows
		const uint32_t yp = i >> lgx;
		const uint32_t *row = s_pl + yp * (2 * kRS32) + r.fq * 2u;
		int32_t acc[3][2];
#pragma unroll
		for (int c = 0; c < 3; ++c) acc[c][0] = acc[c][1] = init;
#pragma unroll
		for (int q = 0; q < T / 4; ++q) {
			if ((uint32_t)q < wq) {
#pragma unroll
				for (int c = 0; c < 3; ++c) {
					const uint2 d = *reinterpret_cast<const uint2 *>(row + c * kPD32 + q * 2);
					const uint2 e = *reinterpret_cast<const uint2 *>(row + c * kPD32 + kRS32 + q * 2);
					acc[c][0] = dot2(d.y, r.k[2 * q + 1], dot2(d.x, r.k[2 * q], acc[c][0]));
					acc[c][1] = dot2(e.y, r.k[2 * q + 1], dot2(e.x, r.k[2 * q], acc[c][1]));
				}
			}
		}
#pragma unroll
		for (uint32_t rr = 0; rr < 2; ++rr) {
			uint32_t px = clip8(acc[0][rr], prec) | (clip8(acc[1][rr], prec) << 8) | (clip8(acc[2][rr], prec) << 16) | (al << 24);
			if (al != 255u) px = unpremultiply(px);
			store_pixel<C>(reinterpret_cast<uint8_t *>(out), (2u * yp + rr) * nw + ox, px);
		}
	}
}

// horizontal pass, item = (ox, pair of rows): nw*16 items, nw/4 per lane, the same ox (table row)
// every time; WQ = quads per window (weights past a lane's own window are zero in the table)
template <int WQ>
__device__ __forceinline__ void fast32_h_pairs(const uint32_t *trows, const AxisTab &tx, const uint32_t *s_pl, uint32_t *s_tmp,
                                               uint32_t lane, uint32_t nw, uint32_t lgx, uint32_t row_pairs = 16u)
{
	const uint32_t ox = lane & (nw - 1u);
	RowRegs r;
	load_row(trows + tx.rows_off + ox * tx.row_stride, r);
	const int prec = tx.precision;
	const int32_t init = 1 << (prec - 1);
	for (uint32_t i = lane; i < nw * row_pairs; i += 64u) {
		const uint32_t yp = i >> lgx;
		const uint32_t *row = s_pl + yp * (2 * kRS32) + r.fq * 2u;
		int32_t a0 = init, a1 = init, a2 = init, b0 = init, b1 = init, b2 = init;
#pragma unroll
		for (int q = 0; q < WQ; ++q) {
			const uint2 d0 = *reinterpret_cast<const uint2 *>(row + q * 2);
			const uint2 e0 = *reinterpret_cast<const uint2 *>(row + kRS32 + q * 2);
			const uint2 d1 = *reinterpret_cast<const uint2 *>(row + kPD32 + q * 2);
			const uint2 e1 = *reinterpret_cast<const uint2 *>(row + kPD32 + kRS32 + q * 2);
			const uint2 d2 = *reinterpret_cast<const uint2 *>(row + 2 * kPD32 + q * 2);
			const uint2 e2 = *reinterpret_cast<const uint2 *>(row + 2 * kPD32 + kRS32 + q * 2);
			const uint32_t k01 = r.k[2 * q], k23 = r.k[2 * q + 1];
			a0 = dot2(d0.y, k23, dot2(d0.x, k01, a0));
			b0 = dot2(e0.y, k23, dot2(e0.x, k01, b0));
			a1 = dot2(d1.y, k23, dot2(d1.x, k01, a1));
			b1 = dot2(e1.y, k23, dot2(e1.x, k01, b1));
			a2 = dot2(d2.y, k23, dot2(d2.x, k01, a2));
			b2 = dot2(e2.y, k23, dot2(e2.x, k01, b2));
		}
		uint32_t *t = s_tmp + ox * kHS32 + yp;
		t[0] = clip8(a0, prec) | (clip8(b0, prec) << 16);
		t[kTD32] = clip8(a1, prec) | (clip8(b1, prec) << 16);
		t[2 * kTD32] = clip8(a2, prec) | (clip8(b2, prec) << 16);
	}
}

__device__ __forceinline__ void resample_fast32_hv(const uint32_t *trows, const AxisTab &tx, const AxisTab &ty,
                                                   uint32_t *s_pl, uint32_t *s_tmp, uint32_t lane, uint32_t nw,
                                                   uint32_t nh, uint32_t *out)
{
	const uint32_t lgx = 31u - (uint32_t)__builtin_clz(nw);  // nw is a power of two <= 16
	if (nw >= 4) {
		switch (tx.wquads) {  // straight-line window code per size: no branches between LDS reads and dot2s
		case 1: fast32_h_pairs<1>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		case 2: fast32_h_pairs<2>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		case 3: fast32_h_pairs<3>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		case 4: fast32_h_pairs<4>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		case 5: fast32_h_pairs<5>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		case 6: fast32_h_pairs<6>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		case 7: fast32_h_pairs<7>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		default: fast32_h_pairs<8>(trows, tx, s_pl, s_tmp, lane, nw, lgx); break;
		}
	} else if (nw == 2) {
		fast32_h_rows<1>(trows, tx, s_pl, s_tmp, lane, nw, lgx);
	} else {
		fast32_h_rows<2>(trows, tx, s_pl, s_tmp, lane, nw, lgx);
	}
	tile_sync<1>();
	const uint32_t items = nw * nh;
	if (items >= 64u) fast32_v<1>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	else if (items >= 32u) fast32_v<2>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	else if (items >= 16u) fast32_v<4>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	else fast32_v<8>(trows, tx, ty, s_tmp, lane, nw, nh, out);
}

// The same for a 16x16 tile that sits somewhere inside the 32x32 LDS image (s_pl points at its first pixel
// pair): windows of at most 4 quads, 16 source rows, nw and nh in {8, 4, 2, 1}.
template <int C = 4>
__device__ __forceinline__ void resample_fast16_hv(const uint32_t *trows, const AxisTab &tx, const AxisTab &ty, const uint32_t *s_pl,
                                                   uint32_t *s_tmp, uint32_t lane, uint32_t nw, uint32_t nh, uint32_t *out)
{
	const uint32_t lgx = 31u - (uint32_t)__builtin_clz(nw);
	if (nw >= 4) {
		switch (tx.wquads) {
		case 1: fast32_h_pairs<1>(trows, tx, s_pl, s_tmp, lane, nw, lgx, 8u); break;
		case 2: fast32_h_pairs<2>(trows, tx, s_pl, s_tmp, lane, nw, lgx, 8u); break;
		case 3: fast32_h_pairs<3>(trows, tx, s_pl, s_tmp, lane, nw, lgx, 8u); break;
		default: fast32_h_pairs<4>(trows, tx, s_pl, s_tmp, lane, nw, lgx, 8u); break;
		}
	} else if (nw == 2) {
		fast32_h_rows<2>(trows, tx, s_pl, s_tmp, lane, nw, lgx, 16u);
	} else {
		fast32_h_rows<4>(trows, tx, s_pl, s_tmp, lane, nw, lgx, 16u);
	}
	tile_sync<1>();
	const uint32_t items = nw * nh;
	if (items >= 64u) fast32_v<1, C>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	else if (items >= 32u) fast32_v<2, C>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	else if (items >= 16u) fast32_v<4, C>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	else fast32_v<8, C>(trows, tx, ty, s_tmp, lane, nw, nh, out);
	tile_sync<1>();  // the next tile of the group reuses the transposed planes
}

// ---------------------------------------------------------------------------
// The same two-pass convolution on the matrix cores, for 32x32 -> nw x nh with nw, nh in {16, 8}:
// the classes whose windows are long AND whose outputs are many, i.e. where the dot2 form above
// spends the most vector instructions.  Integer-exact: v_mfma_i32_16x16x32_i8 multiplies signed bytes,
// so a pixel enters as p - 128 and an i16 weight as two signed bytes K = 256 K_hi + K_lo:
//     sum p K = 256 sum (p-128) K_hi + sum (p-128) K_lo + 128 sum K
// (two products per output block; the last term and the rounding half come in as the C operand).
//
//   horizontal  T[y][ox] = clip8(sum_x P[y][x] Kx[ox][x])   D = A B: A = pixel rows (16 per product),
//               B = weights [x][ox]; the accumulator holds column ox = lane & 15, rows 4g + r (g = lane >> 4)
//   vertical    O[oy][ox] = clip8(sum_y Ky[oy][y] T[y][ox]) D = A B: A = weights [oy][y], B = T.
// T never leaves the registers: after the two horizontal products (rows 0..15, 16..31) lane (ox, g)
// holds T[4g + r][ox] and T[16 + 4g + r][ox], which IS a B operand whose k slots are the rows
// src(g, j) (pxz_internal.h) -- so the weight operand is stored with its k slots in that order, and the
// pixel operand of the horizontal product reads its 8 source columns in that order too (one table
// serves both passes, the axes of a 32x32 tile being alike).
// ---------------------------------------------------------------------------
typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int BYTE>
__device__ __forceinline__ void put_byte_shr(uint32_t &dst, uint32_t value, uint32_t shift)
{
	// dst.byte[BYTE] = (value >> shift) & 0xff, other bytes kept: one SDWA shift
	if constexpr (BYTE == 0)
		asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(shift), "v"(value));
	else if constexpr (BYTE == 1)
		asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(shift), "v"(value));
	else if constexpr (BYTE == 2)
		asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(shift), "v"(value));
	else
		asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(shift), "v"(value));
}

__device__ __forceinline__ uint32_t clamp_fixed(int32_t hi, int32_t lo, int32_t top)
{
	const int32_t v = (int32_t)(((uint32_t)hi << 8) + (uint32_t)lo);  // 256 * hi + lo (the bias is already in lo)
	int32_t r;  // clip8 before its shift: median of (v, 0, top); top is a run-time value, so spell the instruction
	asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "s"(top));
	return (uint32_t)r;
}

// NCH = 3: opaque tile, alpha from the weight sums.  NCH = 4: the planes hold premultiplied colours and the
// alpha plane; all four are convolved and every output pixel is un-premultiplied (fir's U8x4 path).
template <int NCH>
__device__ __forceinline__ void resample_mfma32(const uint32_t *s_tab, const AxisTab &tx, const AxisTab &ty, const uint32_t *s_pl,
                                                uint32_t lane, uint32_t nw, uint32_t nh, uint32_t *out)
{
	const uint32_t o = lane & 15u, g = lane >> 4;
	const uint32_t *mx = s_tab + tx.mf_off, *my = s_tab + ty.mf_off;
	const long kx_lo = *reinterpret_cast<const long *>(mx + 2u * lane), kx_hi = *reinterpret_cast<const long *>(mx + 128u + 2u * lane);
	const long ky_lo = *reinterpret_cast<const long *>(my + 2u * lane), ky_hi = *reinterpret_cast<const long *>(my + 128u + 2u * lane);
	const int32_t bx = (int32_t)mx[256u + o];
	const v4i32 cx = {bx, bx, bx, bx};
	const v4i32 cy = *reinterpret_cast<const v4i32 *>(my + 256u + 4u * g);
	const v4i32 zero = {0, 0, 0, 0};
	const uint32_t px_ = tx.precision, py = ty.precision;
	const int32_t top_x = (int32_t)((256u << px_) - 1u), top_y = (int32_t)((256u << py) - 1u);
	uint32_t pix[4] = {0xff000000u, 0xff000000u, 0xff000000u, 0xff000000u};
	const uint32_t *rowp = s_pl + o * kRS32 + 2u * g;
#pragma unroll
	for (uint32_t c = 0; c < (uint32_t)NCH; ++c) {
		uint32_t t[2];
#pragma unroll
		for (uint32_t mb = 0; mb < 2; ++mb) {
			const uint32_t *row = rowp + c * kPD32 + mb * (16u * kRS32);
			const uint2 d0 = lds_load2(row);       // columns 4g .. 4g+3
			const uint2 d1 = lds_load2(row + 8u);  // columns 16+4g .. 16+4g+3
			const uint32_t a0 = __builtin_amdgcn_perm(d0.y, d0.x, 0x06040200u) ^ 0x80808080u;
			const uint32_t a1 = __builtin_amdgcn_perm(d1.y, d1.x, 0x06040200u) ^ 0x80808080u;
			const long av = (long)(((unsigned long long)a1 << 32) | (unsigned long long)a0);
			const v4i32 lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, kx_lo, cx, 0, 0, 0);
			const v4i32 hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, kx_hi, zero, 0, 0, 0);
			uint32_t packed = 0;
			put_byte_shr<0>(packed, clamp_fixed(hi[0], lo[0], top_x), px_);
			put_byte_shr<1>(packed, clamp_fixed(hi[1], lo[1], top_x), px_);
			put_byte_shr<2>(packed, clamp_fixed(hi[2], lo[2], top_x), px_);
			put_byte_shr<3>(packed, clamp_fixed(hi[3], lo[3], top_x), px_);
			t[mb] = packed ^ 0x80808080u;
		}
		const long tv = (long)(((unsigned long long)t[1] << 32) | (unsigned long long)t[0]);
		const v4i32 lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_lo, tv, cy, 0, 0, 0);
		const v4i32 hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_hi, tv, zero, 0, 0, 0);
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t v = clamp_fixed(hi[r], lo[r], top_y);
			if (c == 0) put_byte_shr<0>(pix[r], v, py);
			else if (c == 1) put_byte_shr<1>(pix[r], v, py);
			else if (c == 2) put_byte_shr<2>(pix[r], v, py);
			else put_byte_shr<3>(pix[r], v, py);
		}
	}
	if constexpr (NCH == 4) {
#pragma unroll
		for (int r = 0; r < 4; ++r) pix[r] = unpremultiply(pix[r]);
	} else if (!(mx[288] & my[288])) {
		// opaque tile: alpha is the convolution of the constant 255 = the windows' weight sums (fast32_v);
		// the table says when that is 255 for every output of the axis
		const int32_t ah = (int32_t)clip8((1 << (px_ - 1)) + 255 * (int32_t)mx[272u + o], (int)px_);
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t al = clip8((1 << (py - 1)) + ah * (int32_t)my[272u + 4u * g + (uint32_t)r], (int)py);
			pix[r] = (pix[r] & 0x00ffffffu) | (al << 24);
			if (al != 255u) pix[r] = unpremultiply(pix[r]);
		}
	}
	if (o < nw) {
#pragma unroll
		for (uint32_t r = 0; r < 4; ++r) {
			const uint32_t oy = 4u * g + r;
			if (oy < nh) out[oy * nw + o] = pix[r];
		}
	}
}

// The matrix-core form for narrow outputs, 32x32 -> nw x nh with nw in {4, 2, 1}, nh <= 16, opaque tile whose alpha
// stays 255 (both tables say so): the three channels share ONE accumulator.  Column n of the horizontal product is
// (channel n / nw, output column n % nw) -- the weight operand of channel c is the level's table in the columns of
// channel c and zero elsewhere (a lane picks its own row of the table or an all-zero one), and the three products
// accumulate: D[y][(c, ox)] = sum_c' sum_x P_c'[y][x] B_c'[x][(c, ox)].  One clamp per 16 rows instead of three, one
// vertical product instead of three, and the columns of a fourth "channel" carry the constant 255 (bias = the clamp's
// top) through the vertical product: the alpha byte.  Lane (n, g) ends with channel n / nw of the pixels (4g + r, n % nw)
// and stores them as bytes of the parked pixels.  Same integers as resample_mfma32, 14 MFMAs + ~85 vector instructions
// (the dot2 form: ~125 for a 2x1 tile; resample_mfma32: ~170).
__device__ __forceinline__ void resample_mfma32_narrow(const uint32_t *s_tab, const AxisTab &tx, const AxisTab &ty, const uint32_t *s_pl,
                                                       uint32_t lane, uint32_t nw, uint32_t nh, uint32_t *out)
{
	const uint32_t o = lane & 15u, g = lane >> 4;
	const uint32_t lgw = nw >> 1;  // 1, 2, 4 -> 0, 1, 2
	const uint32_t ch = o >> lgw, ox = o & (nw - 1u);
	const uint32_t *mx = s_tab + tx.mf_off, *my = s_tab + ty.mf_off;
	const uint32_t own = 2u * (16u * g + ox), none = 2u * (16u * g + 15u);  // (rows >= the output size hold zero weights)
	const long ky_lo = *reinterpret_cast<const long *>(my + 2u * lane), ky_hi = *reinterpret_cast<const long *>(my + 128u + 2u * lane);
	const uint32_t px_ = tx.precision, py = ty.precision;
	const int32_t top_x = (int32_t)((256u << px_) - 1u), top_y = (int32_t)((256u << py) - 1u);
	const int32_t bx = ch == 3u ? top_x : (int32_t)mx[256u + ox];
	const v4i32 cy = *reinterpret_cast<const v4i32 *>(my + 256u + 4u * g);
	const v4i32 zero = {0, 0, 0, 0};
	v4i32 lo[2] = {{bx, bx, bx, bx}, {bx, bx, bx, bx}}, hi[2] = {zero, zero};
	const uint32_t *rowp = s_pl + o * kRS32 + 2u * g;
#pragma unroll
	for (uint32_t c = 0; c < 3; ++c) {
		const uint32_t sel = ch == c ? own : none;
		const long k_lo = *reinterpret_cast<const long *>(mx + sel), k_hi = *reinterpret_cast<const long *>(mx + 128u + sel);
#pragma unroll
		for (uint32_t mb = 0; mb < 2; ++mb) {
			const uint32_t *row = rowp + c * kPD32 + mb * (16u * kRS32);
			const uint2 d0 = lds_load2(row);       // columns 4g .. 4g+3
			const uint2 d1 = lds_load2(row + 8u);  // columns 16+4g .. 16+4g+3
			const uint32_t a0 = __builtin_amdgcn_perm(d0.y, d0.x, 0x06040200u) ^ 0x80808080u;
			const uint32_t a1 = __builtin_amdgcn_perm(d1.y, d1.x, 0x06040200u) ^ 0x80808080u;
			const long av = (long)(((unsigned long long)a1 << 32) | (unsigned long long)a0);
			lo[mb] = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, k_lo, lo[mb], 0, 0, 0);
			hi[mb] = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, k_hi, hi[mb], 0, 0, 0);
		}
	}
	uint32_t t[2];
#pragma unroll
	for (uint32_t mb = 0; mb < 2; ++mb) {
		uint32_t packed = 0;
		put_byte_shr<0>(packed, clamp_fixed(hi[mb][0], lo[mb][0], top_x), px_);
		put_byte_shr<1>(packed, clamp_fixed(hi[mb][1], lo[mb][1], top_x), px_);
		put_byte_shr<2>(packed, clamp_fixed(hi[mb][2], lo[mb][2], top_x), px_);
		put_byte_shr<3>(packed, clamp_fixed(hi[mb][3], lo[mb][3], top_x), px_);
		t[mb] = packed ^ 0x80808080u;
	}
	const long tv = (long)(((unsigned long long)t[1] << 32) | (unsigned long long)t[0]);
	const v4i32 vlo = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_lo, tv, cy, 0, 0, 0);
	const v4i32 vhi = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_hi, tv, zero, 0, 0, 0);
	// rows 4g + r of column (ch, ox): byte ch of pixel (4g + r) * nw + ox.  nh is a power of two: a lane with 4g < nh has
	// min(nh, 4) rows (scalar tests); rows past nh are not produced.
	if (o < 4u * nw && 4u * g < nh) {
		uint8_t *dst = reinterpret_cast<uint8_t *>(out) + (4u * g * nw + ox) * 4u + ch;
		dst[0] = (uint8_t)(clamp_fixed(vhi[0], vlo[0], top_y) >> py);
		if (nh > 1u) dst[nw * 4u] = (uint8_t)(clamp_fixed(vhi[1], vlo[1], top_y) >> py);
		if (nh > 2u) {
			dst[2u * nw * 4u] = (uint8_t)(clamp_fixed(vhi[2], vlo[2], top_y) >> py);
			dst[3u * nw * 4u] = (uint8_t)(clamp_fixed(vhi[3], vlo[3], top_y) >> py);
		}
	}
}

// The two-pass convolution of a GROUP of four 16x16 tiles (a 32x32 region of LDS planes, shrink16_kernel) as ONE set of
// matrix-core products (round 4): the weight operands are block-diagonal.  A k slot (g, j) of v_mfma_i32_16x16x32_i8 stands for
// sample 4g + j of the FIRST 16 (j < 4) or of the SECOND 16 (j >= 4) of the 32, so
//   horizontal, half mb (rows 16 mb ..): B[k][n] = Wx of tile (dx = n >> 3, dy = mb) for output column n & 7 in the k slots of its
//               own 16 source columns and zero in the other 16: one product gives T of the left tile in columns 0..7 and of the
//               right tile in columns 8..15, each at its own level (a lane reads its own tile's table: levels are per lane);
//   vertical    A[m][k] = Wy of the tile in row dy = m >> 3 for output row m & 7, in the k slots of its own 16 source rows.  The
//               left and the right tiles of a row have different y levels, so there are two products into ONE accumulator:
//               A of the left tiles times T with columns 8..15 zeroed, plus A of the right tiles times T with columns 0..7 zeroed
//               (a zero byte is p - 128 = 0: it adds nothing, the bias of the lane's own tile carries its 128 * sum K).
// 24 MFMAs and ~230 vector instructions for the four tiles; the dot2 form (resample_fast16_hv) took ~118 per tile.  Same
// integers: the clamp after each pass, the precisions and the biases are those of the lane's tile.  Opaque tiles whose alpha
// stays 255 (every table involved says so); tiles outside `mask` (clone, one-pass, nothing) ride along and are not stored.
__device__ __forceinline__ uint32_t clamp_fixed_v(int32_t hi, int32_t lo, int32_t top)
{
	const int32_t v = (int32_t)(((uint32_t)hi << 8) + (uint32_t)lo);
	int32_t r;
	asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "v"(top));
	return (uint32_t)r;
}

// Per-lane views of the group (set up by shrink16_kernel while it decides the tiles one by one, so that no per-tile scalar
// outlives its tile): tx[mb] = table of the tile in this lane's COLUMN half (n >> 3) and row half mb (the B operand of the
// horizontal product of half mb); ty[side] = table of the tile in column `side` and the ROW half this lane stands for as a row
// of the weight operand (m >> 3, m = lane & 15); tyo / nw / nh / dst / ok = the tile this lane's outputs belong to (column half
// n >> 3, row half g >> 1): its y table, reduced size, slot, and whether it is one of the two-pass tiles at all.  Tables of
// views without a two-pass tile: any valid one (those columns and rows are not stored).
template <int C>
__device__ __forceinline__ void resample_group16_mfma(const uint32_t *s_tab, const uint32_t (&tx)[2], const uint32_t (&ty)[2], uint32_t tyo,
                                                      const uint32_t *s_pl, uint32_t lane, uint32_t nw, uint32_t nh, bool ok, uint8_t *dst)
{
	const uint32_t n = lane & 15u, g = lane >> 4, o = n & 7u;
	const bool second = n >= 8u;  // as a column: a right tile; as a row of a weight operand: a bottom tile
	const v4i32 zero = {0, 0, 0, 0};
	auto operand = [&](uint32_t w) -> long {  // the lane's four weight bytes in the k slots of its own 16 samples
		return (long)(second ? (unsigned long long)w << 32 : (unsigned long long)w);
	};
	long kx_lo[2], kx_hi[2], ky_lo[2], ky_hi[2];
	int32_t bx[2], top_x[2];
	uint32_t px_[2];
#pragma unroll
	for (uint32_t mb = 0; mb < 2; ++mb) {
		const uint32_t *t = s_tab + tx[mb];
		kx_lo[mb] = operand(t[o * 4u + g]);
		kx_hi[mb] = operand(t[32u + o * 4u + g]);
		bx[mb] = (int32_t)t[64u + o];
		px_[mb] = t[81];
		top_x[mb] = (int32_t)((256u << px_[mb]) - 1u);
	}
#pragma unroll
	for (uint32_t side = 0; side < 2; ++side) {
		const uint32_t *t = s_tab + ty[side];
		ky_lo[side] = operand(t[o * 4u + g]);
		ky_hi[side] = operand(t[32u + o * 4u + g]);
	}
	// this lane's outputs: column n, rows 4g + r -> pixel (ox = o, oy = 4 (g & 1) + r) of its tile
	const uint32_t *to = s_tab + tyo;
	const v4i32 cy = *reinterpret_cast<const v4i32 *>(to + 64u + 4u * (g & 1u));
	const uint32_t py = to[81];
	const int32_t top_y = (int32_t)((256u << py) - 1u);
	uint32_t pix[4] = {0xff000000u, 0xff000000u, 0xff000000u, 0xff000000u};
	const uint32_t *rowp = s_pl + n * kRS32 + 2u * g;
#pragma unroll
	for (uint32_t c = 0; c < 3; ++c) {
		uint32_t t[2];
#pragma unroll
		for (uint32_t mb = 0; mb < 2; ++mb) {
			const uint32_t *row = rowp + c * kPD32 + mb * (16u * kRS32);
			const uint2 d0 = lds_load2(row);       // columns 4g .. 4g+3 (left tile)
			const uint2 d1 = lds_load2(row + 8u);  // columns 16+4g .. 16+4g+3 (right tile)
			const uint32_t a0 = __builtin_amdgcn_perm(d0.y, d0.x, 0x06040200u) ^ 0x80808080u;
			const uint32_t a1 = __builtin_amdgcn_perm(d1.y, d1.x, 0x06040200u) ^ 0x80808080u;
			const long av = (long)(((unsigned long long)a1 << 32) | (unsigned long long)a0);
			const v4i32 cx = {bx[mb], bx[mb], bx[mb], bx[mb]};
			const v4i32 lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, kx_lo[mb], cx, 0, 0, 0);
			const v4i32 hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, kx_hi[mb], zero, 0, 0, 0);
			uint32_t packed = 0;
			put_byte_shr<0>(packed, clamp_fixed_v(hi[0], lo[0], top_x[mb]), px_[mb]);
			put_byte_shr<1>(packed, clamp_fixed_v(hi[1], lo[1], top_x[mb]), px_[mb]);
			put_byte_shr<2>(packed, clamp_fixed_v(hi[2], lo[2], top_x[mb]), px_[mb]);
			put_byte_shr<3>(packed, clamp_fixed_v(hi[3], lo[3], top_x[mb]), px_[mb]);
			t[mb] = packed ^ 0x80808080u;
		}
		const uint32_t l0 = second ? 0u : t[0], l1 = second ? 0u : t[1], r0 = second ? t[0] : 0u, r1 = second ? t[1] : 0u;
		const long tl = (long)(((unsigned long long)l1 << 32) | (unsigned long long)l0);
		const long tr = (long)(((unsigned long long)r1 << 32) | (unsigned long long)r0);
		v4i32 lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_lo[0], tl, cy, 0, 0, 0);
		lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_lo[1], tr, lo, 0, 0, 0);
		v4i32 hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_hi[0], tl, zero, 0, 0, 0);
		hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(ky_hi[1], tr, hi, 0, 0, 0);
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t v = clamp_fixed_v(hi[r], lo[r], top_y);
			if (c == 0) put_byte_shr<0>(pix[r], v, py);
			else if (c == 1) put_byte_shr<1>(pix[r], v, py);
			else put_byte_shr<2>(pix[r], v, py);
		}
	}
	if (ok && o < nw) {
#pragma unroll
		for (uint32_t r = 0; r < 4; ++r) {
			const uint32_t oy = 4u * (g & 1u) + r;
			if (oy < nh) store_pixel<C>(dst, oy * nw + o, pix[r]);
		}
	}
}

// Source pixels are read once per launch: loads marked non-temporal ("nt": stream through the caches, do not displace
// what is reused).  On the headline kernel that alone is worth 6-8 % -- the tile reads no longer evict each other's
// not-yet-consumed lines and the output stream's lines from L2 (round 2, tools: A/B of two builds on one box).
__device__ __forceinline__ uint4 stream_load4(const uint8_t *p)
{
	typedef uint32_t u32q __attribute__((ext_vector_type(4)));
	const u32q v = __builtin_nontemporal_load(reinterpret_cast<const u32q *>(p));
	return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint2 stream_load2(const uint8_t *p)
{
	typedef uint32_t u32d __attribute__((ext_vector_type(2)));
	const u32d v = __builtin_nontemporal_load(reinterpret_cast<const u32d *>(p));
	return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint3 stream_load3(const uint8_t *p)
{
	typedef uint32_t u32t __attribute__((ext_vector_type(3)));
	const u32t v = __builtin_nontemporal_load(reinterpret_cast<const u32t *>(p));
	return make_uint3(v.x, v.y, v.z);
}
// The same from a wave-uniform pointer and a 32-bit lane offset: the scalar-base form of global_load (pointer in two scalar
// registers, offset in one vector register, no address arithmetic on the vector unit).  The pointer passes through an empty
// asm as a scalar: left to add pointer and offset up as it likes, the compiler forms the first address per lane and steps
// from load to load with 64-bit vector adds.  Behind the asm the pointer is named as global memory again, or the loads
// come out as flat ones.
// The offset has to come out of such an asm too (lane_offset_here), in the basic block of the loads: widened to 64 bits
// once, outside the loop that uses it, it reaches the load as a 64-bit register pair and the form is not chosen.
typedef const __attribute__((address_space(1))) uint8_t *global_bytes;
__device__ __forceinline__ uint32_t lane_offset_here(uint32_t off)
{
	asm volatile("" : "+v"(off));
	return off;
}
__device__ __forceinline__ global_bytes uniform_global_at(const uint8_t *&base, uint32_t off)
{
	asm volatile("" : "+s"(base));
	return (global_bytes)base + off;
}
__device__ __forceinline__ uint4 stream_load4_at(const uint8_t *&base, uint32_t off)
{
	typedef uint32_t u32q __attribute__((ext_vector_type(4)));
	const u32q v = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) u32q *>(uniform_global_at(base, off)));
	return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint3 stream_load3_at(const uint8_t *&base, uint32_t off)
{
	typedef uint32_t u32t __attribute__((ext_vector_type(3)));
	const u32t v = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) u32t *>(uniform_global_at(base, off)));
	return make_uint3(v.x, v.y, v.z);
}

// Fast-path eligibility of a tile (full 32x32 RGBA, 16-byte aligned rows) and its first byte.
template <int C = 4, class Args>
__device__ __forceinline__ bool fast32_tile_src(const Args &a, uint32_t tile_g, const uint8_t *&src)
{
	if (tile_g >= a.n_tiles) return false;
	const uint32_t frame = fastdiv(tile_g, a.div_tpf);
	const uint32_t t = tile_g - frame * a.tiles_per_frame;
	const uint32_t ty = fastdiv(t, a.div_cols), tx = t - ty * a.cols;
	src = a.src + (size_t)frame * a.frame_stride + (size_t)(ty * 32u) * a.pitch + (size_t)(tx * 32u) * (uint32_t)C;
	return tx < a.full_cols && ty < a.full_rows;  // full size; the alignment of the batch is folded in by the host
}
// Issues the four loads of a lane's share of a fast tile: rows l/8 + 8k, pixel quad l%8 -- 16 bytes of an RGBA row, 12
// of an RGB one (pre[k].w unused).
// The address is split where the hardware splits it: the tile's first byte and the three steps of eight rows are the same
// for the whole wave and stay on the scalar unit (a 64-bit pointer in two scalar registers), the lane's own part
// (lane/8 rows + its pixel quad) is ONE 32-bit offset that does not change from tile to tile -- the scalar-base form of
// global_load.  Added up per lane it was five 64-bit vector adds per tile.  The offset fits 32 bits for every batch the
// host lets onto the fast path (fast32_lane_offset_fits, pxz_internal.h).
template <int C = 4, class Args>
__device__ __forceinline__ void fast32_prefetch(const Args &a, uint32_t tile_g, uint32_t lane, uint4 (&pre)[4], bool &valid, bool skip_loads = false)
{
	const uint8_t *src;
	valid = fast32_tile_src<C>(a, tile_g, src);
	if (valid && !skip_loads) {  // (skip_loads: the caller knows it will not look at the pixels -- a tile the detector already copied)
		const uint32_t off = lane_offset_here((lane >> 3) * a.pitch + (lane & 7u) * (4u * (uint32_t)C));
		const uint8_t *rows = src;  // wave-uniform
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			if constexpr (C == 4) {
				pre[k] = stream_load4_at(rows, off);
			} else {
				const uint3 v = stream_load3_at(rows, off);  // rows are 4-byte aligned
				pre[k] = make_uint4(v.x, v.y, v.z, 0u);
			}
			rows += (size_t)8 * a.pitch;
		}
	}
}

// Does sums[] already hold this tile's Oklab value (left by an oklab_kernel launch)?  Interior: the full tiles, plus the
// ragged last row of the square sizes when its height is a whole number of bands (ok_rows).  Edges: the regions a
// run-time-geometry launch has taken (ok_edges: bit 0 right column, bit 1 bottom row, bit 2 corner tile).
template <class Args>
__device__ __forceinline__ bool oklab_value_given(const Args &a, uint32_t tx, uint32_t ty)
{
	const bool in_x = tx < a.full_cols, in_y = ty < a.full_rows;
	if (in_x && ty < a.ok_rows) return true;  // (ok_rows >= full_rows)
	const uint32_t bit = in_x ? 2u : (in_y ? 1u : 4u);
	return (a.ok_edges & bit) != 0u;
}

// Detector result of one tile -> stored block value (and the raw detector outputs for pxz_lod_*):
// the f64 part of get_block_variance_directionally (operations.rs:253-258), shrink_*'s closures
// (pixlzr.rs:177-178, :199) and reduce_image_section's value (operations.rs:154).
constexpr uint32_t kDeferredKey = 0xffffffffu;  // sums[] of a tile shrink32_kernel handed to the worklist
__device__ __forceinline__ void finish_tile(const uint2 key, uint32_t w, uint32_t h, uint32_t mode, float factor, float *value,
                                            float *lod0, float *lod1, uint32_t tile_g)
{
	float raw0, raw1, v0, v1;
	if (mode == 1) {
		const uint64_t fac = (uint64_t)(w - 2) * (uint64_t)(h - 2) * 4096ull;  // operations.rs:253-254
		if (fac == 0) {
			// 0/0 on the reference's x86-64 target is the negative default NaN:
			// parse_value turns it into max(1+NaN, 0) = 0 -> stored value 0
			raw0 = raw1 = __uint_as_float(0xFFC00000u);
			v0 = v1 = 0.0f;
		} else {
			const double d = (double)fac;
			raw0 = (float)((double)key.x / d);  // :256
			raw1 = (float)((double)key.y / d);  // :257
			v0 = parse_value(raw0 * factor);    // pixlzr.rs:199
			v1 = parse_value(raw1 * factor);
		}
	} else {
		raw0 = raw1 = __uint_as_float(key.x);
		v0 = v1 = parse_value(raw0);  // pixlzr.rs:177-178
	}
	if (value) value[tile_g] = hypot_f32(v0, v1);  // operations.rs:154
	if (lod0) lod0[tile_g] = raw0;
	if (lod1) lod1[tile_g] = raw1;
}

// ---- diagnostic build only (-DPXZ_STAMPS): per-phase wave-cycle shares of shrink32_kernel.
// Stamp values leave through a buffer of their own (a.work, past the worklist); no output depends on them.
#ifdef PXZ_STAMPS
__device__ __forceinline__ unsigned long long stamp_now()
{
	unsigned long long t;
	__builtin_amdgcn_sched_barrier(0);
	asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
	__builtin_amdgcn_sched_barrier(0);
	return t;
}
#define PXZ_STAMP(i)                                   \
	do {                                               \
		const unsigned long long now_ = stamp_now();   \
		st_acc[i] += now_ - st_last;                   \
		st_last = now_;                                \
	} while (0)
#else
#define PXZ_STAMP(i) \
	do {             \
	} while (0)
#endif

// Worklist appends, batched: a global atomic on ONE address completes every ~12 ns chip-wide, so a frame whose
// every tile is listed (transparent frames: 259 200 tiles) would spend 3 ms on the counter alone.  Each wave
// (or block) parks up to kListBatch tile numbers in LDS and reserves their list slots with one atomic.
constexpr uint32_t kListBatch = 16;
__device__ __forceinline__ void list_flush(uint32_t *buf, uint32_t &cnt, uint32_t *list, uint32_t *counter, uint32_t lane)
{
	if (cnt == 0u) return;
	uint32_t base = 0;
	if (lane == 0u) base = atomicAdd(counter, cnt);
	base = __builtin_amdgcn_readfirstlane(base);
	asm volatile("" ::: "memory");
	if (lane < cnt) list[base + lane] = buf[lane];
	asm volatile("" ::: "memory");
	cnt = 0u;
}
// cnt is uniform over the lanes that call this (a wave, or thread 0 of a block with lane == 0 semantics)
__device__ __forceinline__ void list_push(uint32_t *buf, uint32_t &cnt, uint32_t tile, uint32_t *list, uint32_t *counter,
										   uint32_t lane)
{
	if (lane == 0u) buf[cnt] = tile;
	++cnt;
	if (cnt == kListBatch) list_flush(buf, cnt, list, counter, lane);
}

// ---------------------------------------------------------------------------
// Flat tile spaces (varied batches, pixel windows): a table of owners (VariedImage, WindowEntry), each with a first tile
// tile0 and a first tile row row0, both ascending.  Who holds a flat tile or row number finds its owner here.
// ---------------------------------------------------------------------------

// the last entry of table[0 .. n) whose key member is <= key (n >= 1, table[0]'s key is 0)
template <class Entry>
__device__ __forceinline__ uint32_t owner_of(const Entry *table, uint32_t n, uint32_t key, uint32_t Entry::*first)
{
	uint32_t lo = 0, hi = n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (table[mid].*first <= key) lo = mid;
		else hi = mid - 1u;
	}
	return lo;
}

// The wave-per-tile kernels search a copy of the owners' first tiles in LDS while the call has at most kVxImages owners
// (t0_dw dwords, set by varied_expand_geom; 0: the table itself, in global memory).  distortion_kernel (pxz_distortion.hip) has
// its own copy of this search and of bad_stored_size: a fix here belongs there too.
constexpr uint32_t kVxImages = 2048;  // owners whose first tiles a block keeps in LDS (8 KB)

// every thread of the block calls this once, before the tile loop
template <class Entry>
__device__ __forceinline__ void stage_first_tiles(uint32_t *s_t0, uint32_t t0_dw, const Entry *table, uint32_t n)
{
	for (uint32_t i = threadIdx.x; i < t0_dw; i += blockDim.x) s_t0[i] = i < n ? table[i].tile0 : 0xffffffffu;
	__syncthreads();
}

// owner_of by tile0 for a wave-uniform t: the compare runs on the scalar unit (the first tile read goes through
// readfirstlane as an unsigned value; its sign extension faulted here once)
template <class Entry>
__device__ __forceinline__ uint32_t owner_of_tile(const uint32_t *s_t0, uint32_t t0_dw, const Entry *table, uint32_t n, uint32_t t)
{
	uint32_t lo = 0, hi = n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		const uint32_t t0 = t0_dw ? s_t0[mid] : table[mid].tile0;
		if ((uint32_t)__builtin_amdgcn_readfirstlane(t0) <= t) lo = mid;
		else hi = mid - 1u;
	}
	return lo;
}

// A stored size tw x th that a tile of fw x fh cannot have (zero, or beyond its place): the tile is skipped as
// pxz_expand_frames_device skips it -- status bit 0 and, where the call has flags, the owner's.  True: skip.
__device__ __forceinline__ bool bad_stored_size(uint32_t tw, uint32_t th, uint32_t fw, uint32_t fh, uint32_t lane, uint32_t *status,
                                                uint32_t *flags, uint32_t owner)
{
	if (tw != 0u && th != 0u && tw <= fw && th <= fh) return false;
	if (lane == 0u) {
		atomicOr(status, 1u);
		if (flags) flags[owner] = 1u;
	}
	return true;
}

// ---------------------------------------------------------------------------
// One stored tile of a varied batch back at its full size, in an LDS image: steps 2 and 3 of varied_expand_kernel
// (pxz_varied_expand.hip), which distortion_kernel (pxz_distortion.hip) and window_expand_kernel (pxz_window.hip) run too, one
// wave per tile (G = 64, `lane` the lane, wsync a wave barrier), and reshrink_ladder_kernel with a whole block per tile
// (reshrink_tile_image, pxz_varied_tile.h: G = 256, `lane` the thread, wsync = __syncthreads()).  G is the number of threads
// that share the tile; all of them make the call.
//   2. the stored pixels (tw x th at src, tightly packed) -> one dword per pixel in s_src (RGBA under a convolution
//      alpha-premultiplied as fir does), and the windows of both axis tables -- directory entry (full size, stored size) of
//      a.dir -- in s_wx / s_wy: per output sample a.wdw dwords, first | count << 16, then the weights as i16 pairs;
//   3. the resize of PixlzrBlock::resize (block.rs:273-334): a clone when the sizes agree, the Nearest pick, else the
//      horizontal then the vertical pass with i16 weights and i32 accumulators, u8 between the passes, un-premultiplied
//      at the end.
// Returns the plane (s_src or s_tmp) that holds the fw x fh result, one dword per pixel; wsync() has run behind its last
// write.  stage_x / stage_y false: the windows of that axis are in s_wx / s_wy already (the same full and stored size as
// the tile these threads resized before).  Args: TileResizeArgs, or DistortionArgs (which names the same fields).
// Of global memory, step 2 reads the tile's own slot and the tables and nothing else: an RGB pixel is one unaligned dword from
// its byte address, and the address is clamped at slot_bytes - 4 (the slot's last pixel is read from a byte earlier and
// shifted), so no load reaches behind the slot.  The re-shrink's in-place guarantee -- a block reads only its own tile's slot,
// and before its first store -- rests on that.
// ---------------------------------------------------------------------------

// the clamp spelled as an instruction: left to the compiler, clip8(a) | clip8(b) << 8 of an RGB pixel became
// v_ashr_pk_u8_i32, whose upper half keeps what the destination held (pxz_expand.hip)
__device__ __forceinline__ uint32_t clip8_med3(int32_t acc, int prec)
{
	const int32_t v = acc >> prec;
	int32_t r;
	asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "v"(255));
	return (uint32_t)r;
}

template <int C, uint32_t G = 64u, class Args, class Sync>
__device__ __forceinline__ const uint32_t *varied_resize_tile(const Args &a, uint32_t lane, const uint8_t *src, uint32_t tw, uint32_t th,
                                                              uint32_t fw, uint32_t fh, uint32_t *s_src, uint32_t *s_tmp, uint32_t *s_wx,
                                                              uint32_t *s_wy, bool stage_x, bool stage_y, Sync wsync)
{
	const bool same = tw == fw && th == fh;
	const bool conv = a.filter != 0u && !same;

	// ---- 2. stored pixels -> one dword per pixel; the windows of both axes
	const uint32_t n = tw * th;
	for (uint32_t i = lane; i < n; i += G) {
		uint32_t px;
		if constexpr (C == 4) {
			px = reinterpret_cast<const uint32_t *>(src)[i];
			if (conv) px = premultiply(px);  // fir: U8x4 is alpha-premultiplied before a convolution
		} else {
			// one dword from the pixel's byte address (the slot's last pixel: from a byte earlier, shifted)
			typedef uint32_t u32_a1 __attribute__((aligned(1)));
			if (a.slot_bytes >= 4u) {
				const uint32_t at = 3u * i + 4u <= a.slot_bytes ? 3u * i : a.slot_bytes - 4u;
				px = (*reinterpret_cast<const u32_a1 *>(src + at) >> (8u * (3u * i - at))) | 0xff000000u;
			} else {  // (1x1 blocks)
				px = (uint32_t)src[3 * i] | ((uint32_t)src[3 * i + 1] << 8) | ((uint32_t)src[3 * i + 2] << 16) | 0xff000000u;
			}
		}
		s_src[i] = px;
	}
	ExpandTab tab_x{0, 0, 0, 0}, tab_y{0, 0, 0, 0};
	// per output sample wdw dwords: first | count << 16, then the weights as i16 pairs (a zero in the spare half)
	auto stage_windows = [&](uint32_t *wd, const ExpandTab &tab, uint32_t outs) {
		for (uint32_t o = lane; o < outs; o += G) {
			uint32_t *d = wd + a.wdw * o;
			const uint32_t first = a.starts[tab.start_off + o];
			const uint32_t cnt = a.filter == 0u ? 1u : a.sizes[tab.start_off + o];
			d[0] = first | (cnt << 16);
			if (a.filter != 0u) {
				const int16_t *k = a.coeffs + tab.coeff_off + o * tab.window;
				for (uint32_t j = 0; j < cnt; j += 2u)
					d[1u + (j >> 1)] = (uint32_t)(uint16_t)k[j] | (j + 1u < cnt ? (uint32_t)(uint16_t)k[j + 1u] << 16 : 0u);
			}
		}
	};
	if (tw != fw) {
		tab_x = a.dir[(size_t)a.slot[fw] * a.stride + tw];
		if (stage_x) stage_windows(s_wx, tab_x, fw);
	}
	if (th != fh) {
		tab_y = a.dir[(size_t)a.slot[fh] * a.stride + th];
		if (stage_y) stage_windows(s_wy, tab_y, fh);
	}
	wsync();

	// ---- 3. the resize into an image of fw x fh dwords
	const uint32_t *out = s_src;  // block.rs:279-281: clone
	if (same) {
	} else if (a.filter == 0u) {  // ResizeAlg::Nearest
		RowWalker rw(lane, G, fw);
		for (uint32_t i = lane; i < fw * fh; i += G, rw.next()) {
			const uint32_t x = tw == fw ? rw.col : (s_wx[a.wdw * rw.col] & 0xffffu), y = th == fh ? rw.row : (s_wy[a.wdw * rw.row] & 0xffffu);
			s_tmp[i] = s_src[y * tw + x];
		}
		out = s_tmp;
		wsync();
	} else {
		const bool need_h = tw != fw, need_v = th != fh;
		if (need_h) {
			// horizontal pass: item = (ox, y) of the th stored rows
			const int prec = tab_x.precision;
			const int32_t init = 1 << (prec - 1);
			RowWalker rw(lane, G, fw);
			for (uint32_t i = lane; i < fw * th; i += G, rw.next()) {
				const uint32_t *wd = s_wx + a.wdw * rw.col;
				const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
				const uint32_t *row = s_src + rw.row * tw + first;
				int32_t acc[4] = {init, init, init, init};
				// two taps per v_dot2_i32_i16 (an odd count has a zero weight for the pixel read past the window, which is
				// still inside the image: tw < fw)
				for (uint32_t j = 0; j < cnt; j += 2u) {
					const uint32_t w2 = wd[1u + (j >> 1)], p0 = row[j], p1 = row[j + 1u];
#pragma unroll
					for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
				}
				uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
				px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
				if (C == 4 && !need_v) px = unpremultiply(px);
				s_tmp[i] = px;
			}
			out = s_tmp;
			wsync();
		}
		if (need_v) {
			// vertical pass: item = (ox, oy); the rows it reads are fw wide (fw == tw when only this pass runs)
			const uint32_t *cur = need_h ? s_tmp : s_src;
			uint32_t *o = need_h ? s_src : s_tmp;
			const int prec = tab_y.precision;
			const int32_t init = 1 << (prec - 1);
			RowWalker rw(lane, G, fw);
			for (uint32_t i = lane; i < fw * fh; i += G, rw.next()) {
				const uint32_t *wd = s_wy + a.wdw * rw.row;
				const uint32_t hdr = wd[0], first = hdr & 0xffffu, cnt = hdr >> 16;
				const uint32_t *col = cur + first * fw + rw.col;
				int32_t acc[4] = {init, init, init, init};
				for (uint32_t j = 0; j < cnt; j += 2u) {
					const uint32_t w2 = wd[1u + (j >> 1)], p0 = col[j * fw], p1 = col[(j + 1u) * fw];
#pragma unroll
					for (uint32_t c = 0; c < (uint32_t)C; ++c) acc[c] = dot2(__builtin_amdgcn_perm(p1, p0, c | 0x0c000c00u | ((4u + c) << 16)), w2, acc[c]);
				}
				uint32_t px = clip8_med3(acc[0], prec) | (clip8_med3(acc[1], prec) << 8) | (clip8_med3(acc[2], prec) << 16);
				px |= C == 4 ? clip8_med3(acc[3], prec) << 24 : 0xff000000u;
				if constexpr (C == 4) px = unpremultiply(px);
				o[i] = px;
			}
			out = o;
			wsync();
		}
	}
	return out;
}

// ---------------------------------------------------------------------------
// Step 4 of varied_expand_kernel and window_expand_kernel: nh rows of nw pixels of a wave's image (one dword per pixel,
// row_dw dwords between rows, from `part`) to dst, pitch bytes between rows, C bytes per pixel.  Every row segment once:
// item = (row, group of four pixels) -- 16 bytes per lane with streaming stores where the segment starts on a dword (RGBA,
// dst and pitch multiples of 4), dwords at whatever address they have where it does not; RGB rows as 12-byte groups of four
// pixels, bytes at the tail.  No form writes a byte behind column nw of a row: a window's clipped edge lies in the middle of
// an output row, or beside another window's pixels.
// ---------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void store_tile_part(uint32_t lane, const uint32_t *part, uint32_t row_dw, uint32_t nw, uint32_t nh, uint8_t *dst,
                                                uint32_t pitch)
{
	const uint32_t q4 = (nw + 3u) >> 2;
	typedef uint32_t u32_a1 __attribute__((aligned(1)));
	if (C == 4 && ((reinterpret_cast<uintptr_t>(dst) | pitch) & 3u) == 0u) {
		typedef uint32_t u32q __attribute__((ext_vector_type(4), aligned(4)));
		RowWalker rw(lane, 64u, q4);
		for (uint32_t i = lane; i < q4 * nh; i += 64u, rw.next()) {
			const uint32_t x = 4u * rw.col;
			const uint32_t *p = part + rw.row * row_dw + x;
			uint8_t *d = dst + (size_t)rw.row * pitch + x * 4u;
			if (x + 4u <= nw) {
				const u32q v = {p[0], p[1], p[2], p[3]};
				__builtin_nontemporal_store(v, reinterpret_cast<u32q *>(d));
			} else {
				for (uint32_t k = 0; x + k < nw; ++k) __builtin_nontemporal_store(p[k], reinterpret_cast<uint32_t *>(d) + k);
			}
		}
	} else if (C == 4) {
		// an odd offset or pitch: dwords at whatever byte address they have
		RowWalker rw(lane, 64u, nw);
		for (uint32_t i = lane; i < nw * nh; i += 64u, rw.next())
			*reinterpret_cast<u32_a1 *>(dst + (size_t)rw.row * pitch + rw.col * 4u) = part[rw.row * row_dw + rw.col];
	} else {
		RowWalker rw(lane, 64u, q4);
		for (uint32_t i = lane; i < q4 * nh; i += 64u, rw.next()) {
			const uint32_t x = 4u * rw.col;
			const uint32_t *p = part + rw.row * row_dw + x;
			uint8_t *d = dst + (size_t)rw.row * pitch + x * 3u;
			if (x + 4u <= nw) {
				// four pixels as twelve bytes, three dwords at whatever byte address they have: the last byte written is the
				// fourth pixel's blue, so a group that ends at column nw ends there
				const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
				u32_a1 *o = reinterpret_cast<u32_a1 *>(d);
				o[0] = (p0 & 0xffffffu) | (p1 << 24);
				o[1] = ((p1 >> 8) & 0xffffu) | (p2 << 16);
				o[2] = ((p2 >> 16) & 0xffu) | (p3 << 8);
			} else {
				for (uint32_t k = 0; x + k < nw; ++k) {
					const uint32_t px = p[k];
					d[3u * k] = (uint8_t)px;
					d[3u * k + 1u] = (uint8_t)(px >> 8);
					d[3u * k + 2u] = (uint8_t)(px >> 16);
				}
			}
		}
	}
}

}  // namespace pxz
