// pxz_tables.cpp — host-side tables for the shrink kernels.
//
//  * down-scaling windows: what `PixlzrBlock::resize` (reference
//    src/data_types/block.rs:273-334) gets from fast_image_resize 4.2.1 for
//    ResizeAlg::Convolution(filter) / ResizeAlg::Nearest with default
//    ResizeOptions, per (source size, target size) along one axis.  The crate
//    is Pillow-lineage: f64 window weights normalised to 1, converted to i16
//    at the largest precision that keeps the biggest weight below 2^15.
//  * level thresholds: `value.log2().round().min(0).exp2()` (reference
//    src/operations.rs:147-148) only depends on n = round(log2f(v)); the
//    kernel compares v against the smallest float reaching each n, found here
//    with the platform's own log2f (the one Rust's f32::log2 calls).
//  * the device table sets built from those windows (layouts: pxz_internal.h):
//    the generic shrink tables with the matrix-core operands of 16/32/64-px
//    tiles, the expand directory and its operands, and tree::process's axis
//    tables.  Host vectors only: pxz_api.cpp uploads and caches them.
#include "pxz_tables.h"
#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <tuple>

namespace pxz {

namespace {

constexpr double kPi = 3.14159265358979323846;

struct Kernel1D {
	double support;
	double (*eval)(double);
};

double hamming(double x)
{
	x = std::fabs(x);
	if (x == 0.0) return 1.0;
	if (x >= 1.0) return 0.0;
	x *= kPi;
	return (0.54 + 0.46 * std::cos(x)) * std::sin(x) / x;
}

double catmull_rom(double x)
{
	constexpr double a = -0.5;
	x = std::fabs(x);
	if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
	if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
	return 0.0;
}

double gaussian(double x)
{
	if (x <= -3.0 || x >= 3.0) return 0.0;
	return std::exp(-(x * x) / 0.5) / std::sqrt(2.0 * kPi * 0.25);
}

double sinc(double x)
{
	if (x == 0.0) return 1.0;
	x *= kPi;
	return std::sin(x) / x;
}

double lanczos3(double x)
{
	return (x >= -3.0 && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0;
}

double bilinear(double x)
{
	x = std::fabs(x);
	return x < 1.0 ? 1.0 - x : 0.0;
}

// FilterType -> fir filter (reference src/data_types/mod.rs:65-107): the down-scale branch maps Triangle to
// Convolution(Hamming), the up-scale branch (SuperSampling(filter, 2): a plain convolution when nothing
// shrinks) maps it to Bilinear; the other three keep their kernel
bool kernel_for(uint32_t filter, bool upscale, Kernel1D *k)
{
	switch (filter) {
	case 1:
		if (upscale) *k = {1.0, bilinear};
		else *k = {1.0, hamming};
		return true;
	case 2: *k = {2.0, catmull_rom}; return true;  // CatmullRom
	case 3: *k = {3.0, gaussian}; return true;     // Gaussian
	case 4: *k = {3.0, lanczos3}; return true;     // Lanczos3
	default: return false;
	}
}

}  // namespace

bool build_axis(uint32_t in_size, uint32_t out_size, uint32_t filter, AxisWindows *out, bool upscale)
{
	out->in_size = in_size;
	out->out_size = out_size;
	out->starts.assign(out_size, 0);
	out->sizes.assign(out_size, 0);
	if (filter == 0) {  // ResizeAlg::Nearest: source index per output index
		out->window = 1;
		out->precision = 0;
		out->coeffs.clear();
		const double scale = static_cast<double>(in_size) / static_cast<double>(out_size);
		const double first = scale * 0.5;
		for (uint32_t o = 0; o < out_size; ++o) {
			uint32_t s = static_cast<uint32_t>(first + scale * static_cast<double>(o));
			out->starts[o] = static_cast<int32_t>(s < in_size ? s : in_size - 1);
			out->sizes[o] = 1;
		}
		return true;
	}
	Kernel1D k;
	if (!kernel_for(filter, upscale, &k)) return false;

	const double scale = static_cast<double>(in_size) / static_cast<double>(out_size);
	const double stretch = scale > 1.0 ? scale : 1.0;
	const double radius = k.support * stretch;
	const double inv_stretch = 1.0 / stretch;
	const int window = static_cast<int>(std::ceil(radius)) * 2 + 1;
	out->window = window;

	std::vector<double> weights(static_cast<size_t>(out_size) * window, 0.0);
	double biggest = 0.0;
	for (uint32_t o = 0; o < out_size; ++o) {
		const double centre = (static_cast<double>(o) + 0.5) * scale;
		const double lo = std::floor(centre - radius);
		const double hi = std::ceil(centre + radius);
		const int first = lo < 0.0 ? 0 : static_cast<int>(lo);
		const int last = hi > static_cast<double>(in_size) ? static_cast<int>(in_size) : static_cast<int>(hi);
		const int n = last - first;
		double *w = &weights[static_cast<size_t>(o) * window];
		const double shifted = centre - 0.5;
		double total = 0.0;
		for (int i = 0; i < n; ++i) {
			w[i] = k.eval((static_cast<double>(first + i) - shifted) * inv_stretch);
			total += w[i];
		}
		if (total != 0.0)
			for (int i = 0; i < n; ++i) w[i] /= total;
		for (int i = 0; i < n; ++i)
			if (w[i] > biggest) biggest = w[i];
		out->starts[o] = first;
		out->sizes[o] = n;
	}

	int precision = 0;
	for (int p = 0; p < 22; ++p) {
		precision = p;
		const int next = static_cast<int>(std::round(biggest * static_cast<double>(1 << (p + 1))));
		if (next >= (1 << 15)) break;
	}
	out->precision = precision;
	out->coeffs.assign(weights.size(), 0);
	const double unit = static_cast<double>(1 << precision);
	for (size_t i = 0; i < weights.size(); ++i) {
		double v = std::round(weights[i] * unit);
		if (v > 32767.0) v = 32767.0;
		if (v < -32768.0) v = -32768.0;
		out->coeffs[i] = static_cast<int16_t>(v);
	}
	return true;
}

static inline float from_bits(uint32_t b)
{
	float f;
	std::memcpy(&f, &b, 4);
	return f;
}
static inline uint32_t to_bits(float f)
{
	uint32_t b;
	std::memcpy(&b, &f, 4);
	return b;
}

bool build_level_thresholds(float *thresholds, int count)
{
	for (int k = 0; k < count; ++k) {
		auto reaches = [k](float v) { return std::roundf(::log2f(v)) >= static_cast<float>(-k); };
		uint32_t lo = to_bits(std::ldexp(1.0f, -k - 1));  // log2 = -k-1: does not reach
		uint32_t hi = to_bits(std::ldexp(1.0f, -k));      // log2 = -k: reaches
		if (reaches(from_bits(lo)) || !reaches(from_bits(hi))) return false;
		while (hi - lo > 1) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (reaches(from_bits(mid))) hi = mid; else lo = mid;
		}
		// the decision must be a clean step around the threshold
		for (uint32_t d = 1; d <= 4096; ++d) {
			if (!reaches(from_bits(hi + d - 1)) || reaches(from_bits(hi - d))) return false;
		}
		thresholds[k] = from_bits(hi);
	}
	return true;
}

namespace {

// reduced size for level exponent m (reference operations.rs:150-151)
uint32_t reduced(uint32_t size, uint32_t m)
{
	if (m >= 31) return 1;
	uint64_t r = ((uint64_t)size + ((1ull << m) - 1ull)) >> m;
	return r < 1 ? 1u : (uint32_t)r;
}

// clip8(2^(precision-1) + 255 * total) == 255: a constant-255 alpha comes back as 255 (above 255 is clamped to 255)
bool keeps_opaque(int32_t total, int precision)
{
	return (((1 << (precision - 1)) + 255 * total) >> precision) >= 255;
}

// The matrix-core operand tables (pxz_internal.h: kMfDwords, kMf16Dwords, the shrink64 tables, kXmfDw, kXmf16Dw, kXmf64Dw)
// share their arithmetic; each layout only says where the weights of one output go.  A weight K goes in as two signed
// bytes, K = 256 * hi + lo: lo at bit `shift` of dword dw, hi at the same place `hi_plane` dwords further on.
struct OperandPacker {
	std::vector<uint32_t> mf;  // one table, zeroed
	uint32_t hi_plane;
	int precision;
	int32_t k[64];             // the current output's weights over the whole source axis (at most 64 samples)
	int32_t total = 0;         //   and their sum
	bool fits = true;          // every high byte is a signed 8-bit value
	bool opaque_stays = true;  // keeps_opaque at every output so far

	OperandPacker(size_t dwords, uint32_t hi_plane_, int precision_) : mf(dwords, 0u), hi_plane(hi_plane_), precision(precision_) {}
	void window(const AxisWindows &win, uint32_t o)
	{
		std::fill(k, k + 64, 0);
		total = 0;
		for (uint32_t i = 0; i < (uint32_t)win.sizes[o]; ++i) {
			k[(uint32_t)win.starts[o] + i] = win.coeffs[(size_t)o * win.window + i];
			total += k[(uint32_t)win.starts[o] + i];
		}
		if (!keeps_opaque(total, precision)) opaque_stays = false;
	}
	// source sample i of the current window
	void put(uint32_t i, uint32_t dw, uint32_t shift)
	{
		const int32_t lo = ((k[i] + 128) & 255) - 128, hi = (k[i] - lo) / 256;
		if (hi < -128 || hi > 127) fits = false;
		mf[dw] |= (uint32_t)(uint8_t)lo << shift;
		mf[hi_plane + dw] |= (uint32_t)(uint8_t)hi << shift;
	}
	uint32_t bias() const { return (uint32_t)(128 * total + (1 << (precision - 1))); }
};

// appends v to the blob `to`, returns where it starts
uint32_t append(std::vector<uint32_t> &to, const std::vector<uint32_t> &v)
{
	to.insert(to.end(), v.begin(), v.end());
	return (uint32_t)(to.size() - v.size());
}

// The up-scales 1, 2, 4, .. -> side as matrix-core operands: one table of `dwords` per source size, filled by
// layout(pk, win); empty when a weight does not fit.
template <class Layout>
std::vector<uint32_t> expand_operands(uint32_t side, uint32_t filter, uint32_t levels, size_t dwords, uint32_t hi_plane, Layout layout)
{
	std::vector<uint32_t> xmf;
	for (uint32_t li = 0; li < levels; ++li) {
		AxisWindows win;
		if (!build_axis(1u << li, side, filter, &win, true)) return {};  // (not reached: the directory used the filter)
		OperandPacker pk(dwords, hi_plane, win.precision);
		layout(pk, win);
		if (!pk.fits) return {};
		append(xmf, pk.mf);
	}
	return xmf;
}

}  // namespace

bool build_shrink_tables(uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t filter, ShrinkTableSet *out)
{
	ShrinkTableSet &s = *out;
	s = ShrinkTableSet{};
	std::vector<AxisTab> &tabs = s.tabs;
	tabs.resize(2 * 2 * kMaxLevel);
	s.mf64.assign(4, 0u);  // offset 0 means "no table"
	bool mf64_complete = bw == 64 && bh == 64 && filter != 0;
	const uint32_t sizes[2][2] = {{bw, edge_w}, {bh, edge_h}};
	for (int axis = 0; axis < 2; ++axis) {
		for (int cls = 0; cls < 2; ++cls) {
			const uint32_t in = sizes[axis][cls];
			for (int m = 0; m < kMaxLevel; ++m) {
				AxisTab &t = tabs[(axis * 2 + cls) * kMaxLevel + m];
				const uint32_t outsz = reduced(in, (uint32_t)m);
				t = AxisTab{0, 0, 0, 0, 0, (uint16_t)outsz, 0, 0, (uint16_t)in, 0};
				if (outsz == in) continue;  // identity: never looked up
				// identical (in, out) pairs share one table: the edge class of a grid without ragged
				// edge, and every level past the first that reaches 1 px
				if (cls == 1 && sizes[axis][1] == sizes[axis][0]) {
					t = tabs[(axis * 2 + 0) * kMaxLevel + m];
					continue;
				}
				if (m > 0 && tabs[(axis * 2 + cls) * kMaxLevel + m - 1].out_size == outsz &&
				    tabs[(axis * 2 + cls) * kMaxLevel + m - 1].in_size == in && reduced(in, (uint32_t)m - 1) != in) {
					t = tabs[(axis * 2 + cls) * kMaxLevel + m - 1];
					continue;
				}
				AxisWindows win;
				if (!build_axis(in, outsz, filter, &win)) return false;
				t.bounds_off = (uint32_t)s.bounds.size();
				t.coeff_off = (uint32_t)s.coeffs.size();
				t.ksum_off = (uint32_t)s.ksums.size();
				t.precision = (uint16_t)win.precision;
				if (filter == 0) {
					for (uint32_t o = 0; o < outsz; ++o) s.bounds.push_back((uint16_t)win.starts[o]);
					continue;
				}
				// pad every window to whole quads of 4 source samples (8-byte aligned LDS reads)
				uint32_t wquads = 1;
				for (uint32_t o = 0; o < outsz; ++o) {
					const uint32_t lead = (uint32_t)win.starts[o] & 3u;
					const uint32_t nq = (lead + (uint32_t)win.sizes[o] + 3u) / 4u;
					if (nq > wquads) wquads = nq;
				}
				t.wquads = (uint16_t)wquads;
				t.rows_off = (uint32_t)s.rows.size();
				// rows of up to 8 quads are padded with zero weights to header + 16 dwords: the fast path fetches
				// whole rows with 16-byte loads and needs no per-quad guard
				t.row_stride = wquads <= 8u ? 20u : (4u + wquads * 2u + 3u) & ~3u;
				for (uint32_t o = 0; o < outsz; ++o) {
					const uint32_t first = (uint32_t)win.starts[o], n = (uint32_t)win.sizes[o];
					const uint32_t lead = first & 3u, nq = (lead + n + 3u) / 4u;
					s.bounds.push_back((uint16_t)(first / 4u));
					s.bounds.push_back((uint16_t)nq);
					std::vector<int16_t> k(wquads * 4u, 0);
					int32_t total = 0;
					for (uint32_t i = 0; i < n; ++i) {
						k[lead + i] = win.coeffs[(size_t)o * win.window + i];
						total += k[lead + i];
					}
					const size_t row0 = s.rows.size();
					s.rows.resize(row0 + t.row_stride, 0u);
					s.rows[row0 + 0] = first / 4u;
					s.rows[row0 + 1] = nq;
					s.rows[row0 + 2] = (uint32_t)total;
					for (uint32_t d = 0; d < wquads * 2u; ++d) {
						const uint32_t pr = (uint32_t)(uint16_t)k[2 * d] | ((uint32_t)(uint16_t)k[2 * d + 1] << 16);
						s.coeffs.push_back(pr);
						s.rows[row0 + 4 + d] = pr;
					}
					s.ksums.push_back(total);
					if (!keeps_opaque(total, win.precision)) s.opaque_stays = false;
				}
				// 32x32 tiles: operands for the matrix-core form of the two-pass resample (x axis table,
				// used for both axes of a full tile)
				if (axis == 0 && cls == 0 && bw == 32 && bh == 32 && outsz <= 16) {
					OperandPacker pk(kMfDwords, 128, win.precision);
					for (uint32_t o = 0; o < outsz; ++o) {
						pk.window(win, o);
						for (uint32_t g = 0; g < 4; ++g)
							for (uint32_t j = 0; j < 8; ++j)
								pk.put(j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4), 2 * (g * 16 + o) + j / 4, 8 * (j & 3));
						pk.mf[256 + o] = pk.bias();
						pk.mf[272 + o] = (uint32_t)pk.total;
					}
					pk.mf[288] = pk.opaque_stays ? 1u : 0u;
					if (pk.fits) t.mf_off = append(s.rows, pk.mf);
				}
				// 16x16 tiles: operands of the group-of-four matrix-core resample (resample_group16_mfma): 16 -> 8 | 4 | 2 | 1
				if (axis == 0 && cls == 0 && bw == 16 && bh == 16 && outsz <= 8) {
					OperandPacker pk(kMf16Dwords, 32, win.precision);
					for (uint32_t o = 0; o < outsz; ++o) {
						pk.window(win, o);
						for (uint32_t i = 0; i < 16; ++i) pk.put(i, o * 4 + i / 4, 8 * (i & 3));
						pk.mf[64 + o] = pk.bias();
						pk.mf[72 + o] = (uint32_t)pk.total;
					}
					pk.mf[80] = pk.opaque_stays ? 1u : 0u;
					pk.mf[81] = (uint32_t)win.precision;
					// (the group form writes alpha 255: only where the windows keep it)
					if (pk.fits && pk.opaque_stays) t.mf_off = append(s.rows, pk.mf);
				}
				// 64x64 tiles: operands of shrink64_kernel (Fast64Args), every level from 32 px down to 1 px
				if (axis == 0 && cls == 0 && bw == 64 && bh == 64 && outsz < 64) {
					const uint32_t nblk = outsz > 16 ? outsz / 16 : 1;
					OperandPacker pk((size_t)nblk * 512 + 72, 256, win.precision);
					for (uint32_t o = 0; o < outsz; ++o) {
						pk.window(win, o);
						const uint32_t blk = o / 16, ol = o % 16;
						for (uint32_t g = 0; g < 4; ++g)
							for (uint32_t j = 0; j < 16; ++j) pk.put(16 * g + j, blk * 512 + (g * 16 + ol) * 4 + j / 4, 8 * (j & 3));
						pk.mf[nblk * 512 + o] = pk.bias();
						pk.mf[nblk * 512 + 32 + o] = (uint32_t)pk.total;
					}
					pk.mf[nblk * 512 + 64] = pk.opaque_stays ? 1u : 0u;
					if (pk.fits && outsz <= 32) t.mf_off = append(s.mf64, pk.mf);
					else mf64_complete = false;
				}
			}
		}
	}
	if (s.bounds.empty()) s.bounds.push_back(0);
	if (s.coeffs.empty()) s.coeffs.push_back(0);
	if (s.ksums.empty()) s.ksums.push_back(0);
	s.rows.resize(s.rows.size() + 32, 0u);  // the fast path always fetches 4+16 dwords per row
	if (!mf64_complete) s.mf64.clear();
	return true;
}

// One up-scaling table, `in` stored samples -> `outsz` (PixlzrBlock::resize with the upscale flag set, block.rs:301-304),
// appended to the arrays of an expand table set: the per-axis code of build_expand_tables and build_varied_expand_tables.
static bool append_expand_axis(uint32_t in, uint32_t outsz, uint32_t filter, ExpandTab *t, std::vector<uint16_t> *starts,
                               std::vector<uint16_t> *sizes, std::vector<int16_t> *coeffs)
{
	AxisWindows win;
	if (!build_axis(in, outsz, filter, &win, true)) return false;
	t->start_off = (uint32_t)starts->size();
	t->coeff_off = (uint32_t)coeffs->size();
	t->window = (uint16_t)win.window;
	t->precision = (uint16_t)win.precision;
	for (uint32_t o = 0; o < outsz; ++o) {
		starts->push_back((uint16_t)win.starts[o]);
		sizes->push_back((uint16_t)win.sizes[o]);
	}
	coeffs->insert(coeffs->end(), win.coeffs.begin(), win.coeffs.end());
	return true;
}

// For each axis and size class (full / ragged edge) one up-scaling table per source size 1 .. full-1.
bool build_expand_tables(uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t filter, ExpandTableSet *out)
{
	ExpandTableSet &s = *out;
	s = ExpandTableSet{};
	const uint32_t stride = (bw > bh ? bw : bh) + 1u;
	s.dir_stride = stride;
	s.dir.assign(4u * stride, ExpandTab{0, 0, 0, 0});
	const uint32_t full[2][2] = {{bw, edge_w}, {bh, edge_h}};
	for (uint32_t axis = 0; axis < 2; ++axis) {
		for (uint32_t cls = 0; cls < 2; ++cls) {
			const uint32_t outsz = full[axis][cls];
			if (cls == 1 && outsz == full[axis][0]) {
				for (uint32_t in = 0; in < stride; ++in) s.dir[(axis * 2 + 1) * stride + in] = s.dir[(axis * 2 + 0) * stride + in];
				continue;
			}
			for (uint32_t in = 1; in < outsz; ++in)
				if (!append_expand_axis(in, outsz, filter, &s.dir[(axis * 2 + cls) * stride + in], &s.starts, &s.sizes, &s.coeffs)) return false;
		}
	}
	if (s.starts.empty()) {
		s.starts.push_back(0);
		s.sizes.push_back(0);
	}
	if (s.coeffs.empty()) s.coeffs.push_back(0);
	if (filter == 0) return true;
	// 32x32 tiles: the up-scales 1, 2, 4, 8, 16 -> 32 (layouts: pxz_internal.h)
	if (bw == 32 && bh == 32)
		s.xmf = expand_operands(32, filter, kXmfLevels, kXmfDw, 128, [](OperandPacker &pk, const AxisWindows &win) {
			bool copies = win.in_size == 1 && win.precision < 15;
			for (uint32_t o = 0; o < 32; ++o) {
				pk.window(win, o);
				if (win.sizes[o] != 1 || pk.k[0] != (1 << win.precision)) copies = false;
				for (uint32_t kg = 0; kg < 2; ++kg)
					for (uint32_t j = 0; j < 8; ++j) pk.put(xmf_src(kg, j), 2 * (kg * 32 + o) + j / 4, 8 * (j & 3));
				pk.mf[256 + o] = pk.bias();
			}
			for (uint32_t g = 0; g < 2; ++g)
				for (uint32_t reg = 0; reg < 16; ++reg) pk.mf[288 + 16 * g + reg] = pk.mf[256 + xmf_row(g, reg)];
			pk.mf[320] = (uint32_t)win.precision;
			pk.mf[321] = copies ? 1u : 0u;
		});
	// 16x16 tiles: the up-scales 1, 2, 4, 8 -> 16 for expand16_kernel
	if (bw == 16 && bh == 16)
		s.xmf16 = expand_operands(16, filter, kXmf16Levels, kXmf16Dw, 32, [](OperandPacker &pk, const AxisWindows &win) {
			for (uint32_t o = 0; o < 16; ++o) {
				pk.window(win, o);
				for (uint32_t i = 0; i < 8; ++i) pk.put(i, o * 2 + i / 4, 8 * (i & 3));
				pk.mf[64 + o] = pk.bias();
			}
			for (uint32_t g = 0; g < 2; ++g)
				for (uint32_t r = 0; r < 8; ++r) pk.mf[80 + 8 * g + r] = pk.mf[64 + (r & 3) + 8 * (r >> 2) + 4 * g];
			pk.mf[96] = (uint32_t)win.precision;
		});
	// 64x64 tiles: the up-scales 1 .. 32 -> 64 for expand64_kernel
	if (bw == 64 && bh == 64)
		s.xmf64 = expand_operands(64, filter, kXmf64Levels, kXmf64Dw, 128, [](OperandPacker &pk, const AxisWindows &win) {
			for (uint32_t o = 0; o < 64; ++o) {
				pk.window(win, o);
				const uint32_t q = o >> 5, ol = o & 31u;
				for (uint32_t st = 0; st < 2; ++st)
					for (uint32_t kg = 0; kg < 2; ++kg)
						for (uint32_t j = 0; j < 8; ++j)
							pk.put(16 * st + xmf_src(kg, j), ((q * 2 + st) * 2) * 128 + 2 * (kg * 32 + ol) + j / 4, 8 * (j & 3));
				pk.mf[1024 + o] = pk.bias();
			}
			for (uint32_t q = 0; q < 2; ++q)
				for (uint32_t g = 0; g < 2; ++g)
					for (uint32_t reg = 0; reg < 16; ++reg) pk.mf[1088 + (q * 2 + g) * 16 + reg] = pk.mf[1024 + 32 * q + xmf_row(g, reg)];
			pk.mf[1152] = (uint32_t)win.precision;
		});
	return true;
}

bool build_tree_tables(uint32_t width, uint32_t height, const std::vector<std::pair<uint32_t, uint32_t>> &levels, uint32_t filter,
                       uint32_t filter_upscale, TreeTableSet *out)
{
	// ---- every tile size of every level, per axis (split.rs:18-19 applied level after level to the sizes of the level before)
	auto split = [](uint32_t s, uint32_t b, std::set<uint32_t> &out) {
		const uint32_t c = (s + b - 1) / b;
		if (c > 1) out.insert(b);
		out.insert(s - (c - 1) * b);
	};
	std::set<uint32_t> all[2], cur[2];
	split(width, levels[0].first, cur[0]);
	split(height, levels[0].second, cur[1]);
	for (size_t l = 0;; ++l) {
		for (int ax = 0; ax < 2; ++ax) all[ax].insert(cur[ax].begin(), cur[ax].end());
		if (l + 1 >= levels.size()) break;
		std::set<uint32_t> next[2];
		for (uint32_t v : cur[0]) split(v, levels[l + 1].first, next[0]);
		for (uint32_t v : cur[1]) split(v, levels[l + 1].second, next[1]);
		cur[0].swap(next[0]);
		cur[1].swap(next[1]);
	}
	TreeTableSet &s = *out;
	s = TreeTableSet{};
	std::set<std::tuple<uint32_t, uint32_t, uint32_t>> pairs;  // (in, out, up)
	for (int ax = 0; ax < 2; ++ax)
		for (uint32_t sz : all[ax])
			for (uint32_t m = 1; m <= 32; ++m) {
				const uint32_t o = reduced(sz, m);
				if (o == sz) continue;
				pairs.insert(std::make_tuple(sz, o, 0u));
				pairs.insert(std::make_tuple(o, sz, 1u));
			}
	for (const auto &pr : pairs) {
		const uint32_t in = std::get<0>(pr), out = std::get<1>(pr), up = std::get<2>(pr);
		AxisWindows win;
		if (!build_axis(in, out, up ? filter_upscale : filter, &win, up != 0)) return false;
		TreeAxisEntry e{};
		e.in = (uint16_t)in;
		e.out = (uint16_t)out;
		e.up = (uint16_t)up;
		e.window = (uint16_t)win.window;
		e.precision = (uint32_t)win.precision;
		e.starts_off = (uint32_t)s.starts.size();
		e.coeff_off = (uint32_t)s.coeffs.size();
		for (uint32_t o = 0; o < out; ++o) {
			s.starts.push_back(win.starts[o]);
			s.sizes.push_back(win.sizes.empty() ? 0 : win.sizes[o]);
		}
		s.coeffs.insert(s.coeffs.end(), win.coeffs.begin(), win.coeffs.end());
		s.dir.push_back(e);
	}
	if (s.dir.empty()) s.dir.push_back(TreeAxisEntry{});
	if (s.starts.empty()) { s.starts.push_back(0); s.sizes.push_back(0); }
	if (s.coeffs.empty()) s.coeffs.push_back(0);
	return true;
}

bool build_varied_tables(const std::vector<uint32_t> &sizes, uint32_t filter, VariedTableSet *out)
{
	VariedTableSet &s = *out;
	s = VariedTableSet{};
	const std::set<uint32_t> ins(sizes.begin(), sizes.end());
	const uint32_t top = ins.empty() ? 0u : *ins.rbegin();
	s.dir.assign((size_t)(top + 1u) * kMaxLevel, TreeAxisEntry{});
	std::map<std::pair<uint32_t, uint32_t>, TreeAxisEntry> made;
	for (uint32_t in : ins) {
		if (in == 0u) continue;
		for (uint32_t m = 1; m < (uint32_t)kMaxLevel; ++m) {
			const uint32_t o = reduced(in, m);
			if (o == in) continue;
			auto it = made.find({in, o});
			if (it == made.end()) {
				AxisWindows win;
				if (!build_axis(in, o, filter, &win, false)) return false;
				TreeAxisEntry e{};
				e.in = (uint16_t)in;
				e.out = (uint16_t)o;
				e.window = (uint16_t)win.window;
				e.precision = (uint32_t)win.precision;
				e.starts_off = (uint32_t)s.starts.size();
				e.coeff_off = (uint32_t)s.coeffs.size();
				for (uint32_t k = 0; k < o; ++k) {
					s.starts.push_back(win.starts[k]);
					s.sizes.push_back(win.sizes.empty() ? 0 : win.sizes[k]);
				}
				s.coeffs.insert(s.coeffs.end(), win.coeffs.begin(), win.coeffs.end());
				it = made.emplace(std::make_pair(in, o), e).first;
			}
			s.dir[(size_t)in * kMaxLevel + m] = it->second;
		}
	}
	if (s.dir.empty()) s.dir.push_back(TreeAxisEntry{});
	if (s.starts.empty()) { s.starts.push_back(0); s.sizes.push_back(0); }
	if (s.coeffs.empty()) s.coeffs.push_back(0);
	return true;
}

bool build_varied_expand_tables(const std::vector<uint32_t> &sizes, uint32_t filter, VariedExpandTableSet *out)
{
	VariedExpandTableSet &s = *out;
	s = VariedExpandTableSet{};
	const std::set<uint32_t> fulls(sizes.begin(), sizes.end());
	const uint32_t top = fulls.empty() ? 0u : *fulls.rbegin();
	s.stride = top + 1u;
	s.slot.assign(top + 1u, 0xffffffffu);
	uint32_t n = 0;
	for (uint32_t full : fulls)
		if (full != 0u) s.slot[full] = n++;
	s.dir.assign((size_t)(n ? n : 1u) * s.stride, ExpandTab{0, 0, 0, 0});
	for (uint32_t full : fulls) {
		if (full == 0u) continue;
		for (uint32_t in = 1; in < full; ++in) {
			ExpandTab &t = s.dir[(size_t)s.slot[full] * s.stride + in];
			if (!append_expand_axis(in, full, filter, &t, &s.starts, &s.sizes, &s.coeffs)) return false;
			if (t.window > s.max_window) s.max_window = t.window;
		}
	}
	if (s.starts.empty()) {
		s.starts.push_back(0);
		s.sizes.push_back(0);
	}
	if (s.coeffs.empty()) s.coeffs.push_back(0);
	return true;
}

uint32_t filter_support(uint32_t filter)
{
	Kernel1D k;
	return filter != 0u && kernel_for(filter, false, &k) ? (uint32_t)k.support : 0u;
}

bool build_scaled_expand_tables(const std::vector<uint32_t> &targets, const std::vector<uint32_t> &max_stored, uint32_t filter,
                                ScaledExpandTableSet *out)
{
	ScaledExpandTableSet &s = *out;
	s = ScaledExpandTableSet{};
	if (targets.size() != max_stored.size() || filter > 4u) return false;
	std::map<uint32_t, uint32_t> most;  // target -> its largest stored size
	uint32_t top = 0, top_stored = 0;
	for (size_t i = 0; i < targets.size(); ++i) {
		if (targets[i] == 0u) continue;
		uint32_t &m = most[targets[i]];
		if (max_stored[i] > m) m = max_stored[i];
		if (targets[i] > top) top = targets[i];
		if (max_stored[i] > top_stored) top_stored = max_stored[i];
	}
	s.stride = top_stored + 1u;
	s.slot.assign(top + 1u, 0xffffffffu);
	uint32_t n = 0;
	for (const auto &tm : most) s.slot[tm.first] = n++;
	s.dir.assign((size_t)(n ? n : 1u) * s.stride, ScaledTab{0, 0, 0, 0, 0, 0});
	s.mixed = s.dir;
	auto append = [&](uint32_t in, uint32_t outsz, bool upscale, ScaledTab *t) {
		AxisWindows win;
		if (!build_axis(in, outsz, filter, &win, upscale)) return false;
		t->start_off = (uint32_t)s.starts.size();
		t->coeff_off = (uint32_t)s.coeffs.size();
		t->window = (uint16_t)win.window;
		t->precision = (uint16_t)win.precision;
		uint32_t taps = 0;
		for (uint32_t o = 0; o < outsz; ++o) {
			s.starts.push_back((uint16_t)win.starts[o]);
			s.sizes.push_back((uint16_t)win.sizes[o]);
			if ((uint32_t)win.sizes[o] > taps) taps = (uint32_t)win.sizes[o];
		}
		s.coeffs.insert(s.coeffs.end(), win.coeffs.begin(), win.coeffs.end());
		t->taps = (uint16_t)taps;
		t->wdw = (uint16_t)(filter == 0u ? 1u : 1u + (taps + 1u) / 2u);
		if (taps > s.max_taps) s.max_taps = taps;
		if (outsz * t->wdw > s.max_win_dw) s.max_win_dw = outsz * t->wdw;
		return true;
	};
	for (const auto &tm : most) {
		const uint32_t target = tm.first;
		for (uint32_t in = 1; in <= tm.second; ++in) {
			if (in == target) continue;
			const size_t at = (size_t)s.slot[target] * s.stride + in;
			if (!append(in, target, target > in, &s.dir[at])) return false;
			s.mixed[at] = s.dir[at];
			// (only Triangle's kernel depends on the flag: mod.rs:65-107)
			if (in > target && filter == 1u && !append(in, target, true, &s.mixed[at])) return false;
		}
	}
	if (s.starts.empty()) {
		s.starts.push_back(0);
		s.sizes.push_back(0);
	}
	if (s.coeffs.empty()) s.coeffs.push_back(0);
	return true;
}

const Knobs &knobs()
{
	static const Knobs k = [] {
		auto on = [](const char *name) { return getenv(name) != nullptr; };
		Knobs v;
		v.no_alpha_kernel = on("PXZ_NO_ALPHA_KERNEL");
		v.no_oklab_general = on("PXZ_NO_OKLAB_GENERAL");
		v.no_oklab32 = on("PXZ_NO_OKLAB32");
		v.no_oklab_edges = on("PXZ_NO_OKLAB_EDGES");
		v.no_repitch = on("PXZ_NO_REPITCH");
		v.no_widen = on("PXZ_NO_WIDEN");
		v.no_native_rgb = on("PXZ_NO_NATIVE_RGB");
		v.no_narrow = on("PXZ_NO_NARROW");
		v.no_group16 = on("PXZ_NO_GROUP16");
		v.no_clone_ahead = on("PXZ_NO_CLONE_AHEAD");
		v.no_big_tiles = on("PXZ_NO_BIG_TILES");
		v.no_alpha_first = on("PXZ_NO_ALPHA_FIRST");
		v.oklab_v1 = on("PXZ_OKLAB_V1");
		v.tree_rects = on("PXZ_TREE_RECTS");
		v.no_expand_fast32 = on("PXZ_NO_EXPAND_FAST32");
		const char *e = getenv("PXZ_WPB");
		v.wpb = e ? atoi(e) : 0;
		e = getenv("PXZ_CHUNK_LG");
		v.chunk_lg = e ? (atoi(e) & 15) : -1;
		e = getenv("PXZ_CUS");
		v.cus = e ? atoi(e) : 0;
		return v;
	}();
	return k;
}

}  // namespace pxz
