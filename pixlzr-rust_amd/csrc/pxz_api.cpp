// pxz_api.cpp — host runtime behind the C ABI of include/pixlzr_hip.h:
// handle, per-configuration table cache, HBM staging for the host-buffer entry
// point, kernel launches on the caller's stream, HIP-event timing.
//
// Who owns what: pxz_handle.h has the owners -- DeviceBuffer (a grow-only device allocation: a scratch buffer, or the one
// allocation behind a table set) and PinnedStaging (a pinned block and the event behind the last copy out of it); each
// frees what it holds.  HandleScratch (pxz_runtime.h) is everything pxz_trim gives back, pxz_handle adds what survives a
// trim; the table caches go through cached_tables.  The kernel units' launchers are declared in pxz_launch.h.
// The entry points that take host pointers and compose the device entry points of this file (the host forms) are in
// pxz_host_forms.cpp.  pxz_runtime.h declares what they share with this file; the functions it names are defined here in
// namespace pxz_runtime, everything else of this file stays in the anonymous namespace.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <system_error>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/pixlzr_hip.h"
#include "pxz_fit.h"
#include "pxz_handle.h"
#include "pxz_internal.h"
#include "pxz_launch.h"
#include "pxz_runtime.h"
#include "pxz_shrink_plan.h"
#include "pxz_tables.h"
#include "pxz_tilefit.h"

using namespace pxz_runtime;
using pxz::kLdsPerCu;

constexpr uint32_t kMaxImageSide = 1u << 24;  // see pxz_grid
// a tile image of at most this many bytes is staged whole in LDS by varied_kernel (with its second image and, for shrink_by,
// the detector's tables: 142 KB of the 160 KB)
constexpr uint64_t kVariedMaxTileBytes = 65536;

namespace pxz_runtime {  // (varied_plan, window_plan and stage_host_image stand further down, beside what they use)

int fail(pxz_handle *h, int code, const char *fmt, ...)
{
	if (h) {
		char buf[512];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		h->error = buf;
	}
	return code;
}

int ensure(pxz_handle *h, DeviceBuffer &b, size_t bytes)
{
	return b.reserve(bytes) ? PXZ_OK : fail(h, PXZ_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
}

// the decode side uses neither mode nor factor (and the reader no filter): the caller's parameters with those neutral
pxz_params decode_side_params(const pxz_params *params, bool with_filter)
{
	pxz_params p = *params;
	p.mode = 0;
	p.factor = 0.0f;
	if (!with_filter) p.filter = 0;
	return p;
}

int check_params(pxz_handle *h, const pxz_params *p)
{
	if (p->block_w == 0 || p->block_h == 0) return fail(h, PXZ_ERR_INVALID_ARG, "zero block size");
	if (p->mode > 1) return fail(h, PXZ_ERR_INVALID_ARG, "mode must be 0 or 1");
	if (p->filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "filter must be 0..4");
	if (!std::isfinite(p->factor)) return fail(h, PXZ_ERR_INVALID_ARG, "factor must be finite");
	return PXZ_OK;
}

int varied_check_params(pxz_handle *h, uint32_t channels, const pxz_params *p)
{
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	const int rc = check_params(h, p);
	if (rc != PXZ_OK) return rc;
	if ((uint64_t)p->block_w * p->block_h * channels > kVariedMaxTileBytes)
		return fail(h, PXZ_ERR_UNSUPPORTED, "varied batches stage every tile in LDS: block_w*block_h*channels must not exceed %llu bytes",
		            (unsigned long long)kVariedMaxTileBytes);
	return PXZ_OK;
}

// the ladder's rules for a host array of factors
int check_factors(pxz_handle *h, const float *factors, uint32_t n_factors, uint32_t max_rungs)
{
	if (!factors) return fail(h, PXZ_ERR_INVALID_ARG, "null factors");
	if (n_factors == 0 || n_factors > max_rungs) return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", max_rungs, n_factors);
	for (uint32_t r = 0; r < n_factors; ++r)
		if (!std::isfinite(factors[r])) return fail(h, PXZ_ERR_INVALID_ARG, "factor %u must be finite", r);
	return PXZ_OK;
}

// what pxz_fit_select and pxz_fit_varied_ladder_device check of their sizes (h may be null: the host form has no handle)
int fit_check(pxz_handle *h, uint32_t n_images, uint32_t n_factors, uint32_t channels, uint32_t criterion)
{
	if (n_images == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	if (n_factors == 0 || n_factors > PXZ_VARIED_LADDER_MAX_RUNGS)
		return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", PXZ_VARIED_LADDER_MAX_RUNGS, n_factors);
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	if (criterion != PXZ_FIT_BYTES && criterion != PXZ_FIT_SSE)
		return fail(h, PXZ_ERR_INVALID_ARG, "criterion must be PXZ_FIT_BYTES (0) or PXZ_FIT_SSE (1), got %u", criterion);
	return PXZ_OK;
}

// the groups of the per-tile fit: runs of consecutive images, given by their first images (null: every image its own group)
int tile_groups_check(pxz_handle *h, const uint32_t *group_first, uint32_t n_groups, uint32_t n_images)
{
	if (!group_first) {
		if (n_groups != n_images)
			return fail(h, PXZ_ERR_INVALID_ARG, "group_first is null (every image its own group): n_groups must be n_images = %u, got %u", n_images,
			            n_groups);
		return PXZ_OK;
	}
	if (n_groups == 0 || n_groups > n_images) return fail(h, PXZ_ERR_INVALID_ARG, "n_groups must be 1..n_images = %u, got %u", n_images, n_groups);
	if (group_first[0] != 0 || group_first[n_groups] != n_images)
		return fail(h, PXZ_ERR_INVALID_ARG, "group_first must run from 0 to n_images = %u", n_images);
	for (uint32_t g = 0; g < n_groups; ++g)
		if (group_first[g + 1u] <= group_first[g] || group_first[g + 1u] > n_images)
			return fail(h, PXZ_ERR_INVALID_ARG, "group %u: group_first must ascend (a group has an image)", g);
	return PXZ_OK;
}

// The header fields of one .pixlzr file; on PXZ_ERR_INVALID_ARG *why says what is wrong with it.
int file_header(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint32_t *block_w, uint32_t *block_h,
                uint32_t *channels, uint32_t *filter_byte, const char **why)
{
	*why = "null pointer";
	if (!file || !width || !height || !block_w || !block_h || !channels || !filter_byte) return PXZ_ERR_INVALID_ARG;
	static const uint8_t magic[9] = {'P', 'I', 'X', 'L', 'Z', 'R', 0, 0, 2};
	*why = "not a .pixlzr v0.0.2 file";
	if (len < 26 || std::memcmp(file, magic, 9) != 0) return PXZ_ERR_INVALID_ARG;
	auto be = [&](size_t o) { return ((uint32_t)file[o] << 24) | ((uint32_t)file[o + 1] << 16) | ((uint32_t)file[o + 2] << 8) | file[o + 3]; };
	*filter_byte = file[9];
	*width = be(10);
	*height = be(14);
	*block_w = be(18);
	*block_h = be(22);
	*why = "empty image or block in the header";
	if (*width == 0 || *height == 0 || *block_w == 0 || *block_h == 0) return PXZ_ERR_INVALID_ARG;
	uint32_t cols, rows;
	pxz_grid(*width, *height, *block_w, *block_h, &cols, &rows);
	const size_t first = 26 + (size_t)rows * 4;
	*why = "file ends inside the first record";
	if (len < first + 13 + 10) return PXZ_ERR_INVALID_ARG;
	*channels = file[first + 21];  // the first record's QOI header (decode_block, mod.rs:202-242)
	*why = "first record has neither 3 nor 4 channels";
	if (*channels != 3 && *channels != 4) return PXZ_ERR_INVALID_ARG;
	*why = "";
	return PXZ_OK;
}

// the tiles of a planned batch
uint32_t varied_n_tiles(const std::vector<pxz::VariedImage> &images)
{
	return images.back().tile0 + images.back().cols * images.back().rows;
}

// the covered tiles of a planned call
uint32_t window_n_tiles(const std::vector<pxz::WindowEntry> &entries) { return entries.back().tile0 + entries.back().ccols * entries.back().crows; }

// LDS bytes of a one-wave block of reshrink_distortion_kernel: the wave's image of the launch's own layout function beside the
// images' first tiles at their largest (kVxImages dwords, pxz_device.h) -- what the entry point and the size query hold against
// kLdsPerCu, so that a block the query admits is launched whatever n_images is
uint64_t reshrink_distortion_bytes(uint32_t bw, uint32_t bh, uint32_t wdw)
{
	const uint32_t dw = pxz::reshrink_distortion_tile_dw(bw, bh, wdw);
	return dw == 0xffffffffu ? 0xffffffffull : (uint64_t)dw * 4u + 8192u;
}

// The LDS footprint of one block of each archive kernel, as its launch asks for it: one callable per kernel, (dwords of a staged
// window of the expand side's tables, the same of the sets' tables -- the distortions alone have a second set) -> bytes.  What
// says whether a kernel takes its blocks is its footprint against the CU's: each size query (archive_lds_query) and each
// admission check (beyond_lds under the call's own text) holds one of these against kLdsPerCu, first with windows of 1 dword,
// then with the real ones.  rung_channels: 0 for the one-factor kernel, the tiles' channel count for the ladder kernel, whose
// footprint depends on it (its resampled images).
static auto reshrink_footprint(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t rung_channels)
{
	return [=](uint32_t wdw, uint32_t) -> uint64_t { return pxz::reshrink_lds_bytes(mode, bw, bh, rung_channels, wdw); };
}
static auto retile_footprint(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t rung_channels)
{
	return [=](uint32_t wdw, uint32_t) -> uint64_t {
		return rung_channels == 0u ? pxz::retile_lds_bytes(mode, sbw, sbh, dbw, dbh, wdw)
		                           : pxz::retile_ladder_lds_bytes(mode, sbw, sbh, dbw, dbh, rung_channels, wdw);
	};
}
static auto reshrink_distortion_footprint(uint32_t bw, uint32_t bh)  // (one stride for the windows of both sets: the wider)
{
	return [=](uint32_t wdw_ref, uint32_t wdw_set) -> uint64_t { return reshrink_distortion_bytes(bw, bh, std::max(wdw_ref, wdw_set)); };
}
static auto retile_distortion_footprint(uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh)
{
	return [=](uint32_t wdw_src, uint32_t wdw_set) -> uint64_t { return pxz::retile_distortion_lds_bytes(sbw, sbh, dbw, dbh, wdw_src, wdw_set); };
}
template <class Footprint>
static bool beyond_lds(const Footprint &bytes, uint32_t wdw, uint32_t wdw_set = 1u)
{
	return bytes(wdw, wdw_set) > kLdsPerCu;
}

// whether the re-shrink kernels (and the patch, which is reshrink_kernel's block) take a block
int reshrink_check_block(pxz_handle *h, uint32_t mode, uint32_t bw, uint32_t bh, uint32_t rung_channels, uint32_t wdw)
{
	if (beyond_lds(reshrink_footprint(mode, bw, bh, rung_channels), wdw))
		return fail(h, PXZ_ERR_UNSUPPORTED,
		            "a re-shrink%s keeps two planes of block_w*block_h dwords and the windows of both axes in LDS: block_w*block_h*4 must not exceed 65536 "
		            "bytes, the whole 160 KB (%ux%u)", rung_channels ? " ladder" : "", bw, bh);
	return PXZ_OK;
}

}  // namespace pxz_runtime

namespace {

// ensure() for the buffer that holds a stream kernel's binning counters: a new allocation forgets that they were left
// zeroed (nothing in it is zero)
int ensure_bins(pxz_handle *h, DeviceBuffer &b, size_t bytes, const uint32_t *&bins_clean)
{
	const size_t cap = b.cap;
	const int rc = ensure(h, b, bytes);
	if (b.cap != cap) bins_clean = nullptr;
	return rc;
}

// A launch of a stream kernel leaves its binning counters zeroed for the next one on the same buffer: launch(true) when
// they are at `bins` already.  After a launch that failed nothing is known about them.
template <class Launch>
int launch_on_bins(pxz_handle *h, const uint32_t *&bins_clean, const uint32_t *bins, Launch launch)
{
	const bool clean = bins_clean == bins;
	bins_clean = nullptr;
	PXZ_HIP(h, launch(clean));
	bins_clean = bins;
	return PXZ_OK;
}

// magic number for unsigned division by d >= 1 (exact for every 32-bit dividend)
pxz::FastDiv make_fastdiv(uint32_t d)
{
	uint32_t l = 0;
	while ((1ull << l) < d) ++l;  // ceil(log2 d)
	const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
	return pxz::FastDiv{(uint32_t)m, l < 1 ? l : 1u, l < 1 ? 0u : l - 1};
}

// The tile grid of a batch of equally sized frames (pxz_shrink_plan.h has the arithmetic).
using Grid = pxz::TileGrid;
constexpr uint64_t kAnyTiles = ~0ull;  // make_grid without a limit

// Fills *g with pxz_grid's grid (the caller has checked the sides); PXZ_ERR_UNSUPPORTED when the batch has more than
// `limit` tiles.
int make_grid(pxz_handle *h, uint32_t width, uint32_t height, uint32_t bw, uint32_t bh, uint32_t n_frames, uint64_t limit, Grid *g)
{
	*g = pxz::tile_grid(width, height, bw, bh, n_frames);
	return g->tiles > limit ? fail(h, PXZ_ERR_UNSUPPORTED, "too many tiles") : PXZ_OK;
}

// a checked grid -> the geometry fields every kernel's arguments name alike
template <class Args>
void put_grid(const Grid &g, Args *a)
{
	a->cols = g.cols;
	a->rows = g.rows;
	a->tiles_per_frame = g.tiles_per_frame;
	a->n_tiles = (uint32_t)g.tiles;
	a->edge_w = g.edge_w;
	a->edge_h = g.edge_h;
}

// val, ow and oh for `tiles` tiles, and out for their slots of slot_bytes each (0: no pixels)
int ensure_tile_outputs(pxz_handle *h, size_t tiles, size_t slot_bytes)
{
	int rc = ensure(h, h->val, tiles * 4);
	if (rc == PXZ_OK) rc = ensure(h, h->ow, tiles * 4);
	if (rc == PXZ_OK) rc = ensure(h, h->oh, tiles * 4);
	if (rc == PXZ_OK && slot_bytes != 0) rc = ensure(h, h->out, tiles * slot_bytes);
	return rc;
}

// ... and their way back to the host, queued on the handle's stream (the pixels only when the caller wants them)
int download_tile_outputs(pxz_handle *h, size_t tiles, size_t slot_bytes, float *block_value, uint32_t *tile_w, uint32_t *tile_h,
                          uint8_t *pixels)
{
	PXZ_HIP(h, hipMemcpyAsync(block_value, h->val.ptr, tiles * 4, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(tile_w, h->ow.ptr, tiles * 4, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(tile_h, h->oh.ptr, tiles * 4, hipMemcpyDeviceToHost, h->stream));
	if (pixels) PXZ_HIP(h, hipMemcpyAsync(pixels, h->out.ptr, tiles * slot_bytes, hipMemcpyDeviceToHost, h->stream));
	return PXZ_OK;
}

// The pitch of the device copy of a host image: rows of a 16-byte multiple when the caller's do not have one (tight rows
// of an RGBA image whose width is not a multiple of 4); the copy engine does the re-pitching for free.
uint32_t device_pitch_of(uint32_t width, uint32_t channels, uint32_t pitch_bytes)
{
	if (channels == 4 && (pitch_bytes & 15u) != 0) return (uint32_t)(((size_t)width * channels + 15u) & ~(size_t)15u);
	return pitch_bytes;
}

// One array of a table set on its way to the device: its device address goes to *dst (null when the array is empty).
struct TablePart {
	template <class T>
	TablePart(const std::vector<T> &v, T **d) : src(v.data()), bytes(v.size() * sizeof(T)), dst(reinterpret_cast<void **>(d)) {}
	const void *src;
	size_t bytes;
	void **dst;
};

// Uploads one table set into the single allocation *mem, every array at a 256-byte aligned offset.  On failure nothing
// is left allocated.
int upload_tables(pxz_handle *h, std::initializer_list<TablePart> parts, DeviceBuffer *mem)
{
	size_t total = 0;
	for (const TablePart &p : parts) total += up256(p.bytes);
	mem->release();
	hipError_t e = mem->reserve(total) ? hipSuccess : hipErrorOutOfMemory;
	uint8_t *at = static_cast<uint8_t *>(mem->ptr);
	for (auto p = parts.begin(); e == hipSuccess && p != parts.end(); at += up256(p->bytes), ++p) {
		*p->dst = p->bytes ? at : nullptr;
		if (p->bytes) e = hipMemcpy(at, p->src, p->bytes, hipMemcpyHostToDevice);
	}
	if (e == hipSuccess) return PXZ_OK;
	mem->release();
	return fail(h, PXZ_ERR_HIP, "uploading %zu bytes of tables: %s", total, hipGetErrorString(e));
}

// One cache of table sets: the set under `key`, built and uploaded by build(set) when it is not there yet.  A cache
// with a bound is emptied when it is full -- after the stream has drained: a queued launch may still read a table.
// The sets are map nodes: a pointer handed out stays valid across later insertions.
template <class Cache, class Build>
int cached_tables(pxz_handle *h, Cache &cache, const typename Cache::key_type &key, size_t bound, Build build,
                  const typename Cache::mapped_type **out)
{
	auto it = cache.find(key);
	if (it == cache.end()) {
		if (bound != 0 && cache.size() >= bound) {
			PXZ_HIP(h, hipStreamSynchronize(h->stream));
			cache.clear();
		}
		typename Cache::mapped_type set;
		const int rc = build(set);
		if (rc != PXZ_OK) return rc;
		it = cache.emplace(key, std::move(set)).first;
	}
	*out = &it->second;
	return PXZ_OK;
}

int get_tables(pxz_handle *h, uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t filter,
               const TableSet **out)
{
	return cached_tables(h, h->tables, std::make_tuple(bw, bh, edge_w, edge_h, filter), 0, [&](TableSet &ts) {
		pxz::ShrinkTableSet s;
		if (!pxz::build_shrink_tables(bw, bh, edge_w, edge_h, filter, &s)) return fail(h, PXZ_ERR_INVALID_ARG, "unknown filter %u", filter);
		ts.tabs = s.tabs;
		ts.rows_dw = (uint32_t)s.rows.size();
		ts.opaque_stays = s.opaque_stays;
		return upload_tables(h, {{s.bounds, &ts.d_bounds}, {s.coeffs, &ts.d_coeffs}, {s.ksums, &ts.d_ksums}, {s.rows, &ts.d_rows},
		                         {s.mf64, &ts.d_mf64}}, &ts.mem);
	}, out);
}

int get_expand_tables(pxz_handle *h, uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t filter,
                      const ExpandTables **out)
{
	return cached_tables(h, h->expand_tables, std::make_tuple(bw, bh, edge_w, edge_h, filter), 0, [&](ExpandTables &et) {
		pxz::ExpandTableSet s;
		if (!pxz::build_expand_tables(bw, bh, edge_w, edge_h, filter, &s)) return fail(h, PXZ_ERR_INVALID_ARG, "unknown filter %u", filter);
		et.dir_stride = s.dir_stride;
		return upload_tables(h, {{s.dir, &et.d_dir}, {s.starts, &et.d_starts}, {s.sizes, &et.d_sizes}, {s.coeffs, &et.d_coeffs},
		                         {s.xmf, &et.d_xmf}, {s.xmf16, &et.d_xmf16}, {s.xmf64, &et.d_xmf64}}, &et.mem);
	}, out);
}

// ---- level decision tables ---------------------------------------------------
// reference src/operations.rs:128-138
float parse_value_host(float value)
{
	uint32_t bits;
	std::memcpy(&bits, &value, 4);
	if ((bits >> 31) == 0) return value;
	float t = 1.0f + value;
	return (t != t) ? 0.0f : (t > 0.0f ? t : 0.0f);
}

// level exponent of one tile of (w,h) whose directional gradient sum is `sum`
// (operations.rs:253-258 -> pixlzr.rs:199 -> operations.rs:145-148)
uint32_t level_of_sum(const pxz_handle *h, uint64_t sum, uint32_t w, uint32_t hh, float factor)
{
	const uint64_t fac = (uint64_t)(w - 2) * (uint64_t)(hh - 2) * 4096ull;
	const float raw = (float)((double)sum / (double)fac);
	const float v = parse_value_host(raw * factor);
	uint32_t m = 0;
	for (int j = 0; j < kMaxLevel; ++j) m += (v < h->thresholds[j]) ? 1u : 0u;
	return m;
}

// Fills a->breaks / a->breaks_asc of a kernel's arguments that name the block and the edges (ShrinkArgs, LadderArgs).  Oklab mode: the key is the bit pattern of the (non-negative)
// parsed value, compared against the float thresholds' bit patterns.  Directional mode: the key is
// the integer gradient sum; the float pipeline sum -> value -> level is monotone in the sum, so each
// threshold becomes one integer breakpoint per tile class, found by bisection with the exact formula.
template <class Args>
void build_breaks(pxz_handle *h, uint32_t mode, float factor, Args *a)
{
	uint32_t fbits;
	std::memcpy(&fbits, &factor, 4);
	const auto key = std::make_tuple(mode, fbits, a->bw, a->bh, a->edge_w, a->edge_h);
	auto it = h->breaks.find(key);
	if (it != h->breaks.end()) {
		std::memcpy(a->breaks, it->second.b, sizeof a->breaks);
		std::memcpy(a->breaks_asc, it->second.asc, sizeof a->breaks_asc);
		return;
	}
	struct Saver {
		pxz_handle *h; Args *a; decltype(key) k;
		~Saver() {
			pxz_handle::Breaks br;
			std::memcpy(br.b, a->breaks, sizeof br.b);
			std::memcpy(br.asc, a->breaks_asc, sizeof br.asc);
			h->breaks[k] = br;
		}
	} saver{h, a, key};
	for (int cls = 0; cls < 4; ++cls) {
		a->breaks_asc[cls] = 0;
		for (int j = 0; j < kMaxLevel; ++j) std::memcpy(&a->breaks[cls][j], &h->thresholds[j], 4);
	}
	if (mode != PXZ_MODE_SHRINK_DIRECTIONALLY) return;
	for (int cls = 0; cls < 4; ++cls) {
		const uint32_t w = (cls & 1) ? a->edge_w : a->bw, hh = (cls & 2) ? a->edge_h : a->bh;
		if (w <= 2 || hh <= 2) {  // 0/0 tiles are special-cased in the kernel
			for (int j = 0; j < kMaxLevel; ++j) a->breaks[cls][j] = 0xffffffffu;
			continue;
		}
		const uint64_t max_sum = (uint64_t)(w - 2) * (hh - 2) * 3u * 1020u;
		const uint32_t m_lo = level_of_sum(h, 0, w, hh, factor), m_hi = level_of_sum(h, max_sum, w, hh, factor);
		const bool asc = m_hi > m_lo;  // level exponent grows with the sum (negative factors)
		a->breaks_asc[cls] = asc ? 1u : 0u;
		for (int j = 0; j < kMaxLevel; ++j) {
			// predicate "v < T[j]"  <=>  level exponent > j
			auto below = [&](uint64_t s) { return level_of_sum(h, s, w, hh, factor) > (uint32_t)j; };
			const bool at0 = below(0), atmax = below(max_sum);
			uint32_t brk;
			if (at0 == atmax) {
				// constant: encode always-true / never for the class' comparison direction
				const bool always = at0;
				brk = asc ? (always ? 0u : 0xffffffffu) : (always ? 0xffffffffu : 0u);
			} else {
				uint64_t lo = 0, hi = max_sum;  // below(lo) == at0, below(hi) == atmax
				while (hi - lo > 1) {
					const uint64_t mid = lo + (hi - lo) / 2;
					if (below(mid) == at0) lo = mid; else hi = mid;
				}
				brk = (uint32_t)hi;  // first sum on the far side
			}
			a->breaks[cls][j] = brk;
		}
	}
}

int check_frames(pxz_handle *h, const pxz_frames *f, const pxz_params *p)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!f || !p) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	if (f->width == 0 || f->height == 0 || f->n_frames == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty frame batch");
	if (f->width > kMaxImageSide || f->height > kMaxImageSide)
		return fail(h, PXZ_ERR_UNSUPPORTED, "image sides above 2^24 are not supported (the reference's f32 and f64 tile grids part there)");
	if (f->channels != 3 && f->channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", f->channels);
	if ((uint64_t)f->pitch_bytes < (uint64_t)f->width * f->channels) return fail(h, PXZ_ERR_INVALID_ARG, "pitch smaller than a row");
	if (f->n_frames > 1 && f->frame_stride_bytes < (uint64_t)f->pitch_bytes * f->height)
		return fail(h, PXZ_ERR_INVALID_ARG, "frame stride smaller than a frame");
	return check_params(h, p);
}

// an LDS layout -> the carve-up fields ShrinkArgs and LadderArgs name alike
template <class Args>
void put_layout(const pxz::ShrinkLayout &l, Args *a)
{
	a->rs = l.rs;
	a->plane_dw = l.plane_dw;
	a->hps = l.hps;
	a->tmp_dw = l.tmp_dw;
	a->tile_dw = l.tile_dw;
}

// a table set -> the fields both name alike
template <class Args>
void put_tables(const TableSet &ts, Args *a)
{
	static_assert(sizeof a->tabs == sizeof(AxisTab) * 4 * kMaxLevel, "tables");
	std::memcpy(a->tabs, ts.tabs.data(), sizeof a->tabs);
	a->bounds = ts.d_bounds;
	a->coeffs = ts.d_coeffs;
	a->ksums = ts.d_ksums;
}

// The kernel arguments of a planned single-geometry call, filled once: everything but the handle's scratch pointers and the
// caller's outputs.  ts: the table set when pixels are wanted, else null.
void fill_shrink_args(pxz_handle *h, const pxz::ShrinkRoute &r, const pxz_params *p, const TableSet *ts, pxz::ShrinkArgs *a)
{
	const Grid &g = r.grid;
	a->frame_stride = r.frame_stride;
	a->pitch = r.frames.pitch_bytes;
	a->width = r.frames.width;
	a->height = r.frames.height;
	a->bw = p->block_w;
	a->bh = p->block_h;
	put_grid(g, a);
	a->div_tpf = make_fastdiv(g.tiles_per_frame);
	a->div_cols = make_fastdiv(g.cols);
	{
		// shrink16_kernel walks 2x2 groups of tiles
		const uint32_t gcols = (g.cols + 1u) / 2u, grows = (g.rows + 1u) / 2u;
		a->div_gpf = make_fastdiv(gcols * grows);
		a->div_gcols = make_fastdiv(gcols);
		a->n_frames_x_groups = gcols * grows * r.frames.n_frames;
	}
	a->mode = p->mode;
	a->filter = p->filter;
	a->finish_scan = 1;
	a->slot_bytes = p->block_w * p->block_h * r.channels;
	build_breaks(h, p->mode, p->factor, a);
	a->factor = r.factor;
	a->scale2 = r.scale2;
	if (ts) {
		put_tables(*ts, a);
		a->trows = ts->d_rows;
		a->tab_dw = ts->rows_dw * 4u <= 48u * 1024u ? (ts->rows_dw + 3u) & ~3u : 0u;
		a->mf64 = ts->d_mf64;
	}
	put_layout(r.layout, a);
	a->lab_dw = r.layout.lab_dw;
	a->big_blocks = r.big_blocks;
	a->oklab_given = r.detector != pxz::ShrinkDetector::None ? 1u : 0u;
	a->ok_bands = r.ok_bands;
	a->ok_count = (uint32_t)g.tiles;  // (region 0: every tile is enumerated)
	a->ok_rows = r.ok_rows;
	a->clone_ahead = r.clone_ahead;
	a->full_cols = r.full_cols;
	a->full_rows = r.full_rows;
	a->alpha_kernel = r.alpha_kernel;
	a->alpha_first = r.alpha_first;
	a->stats_sig = r.stats_sig;
	a->expect_listed = r.expect_listed;
}

// The launches of a planned call, timed together: detector, its edge regions, the fused kernel (+ the finishing kernel where no
// fast kernel finishes its own tiles).  a: filled, with its source, scratch and outputs set.
int launch_route(pxz_handle *h, const pxz::ShrinkRoute &r, pxz::ShrinkArgs &a)
{
	const pxz::FinishArgs fin{a.sums, a.value, a.lod0, a.lod1, a.n_tiles, a.tiles_per_frame, a.cols, a.rows,
	                          a.bw, a.bh, a.edge_w, a.edge_h, a.mode, a.factor};
	hipEvent_t e0 = nullptr, e1 = nullptr, emid = nullptr;
	const bool record = !h->quiet_stats && h->timing && (h->timing_count++ % h->timing_stride) == 0;
	if (record) {
		if (h->events_used == h->events.size()) {
			PXZ_HIP(h, hipEventCreate(&e0));
			PXZ_HIP(h, hipEventCreate(&e1));
			PXZ_HIP(h, hipEventCreate(&emid));
			h->events.emplace_back(e0, e1);
			h->mid_events.push_back(emid);
		}
		e0 = h->events[h->events_used].first;
		e1 = h->events[h->events_used].second;
		emid = h->mid_events[h->events_used];
		++h->events_used;
		PXZ_HIP(h, hipEventRecord(e0, h->stream));
		a.mid_event = emid;  // recorded behind the first kernel of the step (pxz_last_first_kernel_ms)
	}
	// shrink_by: the block-cooperative Oklab detector first, then the fused kernel only stages + resamples (it still runs the
	// generic detector on the tiles the route left it).  The square detectors copy every tile into its slot while they have its
	// pixels (clone_ahead): the shrink kernel then skips the tiles that are stored at full size instead of reading them again
	if (r.detector != pxz::ShrinkDetector::None) {
		PXZ_HIP(h, pxz::launch_oklab(a, h->n_cus, h->stream, r.detector == pxz::ShrinkDetector::Rgba ? 4 : 3));
		if (a.mid_event) {
			PXZ_HIP(h, hipEventRecord(static_cast<hipEvent_t>(a.mid_event), h->stream));
			a.mid_event = nullptr;
		}
		for (const pxz::ShrinkRegion &reg : r.regions) {
			if (!reg.wanted) continue;
			pxz::ShrinkArgs e = a;
			e.ok_region = reg.id;
			e.ok_bands = reg.bands;
			e.ok_count = reg.count;
			PXZ_HIP(h, pxz::launch_oklab(e, h->n_cus, h->stream));
			a.ok_edges |= reg.bit;
		}
	}
	// 32x32 RGBA flow: shrink32_kernel, then the worklist kernel, which also finishes every tile and zeroes the worklist counter
	// of the next launch (two counters, used alternately).  Which kernel takes the batch depends on the table set (tab_dw, mf64)
	// beside the route: the launchers' own predicates say
	const bool fast = pxz::fast32_applicable(a, r.channels) || pxz::fast64_applicable(a, r.channels) || pxz::fast16_applicable(a, r.channels);
	if (fast) {
		if (!h->work_ready) {
			PXZ_HIP(h, hipMemsetAsync(h->work.ptr, 0, pxz::kWorkList * 4u, h->stream));
			h->work_slot = 0;
		}
		h->work_ready = false;  // stays false if a launch below fails: the counters are then re-zeroed next time
		a.work_slot = h->work_slot;
	}
	PXZ_HIP(h, pxz::launch_shrink(a, r.channels, h->n_cus, h->stream));
	if (!fast && a.mid_event) PXZ_HIP(h, hipEventRecord(static_cast<hipEvent_t>(a.mid_event), h->stream));  // the generic kernel is the step
	if (fast) {
		h->work_slot ^= 1u;
		h->work_ready = true;
	} else {
		PXZ_HIP(h, pxz::launch_finish(fin, h->stream));
	}
	if (record) PXZ_HIP(h, hipEventRecord(e1, h->stream));
	return PXZ_OK;
}

}  // namespace

namespace {
// Upload of a host image for the host-buffer entry points, re-pitched where device_pitch_of says so.
int upload_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t pitch_bytes,
                 uint32_t *device_pitch)
{
	const size_t row_bytes = (size_t)width * channels;
	const uint32_t dp = device_pitch_of(width, channels, pitch_bytes);
	const size_t bytes = (size_t)dp * (height - 1) + row_bytes;
	int rc = ensure(h, h->in, bytes);
	if (rc != PXZ_OK) return rc;
	if (dp == pitch_bytes) PXZ_HIP(h, hipMemcpyAsync(h->in.ptr, pixels, bytes, hipMemcpyHostToDevice, h->stream));
	else PXZ_HIP(h, hipMemcpy2DAsync(h->in.ptr, dp, pixels, pitch_bytes, row_bytes, height, hipMemcpyHostToDevice, h->stream));
	*device_pitch = dp;
	return PXZ_OK;
}

// The pixels are here on the host: a sparse look at the alpha channel (one pixel in 61 per sampled row, every 7th
// row) decides whether the kernels for transparent tiles are worth their launch (> 2 % of the samples).
bool host_image_has_transparency(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t pitch_bytes)
{
	uint32_t seen = 0, looked = 0;
	for (uint32_t y = 0; y < height; y += 7)
		for (uint32_t x = (y * 13u) % 61u; x < width; x += 61, ++looked)
			seen += pixels[(size_t)y * pitch_bytes + (size_t)x * 4u + 3u] != 255u;
	return looked && seen * 50u > looked;
}
}  // namespace

extern "C" {

const char *pxz_version(void) { return "pixlzr-hip 0.1.0 (gfx950)"; }

int pxz_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int pxz_create(int device_id, pxz_handle **out)
{
	if (!out) return PXZ_ERR_INVALID_ARG;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return PXZ_ERR_NO_DEVICE;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return PXZ_ERR_NO_DEVICE;
	if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PXZ_ERR_NO_DEVICE;  // kernels are gfx950 only
	if (hipSetDevice(device_id) != hipSuccess) return PXZ_ERR_HIP;
	pxz_handle *h = new (std::nothrow) pxz_handle();
	if (!h) return PXZ_ERR_NOMEM;
	h->device = device_id;
	h->n_cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
	if (const int v = pxz::knobs().cus; v >= 1 && (uint32_t)v < h->n_cus) h->n_cus = (uint32_t)v;  // test knob: every launcher sizes its grid by this
	if (!pxz::build_level_thresholds(h->thresholds, pxz::kNumThresholds)) {
		delete h;
		return PXZ_ERR_UNSUPPORTED;  // platform log2f is not a clean step around 2^(k+1/2)
	}
	void *hs = nullptr, *ds = nullptr;
	if (hipHostMalloc(&hs, 64, hipHostMallocMapped) == hipSuccess) {
		std::memset(hs, 0, 64);
		static_cast<uint32_t *>(hs)[1] = 0xffffffffu;  // listed tiles of the last launch: unknown
		if (hipHostGetDevicePointer(&ds, hs, 0) == hipSuccess) {
			h->host_stats = static_cast<uint32_t *>(hs);
			h->dev_stats = static_cast<uint32_t *>(ds);
		} else {
			(void)hipHostFree(hs);
		}
	}
	(void)hipGetLastError();  // no pinned dword: no adaptive kernel choice, nothing else changes
	*out = h;
	return PXZ_OK;
}

void pxz_destroy(pxz_handle *h)
{
	if (!h) return;
	(void)hipSetDevice(h->device);
	for (auto &ev : h->events) {
		(void)hipEventDestroy(ev.first);
		(void)hipEventDestroy(ev.second);
	}
	for (hipEvent_t ev : h->mid_events) (void)hipEventDestroy(ev);
	if (h->host_stats) {
		(void)hipDeviceSynchronize();  // a queued launch may still write it
		(void)hipHostFree(h->host_stats);
	}
	delete h;  // (every buffer, table set and staging block frees itself)
}

const char *pxz_last_error(const pxz_handle *h) { return h ? h->error.c_str() : "null handle"; }

int pxz_trim(pxz_handle *h)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	PXZ_HIP(h, hipSetDevice(h->device));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	// the scratch and ring buffers, the bounded table caches and both pinned stagings go; packed_len, work_ready (the
	// worklist counters went with their buffer), qbins_clean and dbins_clean start over
	static_cast<HandleScratch &>(*h) = HandleScratch();
	return PXZ_OK;
}

int pxz_set_stream(pxz_handle *h, void *hip_stream)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	hipStream_t next = static_cast<hipStream_t>(hip_stream);
	if (next != h->stream) {
		// the handle's scratch buffers (and the worklist counters a launch leaves for the next one) are
		// ordered by the stream: finish what is queued on the old one before moving on
		PXZ_HIP(h, hipSetDevice(h->device));
		PXZ_HIP(h, hipStreamSynchronize(h->stream));
		h->stream = next;
	}
	return PXZ_OK;
}

int pxz_synchronize(pxz_handle *h)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	return PXZ_OK;
}

int pxz_grid(uint32_t width, uint32_t height, uint32_t block_w, uint32_t block_h, uint32_t *cols, uint32_t *rows)
{
	if (!cols || !rows || block_w == 0 || block_h == 0) return PXZ_ERR_INVALID_ARG;
	// The reference rounds up in f64 when it splits an image (iter.rs:38-41, split.rs:45-46) and in f32 when it writes
	// and expands one (pixlzr.rs:36-46).  Up to 2^24 both are the integer ceiling; beyond, the f32 form can differ from
	// it (and the reference's own two grids from each other), so larger images are refused here and by every entry
	// point -- ONE grid, this one, is used throughout the library.
	if (width > kMaxImageSide || height > kMaxImageSide) return PXZ_ERR_UNSUPPORTED;
	const pxz::TileGrid g = pxz::tile_grid(width, height, block_w, block_h, 1);
	*cols = g.cols;
	*rows = g.rows;
	return PXZ_OK;
}

// One shrink / detector pass over a batch.  identity: the closures of process() instead of shrink_by's.
// The route -- input form, LDS layout, detector, fast region, transparency, scratch -- is planned once (pxz_shrink_plan.h);
// this body validates, plans and executes it.  RGB batches whose tile size has an RGBA fast path are widened to RGBA (alpha
// 255) in scratch memory, run there, and their tile slots narrowed back (see rgb_to_rgba_kernel for why the results are the same).
static int run_shrink(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, const uint8_t *d_pixels,
                      float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, float *d_lod0,
                      float *d_lod1, bool identity)
{
	PXZ_HIP(h, hipSetDevice(h->device));
	int rc = check_frames(h, frames, params);
	if (rc != PXZ_OK) return rc;
	const pxz::Knobs &knobs = pxz::knobs();
	pxz::ShrinkRequest q{};
	q.frames = frames;
	q.params = params;
	q.want_pixels = d_out_pixels != nullptr;
	q.identity = identity;
	q.src_low_bits = (uint32_t)(reinterpret_cast<uintptr_t>(d_pixels) & 15u);
	q.n_cus = h->n_cus;
	if (volatile const uint32_t *hs = h->host_stats) {
		q.have_stats = true;
		for (int i = 0; i < 3; ++i) q.stats[i] = hs[i];
	}
	q.quiet_stats = h->quiet_stats;
	const TableSet *ts = nullptr;
	const Grid g = pxz::tile_grid(frames->width, frames->height, params->block_w, params->block_h, frames->n_frames);
	if (pxz::shrink_plan_needs_opaque_stays(q, knobs)) {
		if ((rc = get_tables(h, params->block_w, params->block_h, g.edge_w, g.edge_h, params->filter, &ts)) != PXZ_OK) return rc;
		q.opaque_stays = ts->opaque_stays;
	}
	pxz::ShrinkRoute r;
	char why[256];
	if ((rc = pxz::shrink_plan(q, knobs, &r, why, sizeof why)) != PXZ_OK) return fail(h, rc, "%s", why);
	if (q.want_pixels && !ts && (rc = get_tables(h, params->block_w, params->block_h, g.edge_w, g.edge_h, params->filter, &ts)) != PXZ_OK) return rc;

	// ---- buffers ----
	const void *work_before = h->work.ptr;
	if ((rc = ensure(h, h->sums, r.sums_bytes)) != PXZ_OK || (rc = ensure(h, h->work, r.work_total_bytes)) != PXZ_OK) return rc;
	if (h->work.ptr != work_before) h->work_ready = false;
	if (r.bigscratch_bytes != 0 && (rc = ensure(h, h->bigscratch, r.bigscratch_bytes)) != PXZ_OK) return rc;
	if (r.okscratch_bytes != 0 && (rc = ensure(h, h->okscratch, r.okscratch_bytes)) != PXZ_OK) return rc;
	if (r.rgba_bytes != 0 && (rc = ensure(h, h->rgba, r.rgba_bytes)) != PXZ_OK) return rc;
	if (r.slots4_bytes != 0 && (rc = ensure(h, h->slots4, r.slots4_bytes)) != PXZ_OK) return rc;

	// ---- input form ----
	const uint64_t src_stride = pxz::frame_stride_of(*frames);
	if (r.input == pxz::ShrinkInput::Widened) {
		const pxz::WidenArgs w{d_pixels, (uint8_t *)h->rgba.ptr, src_stride, r.frames.frame_stride_bytes, frames->pitch_bytes, r.frames.pitch_bytes,
		                       frames->width, frames->height, frames->n_frames};
		PXZ_HIP(h, pxz::launch_widen(w, h->stream));
	} else if (r.input == pxz::ShrinkInput::Repitched) {
		for (uint32_t n = 0; n < frames->n_frames; ++n)
			PXZ_HIP(h, hipMemcpy2DAsync((uint8_t *)h->rgba.ptr + (size_t)n * r.frames.frame_stride_bytes, r.frames.pitch_bytes,
			                            d_pixels + (size_t)n * src_stride, frames->pitch_bytes, (size_t)frames->width * 4u, frames->height,
			                            hipMemcpyDeviceToDevice, h->stream));
	}
	const bool narrow = r.slots4_bytes != 0;

	// ---- arguments ----
	pxz::ShrinkArgs a{};
	fill_shrink_args(h, r, params, ts, &a);
	a.src = r.input == pxz::ShrinkInput::AsGiven ? d_pixels : (const uint8_t *)h->rgba.ptr;
	a.out_w = d_out_w;
	a.out_h = d_out_h;
	a.out_px = narrow ? (uint8_t *)h->slots4.ptr : d_out_pixels;
	a.value = d_block_value;
	a.lod0 = d_lod0;
	a.lod1 = d_lod1;
	a.sums = (uint32_t *)h->sums.ptr;
	a.work = (uint32_t *)h->work.ptr;
	a.ahead_spare = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(h->work.ptr) + ((r.work_bytes + 7u) & ~(size_t)7u));
	a.clone_list = a.ahead_spare + 512u;
	if (r.big_blocks != 0u) a.big_scratch = (uint32_t *)h->bigscratch.ptr;
	if (r.okscratch_bytes != 0) a.ok_scratch = (float *)h->okscratch.ptr;
	a.stats = r.write_stats ? h->dev_stats : nullptr;
	if (r.write_stats) {
		h->last_alpha_kernel = r.alpha_kernel;
		h->last_alpha_first = r.alpha_first;
	}

	// ---- launches ----
	if ((rc = launch_route(h, r, a)) != PXZ_OK) return rc;
	if (narrow) {
		const pxz::NarrowArgs n{(const uint8_t *)h->slots4.ptr, d_out_pixels, d_out_w, d_out_h, a.n_tiles, a.bw * a.bh * 4u, a.bw * a.bh * 3u};
		PXZ_HIP(h, pxz::launch_narrow(n, h->stream));
	}
	return PXZ_OK;
}

int pxz_shrink_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                             const uint8_t *d_pixels, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                             uint8_t *d_out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!d_pixels || !d_block_value || !d_out_w || !d_out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	return run_shrink(h, frames, params, d_pixels, d_block_value, d_out_w, d_out_h, d_out_pixels, nullptr, nullptr, false);
}

int pxz_lod_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                          const uint8_t *d_pixels, float *d_lod0, float *d_lod1)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!d_pixels || !d_lod0 || !d_lod1) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	return run_shrink(h, frames, params, d_pixels, nullptr, nullptr, nullptr, nullptr, d_lod0, d_lod1, false);
}

// Factor ladder.  shrink_by over tiles whose LDS image fits (the generic kernel's layout with its detector planes, so
// that the single-factor call is sure to run too): the detector once in its identity form, then ladder_kernel
// (pxz_ladder.hip).  Everything else -- shrink_directionally, tiles beyond LDS -- is one single-factor call per rung.
int pxz_shrink_ladder_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, const float *factors,
                                    uint32_t n_factors, const uint8_t *d_pixels, float *d_block_value, uint32_t *d_out_w,
                                    uint32_t *d_out_h, uint8_t *d_out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!factors) return fail(h, PXZ_ERR_INVALID_ARG, "null factors");
	if (n_factors == 0 || n_factors > PXZ_LADDER_MAX_RUNGS)
		return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", PXZ_LADDER_MAX_RUNGS, n_factors);
	for (uint32_t r = 0; r < n_factors; ++r)
		if (!std::isfinite(factors[r])) return fail(h, PXZ_ERR_INVALID_ARG, "factor %u must be finite", r);
	if (!d_pixels || !d_block_value || !d_out_w || !d_out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (!frames || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz_params p = *params;
	p.factor = 1.0f;  // (a rung's factor enters nothing but its level)
	int rc = check_frames(h, frames, &p);
	if (rc != PXZ_OK) return rc;
	const bool want = d_out_pixels != nullptr;
	const Grid g = pxz::tile_grid(frames->width, frames->height, p.block_w, p.block_h, frames->n_frames);
	pxz::ShrinkLayout bare{};  // ladder_kernel's LDS image
	if (!pxz::shrink_ladder_in_lds(p, want, g.tiles, h->n_cus, pxz::knobs(), &bare)) {
		// one single-factor flow per rung: no amortisation, the same results and errors by construction
		const size_t tiles = (size_t)g.tiles;  // (the calls below check)
		const size_t slot = (size_t)p.block_w * p.block_h * frames->channels;
		for (uint32_t r = 0; r < n_factors; ++r) {
			pxz_params pr = *params;
			pr.factor = factors[r];
			if ((rc = pxz_shrink_frames_device(h, frames, &pr, d_pixels, d_block_value + r * tiles, d_out_w + r * tiles, d_out_h + r * tiles,
			                                   want ? d_out_pixels + r * tiles * slot : nullptr)) != PXZ_OK)
				return rc;
		}
		return PXZ_OK;
	}
	const TableSet *ts = nullptr;
	if (want && (rc = get_tables(h, p.block_w, p.block_h, g.edge_w, g.edge_h, p.filter, &ts)) != PXZ_OK) return rc;
	const size_t x_bytes = up256((size_t)g.tiles * 4u);
	if ((rc = ensure(h, h->ladder, x_bytes + PXZ_LADDER_MAX_RUNGS * 4u)) != PXZ_OK) return rc;
	float *d_x = (float *)h->ladder.ptr;
	float *d_factors = (float *)((uint8_t *)h->ladder.ptr + x_bytes);
	// the factors go through pinned staging, reused once the copy queued by the previous ladder call has run
	PXZ_HIP(h, h->ladder_factors.send(factors, n_factors * 4u, d_factors, h->stream, PXZ_LADDER_MAX_RUNGS * 4u));
	// stage 1: get_block_variance with the identity closure (factor 1, scale 1) -> x of every tile, no pixels
	h->quiet_stats = true;
	rc = run_shrink(h, frames, &p, d_pixels, nullptr, nullptr, nullptr, nullptr, d_x, nullptr, true);
	h->quiet_stats = false;
	if (rc != PXZ_OK) return rc;
	// stage 2: every rung of every tile, from the caller's frames as they are (any alignment, 3 or 4 channels)
	pxz::LadderArgs l{};
	l.src = d_pixels;
	l.frame_stride = pxz::frame_stride_of(*frames);
	l.pitch = frames->pitch_bytes;
	l.bw = p.block_w;
	l.bh = p.block_h;
	put_grid(g, &l);
	l.div_tpf = make_fastdiv(g.tiles_per_frame);
	l.div_cols = make_fastdiv(g.cols);
	l.filter = p.filter;
	l.n_rungs = n_factors;
	l.x = d_x;
	l.factors = d_factors;
	l.value = d_block_value;
	l.out_w = d_out_w;
	l.out_h = d_out_h;
	l.out_px = d_out_pixels;
	l.slot_bytes = p.block_w * p.block_h * frames->channels;
	put_layout(bare, &l);
	if (ts) put_tables(*ts, &l);
	build_breaks(h, p.mode, p.factor, &l);
	PXZ_HIP(h, pxz::launch_ladder(l, frames->channels, pxz::waves_per_tile(l.bw, l.bh), h->n_cus, h->stream));
	return PXZ_OK;
}

// frames: the OUTPUT batch (its channels = bytes per output pixel); slot_channels: channels of the stored tiles
static int expand_launch(pxz_handle *h, const pxz_frames *frames, uint32_t slot_channels, const pxz_params *params,
                         const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_out_pixels,
                         bool quiet_empty = false)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	const pxz_params p = decode_side_params(params, true);
	int rc = check_frames(h, frames, &p);
	if (rc != PXZ_OK) return rc;
	if (!d_tile_w || !d_tile_h || !d_slots || !d_out_pixels) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	PXZ_HIP(h, hipSetDevice(h->device));
	const uint32_t bw = p.block_w, bh = p.block_h;
	Grid g;
	if ((rc = make_grid(h, frames->width, frames->height, bw, bh, frames->n_frames, 0xffffffffull, &g)) != PXZ_OK) return rc;
	const uint32_t cols = g.cols, rows = g.rows;
	if (bw > 0xffffu || bh > 0xffffu) return fail(h, PXZ_ERR_UNSUPPORTED, "block side above 65535");
	// one wave: source pixels + horizontal-pass result + the staged windows (5 dwords per output sample of both axes)
	const uint64_t lds_bytes = (2ull * bw * bh + 5ull * (bw + bh) + 3ull) / 4ull * 16ull + 16ull;
	// (round 4) a tile image beyond LDS lives in HBM, one per wave of the grid (expand_kernel<C, false, true>)
	const bool big = lds_bytes > 160u * 1024u;
	if (big && ((uint64_t)bw * bh >= (1u << 20) || pxz::knobs().no_big_tiles))
		return fail(h, PXZ_ERR_UNSUPPORTED, "a %ux%u tile needs %llu B of LDS (limit 163840) and has too many pixels for the HBM-resident form (limit 2^20 - 1)", bw, bh, (unsigned long long)lds_bytes);
	pxz::ExpandArgs a{};
	a.tile_w = d_tile_w;
	a.tile_h = d_tile_h;
	a.slots = d_slots;
	a.dst = d_out_pixels;
	a.frame_stride = pxz::frame_stride_of(*frames);
	a.pitch = frames->pitch_bytes;
	a.width = frames->width;
	a.height = frames->height;
	a.channels = slot_channels;
	a.bw = bw;
	a.bh = bh;
	put_grid(g, &a);
	a.slot_bytes = bw * bh * slot_channels;
	a.filter = p.filter;
	a.out_channels = frames->channels;
	a.quiet_empty = quiet_empty ? 1u : 0u;
	const ExpandTables *et = nullptr;
	if ((rc = get_expand_tables(h, bw, bh, a.edge_w, a.edge_h, p.filter, &et)) != PXZ_OK) return rc;
	a.tabs = et->d_dir;
	a.dir_stride = et->dir_stride;
	a.starts = et->d_starts;
	a.sizes = et->d_sizes;
	a.coeffs = et->d_coeffs;
	a.fast32 = pxz::knobs().no_expand_fast32 ? 0u : 1u;
	a.xmf = a.fast32 ? et->d_xmf : nullptr;
	a.tile_dw = (2u * bw * bh + 5u * (bw + bh) + 3u) & ~3u;
	if (big) {
		uint64_t waves = (2ull << 30) / ((uint64_t)a.tile_dw * 4u);
		if (waves > 8ull * h->n_cus) waves = 8ull * h->n_cus;
		waves &= ~3ull;
		if (waves < 4) waves = 4;
		if ((rc = ensure(h, h->bigscratch, (size_t)waves * a.tile_dw * 4u)) != PXZ_OK) return rc;
		a.big_scratch = (uint32_t *)h->bigscratch.ptr;
		a.big_waves = (uint32_t)waves;
	}
	// 16x16 RGBA tiles in RGBA frames: expand16_kernel takes the 2x2 groups of full tiles (clones, powers of two), the rest -- and
	// what it leaves -- goes to expand_kernel through a list (status[1] counts it)
	const bool groups16 = a.fast32 && bw == 16 && bh == 16 && slot_channels == 4 && frames->channels == 4 && cols >= 2 && rows >= 2 &&
	                      (p.filter == 0 || et->d_xmf16 != nullptr);
	if (groups16) {
		if ((rc = ensure(h, h->xlist, (size_t)a.n_tiles * 4u)) != PXZ_OK) return rc;
		a.list = (uint32_t *)h->xlist.ptr;
		a.xmf16 = et->d_xmf16;
		a.div_gpf = make_fastdiv(((cols + 1u) / 2u) * ((rows + 1u) / 2u));
		a.div_gcols = make_fastdiv((cols + 1u) / 2u);
	}
	// 64x64 RGBA tiles in RGBA frames (the reference CLI's default block): expand64_kernel takes the full tiles stored at powers
	// of two (clones, Nearest, the two-pass convolutions), expand_kernel the rest through the list
	const bool fast64 = a.fast32 && bw == 64 && bh == 64 && ((slot_channels == 4 && frames->channels == 4) || (slot_channels == 3 && frames->channels == 3)) &&
	                    (p.filter == 0 || et->d_xmf64 != nullptr);
	if (fast64) {
		if ((rc = ensure(h, h->xlist, (size_t)a.n_tiles * 4u)) != PXZ_OK) return rc;
		a.list = (uint32_t *)h->xlist.ptr;
		a.xmf64 = et->d_xmf64;
		a.div_gpf = make_fastdiv(cols * rows);  // (tiles per frame, tile columns)
		a.div_gcols = make_fastdiv(cols);
	}
#ifdef PXZ_STAMPS
	constexpr size_t status_bytes = 256;  // (stamps behind the flags: pxz_debug_read_status)
#else
	constexpr size_t status_bytes = 8;
#endif
	if ((rc = ensure(h, h->status, status_bytes)) != PXZ_OK) return rc;
	a.status = (uint32_t *)h->status.ptr;
	PXZ_HIP(h, hipMemsetAsync(a.status, 0, 8, h->stream));
	PXZ_HIP(h, pxz::launch_expand(a, h->n_cus, h->stream));
	return PXZ_OK;
}

int pxz_expand_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, const uint32_t *d_tile_w,
                             const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	return expand_launch(h, frames, frames->channels, params, d_tile_w, d_tile_h, d_slots, d_out_pixels);
}

int pxz_process_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, uint32_t filter_upscale,
                              const uint8_t *d_pixels, uint8_t *d_out_rgba, uint32_t out_pitch_bytes,
                              uint64_t out_frame_stride_bytes)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	if (!d_pixels || !d_out_rgba) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (filter_upscale > 4) return fail(h, PXZ_ERR_INVALID_ARG, "filter must be 0..4");
	PXZ_HIP(h, hipSetDevice(h->device));
	// 1) get_block_variance with |x - avg| and the identity (process/mod.rs:108-111) -> reduce_image_section((v, v))
	pxz_params p = *params;
	p.mode = PXZ_MODE_SHRINK_BY;
	p.factor = 1.0f;
	int rc = check_frames(h, frames, &p);
	if (rc != PXZ_OK) return rc;
	Grid g;
	(void)make_grid(h, frames->width, frames->height, p.block_w, p.block_h, frames->n_frames, kAnyTiles, &g);  // (run_shrink checks)
	const size_t tiles = (size_t)g.tiles, slot = (size_t)p.block_w * p.block_h * frames->channels;
	if ((rc = ensure_tile_outputs(h, tiles, slot)) != PXZ_OK) return rc;
	if ((rc = run_shrink(h, frames, &p, d_pixels, (float *)h->val.ptr, (uint32_t *)h->ow.ptr, (uint32_t *)h->oh.ptr,
	                     (uint8_t *)h->out.ptr, nullptr, nullptr, true)) != PXZ_OK)
		return rc;
	// 2) .resize(w0, h0, filter_upscale) + copy_from into the RGBA output (process/mod.rs:58-63)
	pxz_frames of{frames->width, frames->height, 4, out_pitch_bytes, frames->n_frames, 0, out_frame_stride_bytes};
	pxz_params up{params->block_w, params->block_h, 0, filter_upscale, 0.0f, 0};
	return expand_launch(h, &of, frames->channels, &up, (const uint32_t *)h->ow.ptr, (const uint32_t *)h->oh.ptr,
	                     (const uint8_t *)h->out.ptr, d_out_rgba);
}

namespace {
// tree::process for any block geometry (round 3): the levels of the recursion as lists of rectangles, one launch of
// pxz::tree_rect_kernel per level (pxz_tree.hip).  The host only learns how many tiles went on to the next level -- one
// 4-byte read-back per level.
int tree_process_rects(pxz_handle *h, const pxz_frames *frames, const pxz_params &p, uint32_t filter_upscale, float threshold,
                       uint32_t mbw, uint32_t mbh, const std::vector<std::pair<uint32_t, uint32_t>> &levels, const uint8_t *d_pixels,
                       uint8_t *d_out_rgba, uint32_t out_pitch_bytes, uint64_t src_stride, uint64_t dst_stride)
{
	constexpr uint32_t kMaxSide = 128;  // pxz_tree.hip: kTreeMaxSide
	if (levels[0].first > kMaxSide || levels[0].second > kMaxSide)
		return fail(h, PXZ_ERR_UNSUPPORTED, "tree::process on the device takes blocks up to %ux%u (got %ux%u)", kMaxSide, kMaxSide,
		            levels[0].first, levels[0].second);
	const TreeTables *ttp = nullptr;
	int rc = cached_tables(h, h->tree_tables,
	                       std::make_tuple(frames->width, frames->height, levels[0].first, levels[0].second, mbw, mbh, p.filter, filter_upscale),
	                       kTableCacheBound, [&](TreeTables &t) {
		pxz::TreeTableSet s;
		if (!pxz::build_tree_tables(frames->width, frames->height, levels, p.filter, filter_upscale, &s))
			return fail(h, PXZ_ERR_INVALID_ARG, "unknown filter");
		t.n_dir = (uint32_t)s.dir.size();
		return upload_tables(h, {{s.dir, &t.d_dir}, {s.starts, &t.d_starts}, {s.sizes, &t.d_sizes}, {s.coeffs, &t.d_coeffs}}, &t.mem);
	}, &ttp);
	if (rc != PXZ_OK) return rc;
	const TreeTables &tt = *ttp;
	// ---- level 0: the frame's own grid (split.rs:37-61)
	Grid g;
	if ((rc = make_grid(h, frames->width, frames->height, levels[0].first, levels[0].second, frames->n_frames, 0x0fffffffull, &g)) != PXZ_OK) return rc;
	const uint32_t cols = g.cols, rows = g.rows;
	uint32_t n = (uint32_t)g.tiles;
	{
		std::vector<pxz::TreeRect> r0(n);
		size_t i = 0;
		for (uint32_t f = 0; f < frames->n_frames; ++f)
			for (uint32_t ty = 0; ty < rows; ++ty)
				for (uint32_t tx = 0; tx < cols; ++tx, ++i) {
					r0[i].x = tx * levels[0].first;
					r0[i].y = ty * levels[0].second;
					r0[i].w = (uint16_t)std::min(levels[0].first, frames->width - r0[i].x);
					r0[i].h = (uint16_t)std::min(levels[0].second, frames->height - r0[i].y);
					r0[i].frame = f;
				}
		if ((rc = ensure(h, h->tree_rects[0], (size_t)n * sizeof(pxz::TreeRect))) != PXZ_OK) return rc;
		PXZ_HIP(h, hipMemcpyAsync(h->tree_rects[0].ptr, r0.data(), (size_t)n * sizeof(pxz::TreeRect), hipMemcpyHostToDevice, h->stream));
		PXZ_HIP(h, hipStreamSynchronize(h->stream));  // (r0 leaves scope)
	}
	if ((rc = ensure(h, h->tree_count, 64)) != PXZ_OK) return rc;
	pxz::TreeRectArgs a{};
	a.src = d_pixels;
	a.dst = d_out_rgba;
	a.src_frame_stride = src_stride;
	a.dst_frame_stride = dst_stride;
	a.src_pitch = frames->pitch_bytes;
	a.dst_pitch = out_pitch_bytes;
	a.channels = frames->channels;
	a.filter_down = p.filter;
	a.filter_up = filter_upscale;
	a.dir = tt.d_dir;
	a.n_dir = tt.n_dir;
	a.starts = tt.d_starts;
	a.sizes = tt.d_sizes;
	a.coeffs = tt.d_coeffs;
	std::memcpy(a.thresholds, h->thresholds, sizeof a.thresholds);
	PXZ_HIP(h, hipMemsetAsync(h->tree_count.ptr, 0, 8, h->stream));  // [0] the next level's tile count, [1] "an axis table was missing"
	for (size_t l = 0; l < levels.size() && n != 0; ++l) {
		const bool leaf_next = l + 1 == levels.size();
		const uint32_t nbw = levels[l].first >> 1, nbh = levels[l].second >> 1;
		// every tile of this level may go on: (ceil(bw / (bw >> 1)))^2 children each at most
		const uint64_t per_tile = leaf_next ? 0 : (uint64_t)((levels[l].first + nbw - 1) / nbw) * ((levels[l].second + nbh - 1) / nbh);
		const uint64_t cap = per_tile * n;
		if (cap > 0x7fffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "too many tiles");
		DeviceBuffer &cur = h->tree_rects[l & 1], &nxt = h->tree_rects[(l + 1) & 1];
		if (!leaf_next && (rc = ensure(h, nxt, (size_t)cap * sizeof(pxz::TreeRect))) != PXZ_OK) return rc;
		PXZ_HIP(h, hipMemsetAsync(h->tree_count.ptr, 0, 4, h->stream));
		a.rects = (const pxz::TreeRect *)cur.ptr;
		a.n_rects = n;
		a.threshold = std::fabs(threshold);
		a.positive = (l == 0 ? threshold >= 0.0f : true) ? 1u : 0u;  // tree.rs:37-38: the recursion passes |threshold| on
		a.next_bw = nbw;
		a.next_bh = nbh;
		a.next_is_leaf = leaf_next ? 1u : 0u;
		a.next_rects = leaf_next ? nullptr : (pxz::TreeRect *)nxt.ptr;
		a.next_count = (uint32_t *)h->tree_count.ptr;
		a.next_capacity = (uint32_t)cap;
		PXZ_HIP(h, pxz::launch_tree_rects(a, h->stream));
		uint32_t back[2] = {0, 0};
		PXZ_HIP(h, hipMemcpyAsync(back, h->tree_count.ptr, 8, hipMemcpyDeviceToHost, h->stream));
		PXZ_HIP(h, hipStreamSynchronize(h->stream));
		if (back[1] != 0) return fail(h, PXZ_ERR_INTERNAL, "tree::process: level %zu met a tile size the axis tables do not list", l);
		if (leaf_next) break;
		if (back[0] > cap) return fail(h, PXZ_ERR_HIP, "tree::process: %u tiles for a list of %llu", back[0], (unsigned long long)cap);
		n = back[0];
	}
	return PXZ_OK;
}
}  // namespace

int pxz_tree_process_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, uint32_t filter_upscale,
                                   float threshold, uint32_t min_block_w, uint32_t min_block_h, const uint8_t *d_pixels,
                                   uint8_t *d_out_rgba, uint32_t out_pitch_bytes, uint64_t out_frame_stride_bytes)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	if (!d_pixels || !d_out_rgba) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (filter_upscale > 4) return fail(h, PXZ_ERR_INVALID_ARG, "filter must be 0..4");
	if (!std::isfinite(threshold)) return fail(h, PXZ_ERR_INVALID_ARG, "threshold must be finite");
	pxz_params p = *params;
	p.mode = PXZ_MODE_SHRINK_BY;
	p.factor = 1.0f;
	int rc = check_frames(h, frames, &p);
	if (rc != PXZ_OK) return rc;
	if ((uint64_t)out_pitch_bytes < (uint64_t)frames->width * 4u) return fail(h, PXZ_ERR_INVALID_ARG, "output pitch smaller than a row");
	// (the kernels store whole RGBA pixels)
	if ((reinterpret_cast<uintptr_t>(d_out_rgba) & 3u) != 0 || (out_pitch_bytes & 3u) != 0 || (frames->n_frames > 1 && (out_frame_stride_bytes & 3u) != 0))
		return fail(h, PXZ_ERR_INVALID_ARG, "the RGBA output must be 4-byte aligned (pointer, pitch and frame stride)");
	PXZ_HIP(h, hipSetDevice(h->device));
	// the levels of the recursion (tree.rs:32-36): block sizes halve while both stay above the minimum (at least 4)
	const uint32_t mbw = min_block_w > 4u ? min_block_w : 4u, mbh = min_block_h > 4u ? min_block_h : 4u;
	std::vector<std::pair<uint32_t, uint32_t>> levels;
	for (uint32_t bw = p.block_w, bh = p.block_h; bw > mbw && bh > mbh; bw >>= 1, bh >>= 1) levels.emplace_back(bw, bh);
	const uint64_t src_stride = pxz::frame_stride_of(*frames);
	const uint64_t dst_stride = frames->n_frames > 1 ? out_frame_stride_bytes : (uint64_t)out_pitch_bytes * frames->height;
	// A level's tiles are the children of the level before: they form that level's regular grid over the frame as long as
	// a block is exactly two of the next (the recursion splits every tile from its own corner), and the per-level passes
	// below need tiles that fit the fused kernel's LDS image.  Anything else -- 50 -> 25 -> 12, the 128-px blocks of
	// src/bin/tree.rs:6 -- goes level by level over lists of rectangles (round 3).
	bool regular = !pxz::knobs().tree_rects;
	for (size_t l = 0; l + 1 < levels.size(); ++l)
		if ((levels[l].first & 1u) || (levels[l].second & 1u)) regular = false;
	if (!levels.empty() && (levels[0].first > 64u || levels[0].second > 64u)) regular = false;
	if (!regular && !levels.empty())
		return tree_process_rects(h, frames, p, filter_upscale, threshold, mbw, mbh, levels, d_pixels, d_out_rgba, out_pitch_bytes,
		                          src_stride, dst_stride);
	pxz::TreeArgs t{};
	t.src = d_pixels;
	t.dst = d_out_rgba;
	t.src_frame_stride = src_stride;
	t.dst_frame_stride = dst_stride;
	t.src_pitch = frames->pitch_bytes;
	t.dst_pitch = out_pitch_bytes;
	t.channels = frames->channels;
	if (levels.empty()) {
		// tree.rs:34-36: the image comes back as it is (as RGBA here): a plain 2-D copy / widening of the frames
		if (frames->channels == 4) {
			for (uint32_t f = 0; f < frames->n_frames; ++f)
				PXZ_HIP(h, hipMemcpy2DAsync(d_out_rgba + (size_t)f * dst_stride, out_pitch_bytes, d_pixels + (size_t)f * src_stride, frames->pitch_bytes,
				                            (size_t)frames->width * 4u, frames->height, hipMemcpyDeviceToDevice, h->stream));
		} else {
			pxz::WidenArgs wa{d_pixels, d_out_rgba, src_stride, dst_stride, frames->pitch_bytes, out_pitch_bytes, frames->width, frames->height, frames->n_frames};
			PXZ_HIP(h, pxz::launch_widen(wa, h->stream));
		}
		return PXZ_OK;
	}
	uint32_t prev_cols = 0, prev_tpf = 0;
	size_t max_tiles = 0;
	for (auto &lv : levels) {
		Grid g;
		if ((rc = make_grid(h, frames->width, frames->height, lv.first, lv.second, frames->n_frames, 0xffffffffull, &g)) != PXZ_OK) return rc;
		max_tiles = std::max(max_tiles, (size_t)g.tiles);
	}
	// per tile: the detector's own output (the stored block value is hypot(v, v), operations.rs:154) + two sets of flags
	if ((rc = ensure(h, h->tree, 4 * max_tiles + 2 * max_tiles)) != PXZ_OK) return rc;
	float *raw_value = (float *)h->tree.ptr;
	uint8_t *open_flags[2] = {(uint8_t *)h->tree.ptr + 4 * max_tiles, (uint8_t *)h->tree.ptr + 5 * max_tiles};
	const bool whole = p.block_w <= mbw || p.block_h <= mbh;
	for (size_t l = 0; l < levels.size(); ++l) {
		const uint32_t bw = levels[l].first, bh = levels[l].second;
		Grid g;
		(void)make_grid(h, frames->width, frames->height, bw, bh, frames->n_frames, kAnyTiles, &g);  // (checked above)
		const size_t tiles = (size_t)g.tiles, slot = (size_t)bw * bh * frames->channels;
		if ((rc = ensure_tile_outputs(h, tiles, whole ? 0 : slot)) != PXZ_OK) return rc;
		if (!whole) {
			// get_block_variance + reduce_image_section((v, v)) of every tile of this level's grid (process/mod.rs:84-95); the
			// tiles that do not take part are discarded by the decision below
			pxz_params lp = p;
			lp.block_w = bw;
			lp.block_h = bh;
			if ((rc = run_shrink(h, frames, &lp, d_pixels, (float *)h->val.ptr, (uint32_t *)h->ow.ptr, (uint32_t *)h->oh.ptr,
			                     (uint8_t *)h->out.ptr, raw_value, nullptr, true)) != PXZ_OK)
				return rc;
		} else {
			PXZ_HIP(h, hipMemsetAsync(raw_value, 0, tiles * 4, h->stream));
		}
		t.value = raw_value;
		t.tile_w = (uint32_t *)h->ow.ptr;
		t.tile_h = (uint32_t *)h->oh.ptr;
		t.parent_open = l ? open_flags[(l - 1) & 1] : nullptr;
		t.open = open_flags[l & 1];
		t.bw = bw;
		t.bh = bh;
		put_grid(g, &t);
		t.parent_cols = prev_cols;
		t.parent_tiles_per_frame = prev_tpf;
		t.threshold = whole ? 1.0f : std::fabs(threshold);
		t.positive = whole ? 0u : ((l == 0 ? threshold >= 0.0f : true) ? 1u : 0u);  // whole: (0 >= 1) ^ false = false: nothing is pixelised
		t.last = l + 1 == levels.size() ? 1u : 0u;
		PXZ_HIP(h, pxz::launch_tree_decide(t, h->stream));
		if (!whole) {
			pxz_frames of{frames->width, frames->height, 4, out_pitch_bytes, frames->n_frames, 0, out_frame_stride_bytes};
			pxz_params up{bw, bh, 0, filter_upscale, 0.0f, 0};
			if ((rc = expand_launch(h, &of, frames->channels, &up, (const uint32_t *)h->ow.ptr, (const uint32_t *)h->oh.ptr,
			                        (const uint8_t *)h->out.ptr, d_out_rgba, true)) != PXZ_OK)
				return rc;
		}
		prev_cols = g.cols;
		prev_tpf = g.tiles_per_frame;
	}
	return PXZ_OK;
}

// The reader's scratch (pxz_stream.hip), for a.n_tiles tiles: rec_off, rec_len, perm and the bin counters in dmeta, and the
// status word, zeroed, with room for the stamps of the diagnostic build behind it (pxz_debug_read_status).
static int reader_scratch(pxz_handle *h, pxz::DecodeArgs *a)
{
	int rc = ensure_bins(h, h->dmeta, (size_t)a->n_tiles * 16u + 4u * pxz::qoi_bins_dwords(), h->dbins_clean);
	if (rc != PXZ_OK) return rc;
	a->rec_off = (unsigned long long *)h->dmeta.ptr;
	a->rec_len = (uint32_t *)((uint8_t *)h->dmeta.ptr + (size_t)a->n_tiles * 8u);
	a->perm = a->rec_len + a->n_tiles;
	a->bins = a->perm + a->n_tiles;
	if ((rc = ensure(h, h->status, 256)) != PXZ_OK) return rc;
	a->status = (uint32_t *)h->status.ptr;
	PXZ_HIP(h, hipMemsetAsync(a->status, 0, 4, h->stream));
	return PXZ_OK;
}

int pxz_decode_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, const uint8_t *d_files,
                             const uint64_t *d_file_offsets, float *d_block_value, uint32_t *d_tile_w, uint32_t *d_tile_h,
                             uint8_t *d_slots)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	const pxz_params p = decode_side_params(params, false);
	pxz_frames f = *frames;
	f.pitch_bytes = f.width * f.channels;  // only the geometry of the frames matters here
	f.frame_stride_bytes = (uint64_t)f.pitch_bytes * f.height;
	int rc = check_frames(h, &f, &p);
	if (rc != PXZ_OK) return rc;
	if (!d_files || !d_file_offsets || !d_block_value || !d_tile_w || !d_tile_h || !d_slots)
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	PXZ_HIP(h, hipSetDevice(h->device));
	Grid g;
	if ((rc = make_grid(h, f.width, f.height, p.block_w, p.block_h, f.n_frames, 0xffffffffull, &g)) != PXZ_OK) return rc;
	pxz::DecodeArgs a{};
	a.files = d_files;
	a.file_offsets = reinterpret_cast<const unsigned long long *>(d_file_offsets);
	a.value = d_block_value;
	a.tile_w = d_tile_w;
	a.tile_h = d_tile_h;
	a.slots = d_slots;
	a.width = f.width;
	a.height = f.height;
	a.bw = p.block_w;
	a.bh = p.block_h;
	put_grid(g, &a);
	a.n_frames = f.n_frames;
	a.channels = f.channels;
	a.slot_bytes = p.block_w * p.block_h * f.channels;
	if ((rc = reader_scratch(h, &a)) != PXZ_OK) return rc;
	return launch_on_bins(h, h->dbins_clean, a.bins, [&](bool bins_clean) { return pxz::launch_decode(a, bins_clean, h->stream); });
}

int pxz_file_header(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint32_t *block_w, uint32_t *block_h,
                    uint32_t *channels, uint32_t *filter_byte)
{
	const char *why;
	return file_header(file, len, width, height, block_w, block_h, channels, filter_byte, &why);
}

int pxz_decode_file(pxz_handle *h, const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint32_t *block_w,
                    uint32_t *block_h, uint32_t *channels, uint32_t *filter_byte, float *block_value, uint32_t *tile_w,
                    uint32_t *tile_h, uint8_t *slots)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	const char *why;
	int hrc = file_header(file, len, width, height, block_w, block_h, channels, filter_byte, &why);
	if (hrc != PXZ_OK) return fail(h, hrc, "%s", why);
	if (!block_value && !tile_w && !tile_h && !slots) return PXZ_OK;  // header query
	if (!block_value || !tile_w || !tile_h || !slots) return fail(h, PXZ_ERR_INVALID_ARG, "null output pointer");
	PXZ_HIP(h, hipSetDevice(h->device));
	Grid g;
	(void)make_grid(h, *width, *height, *block_w, *block_h, 1, kAnyTiles, &g);
	const size_t tiles = (size_t)g.tiles, slot = (size_t)*block_w * *block_h * *channels;
	int rc;
	if ((rc = ensure(h, h->in, len + 16)) != PXZ_OK) return rc;
	if ((rc = ensure_tile_outputs(h, tiles, slot)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->chunks, 16)) != PXZ_OK) return rc;
	const uint64_t offs[2] = {0, (uint64_t)len};
	PXZ_HIP(h, hipMemcpyAsync(h->in.ptr, file, len, hipMemcpyHostToDevice, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(h->chunks.ptr, offs, 16, hipMemcpyHostToDevice, h->stream));
	PXZ_HIP(h, hipMemsetAsync(h->out.ptr, 0, tiles * slot, h->stream));
	pxz_frames f{*width, *height, *channels, *width * *channels, 1, 0, 0};
	pxz_params p{*block_w, *block_h, 0, 0, 0.0f, 0};
	rc = pxz_decode_frames_device(h, &f, &p, (const uint8_t *)h->in.ptr, (const uint64_t *)h->chunks.ptr, (float *)h->val.ptr,
	                              (uint32_t *)h->ow.ptr, (uint32_t *)h->oh.ptr, (uint8_t *)h->out.ptr);
	if (rc != PXZ_OK) return rc;
	if ((rc = download_tile_outputs(h, tiles, slot, block_value, tile_w, tile_h, slots)) != PXZ_OK) return rc;
	uint32_t flags = 0;
	if ((rc = pxz_decode_status(h, &flags)) != PXZ_OK) return rc;
	if (flags & 2u) return fail(h, PXZ_ERR_INVALID_ARG, "malformed .pixlzr file or record");
	return PXZ_OK;
}

int pxz_decode_status(pxz_handle *h, uint32_t *flags)
{
	if (!h || !flags) return PXZ_ERR_INVALID_ARG;
	*flags = 0;
	if (!h->status.ptr) return PXZ_OK;
	PXZ_HIP(h, hipSetDevice(h->device));
	PXZ_HIP(h, hipMemcpyAsync(flags, h->status.ptr, 4, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	return PXZ_OK;
}

int pxz_expand_image(pxz_handle *h, uint32_t width, uint32_t height, uint32_t channels, uint32_t pitch_bytes, uint32_t block_w,
                     uint32_t block_h, uint32_t filter, const uint32_t *tile_w, const uint32_t *tile_h, const uint8_t *slots,
                     uint8_t *out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!tile_w || !tile_h || !slots || !out_pixels) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	pxz_frames f{width, height, channels, pitch_bytes, 1, 0, 0};
	pxz_params p{block_w, block_h, 0, filter, 0.0f, 0};
	int rc = check_frames(h, &f, &p);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	Grid g;
	(void)make_grid(h, width, height, block_w, block_h, 1, kAnyTiles, &g);
	const size_t tiles = (size_t)g.tiles, slot = (size_t)block_w * block_h * channels;
	const size_t out_bytes = (size_t)pitch_bytes * (height - 1) + (size_t)width * channels;
	if ((rc = ensure(h, h->ow, tiles * 4)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->oh, tiles * 4)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->out, tiles * slot)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->in, out_bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipMemcpyAsync(h->ow.ptr, tile_w, tiles * 4, hipMemcpyHostToDevice, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(h->oh.ptr, tile_h, tiles * 4, hipMemcpyHostToDevice, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(h->out.ptr, slots, tiles * slot, hipMemcpyHostToDevice, h->stream));
	PXZ_HIP(h, hipMemsetAsync(h->in.ptr, 0, out_bytes, h->stream));  // row padding of a pitched image stays zero
	rc = pxz_expand_frames_device(h, &f, &p, (const uint32_t *)h->ow.ptr, (const uint32_t *)h->oh.ptr, (const uint8_t *)h->out.ptr,
	                              (uint8_t *)h->in.ptr);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipMemcpyAsync(out_pixels, h->in.ptr, out_bytes, hipMemcpyDeviceToHost, h->stream));
	uint32_t bad = 0;
	if ((rc = pxz_decode_status(h, &bad)) != PXZ_OK) return rc;
	if (bad) return fail(h, PXZ_ERR_INVALID_ARG, "a tile's stored size is zero or larger than its place in the image");
	return PXZ_OK;
}

}  // extern "C"

namespace pxz_runtime {

// The front half of the host-buffer entry points of one image (pxz_shrink_image, _ladder, _packed, pxz_rate_distortion_image)
// after their pointer checks: the checks of the geometry, the transparency hint (*p), the tile outputs of `sets` results in
// handle scratch (the pixels only with device_px) and the upload.  *f: the frame with its device pitch; *tiles: the tiles of
// all sets; *slot: bytes of one slot.
int stage_host_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t pitch_bytes,
                     pxz_params *p, uint32_t sets, bool device_px, pxz_frames *f, size_t *tiles, size_t *slot)
{
	*f = pxz_frames{width, height, channels, pitch_bytes, 1, 0, 0};
	int rc = check_frames(h, f, p);
	if (rc != PXZ_OK) return rc;
	if (channels == 4 && host_image_has_transparency(pixels, width, height, pitch_bytes)) p->reserved |= PXZ_HINT_TRANSPARENCY;
	PXZ_HIP(h, hipSetDevice(h->device));
	Grid g;
	(void)make_grid(h, width, height, p->block_w, p->block_h, 1, kAnyTiles, &g);  // (the device call checks)
	*tiles = (size_t)g.tiles * sets;
	*slot = (size_t)p->block_w * p->block_h * channels;
	if ((rc = ensure_tile_outputs(h, *tiles, device_px ? *slot : 0)) != PXZ_OK) return rc;
	return upload_image(h, pixels, width, height, channels, pitch_bytes, &f->pitch_bytes);
}

}  // namespace pxz_runtime

namespace {

// ... then device_call(frames with the device pitch, parameters with the hint, tiles, slot bytes), and the download of the
// tile outputs (the pixels only with out_pixels).  The caller queues what it downloads besides and synchronises.
template <class DeviceCall>
int shrink_host_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t pitch_bytes,
                      pxz_params p, uint32_t sets, bool device_px, float *block_value, uint32_t *out_w, uint32_t *out_h,
                      uint8_t *out_pixels, DeviceCall device_call)
{
	pxz_frames f;
	size_t tiles = 0, slot = 0;
	int rc = stage_host_image(h, pixels, width, height, channels, pitch_bytes, &p, sets, device_px, &f, &tiles, &slot);
	if (rc != PXZ_OK) return rc;
	if ((rc = device_call(f, p, tiles, slot)) != PXZ_OK) return rc;
	return download_tile_outputs(h, tiles, slot, block_value, out_w, out_h, out_pixels);
}
}  // namespace

extern "C" {

int pxz_shrink_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                     uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter,
                     float factor, float *block_value, uint32_t *out_w, uint32_t *out_h, uint8_t *out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!pixels || !block_value || !out_w || !out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const int rc = shrink_host_image(h, pixels, width, height, channels, pitch_bytes, pxz_params{block_w, block_h, mode, filter, factor, 0}, 1,
	                                 out_pixels != nullptr, block_value, out_w, out_h, out_pixels,
	                                 [&](const pxz_frames &f, const pxz_params &p, size_t, size_t) {
		return pxz_shrink_frames_device(h, &f, &p, (const uint8_t *)h->in.ptr, (float *)h->val.ptr, (uint32_t *)h->ow.ptr,
		                                (uint32_t *)h->oh.ptr, out_pixels ? (uint8_t *)h->out.ptr : nullptr);
	});
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	return PXZ_OK;
}

int pxz_shrink_image_ladder(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                            uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter,
                            const float *factors, uint32_t n_factors, float *block_value, uint32_t *out_w, uint32_t *out_h,
                            uint8_t *out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!factors) return fail(h, PXZ_ERR_INVALID_ARG, "null factors");
	if (n_factors == 0 || n_factors > PXZ_LADDER_MAX_RUNGS)
		return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", PXZ_LADDER_MAX_RUNGS, n_factors);
	if (!pixels || !block_value || !out_w || !out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const int rc = shrink_host_image(h, pixels, width, height, channels, pitch_bytes, pxz_params{block_w, block_h, mode, filter, 1.0f, 0}, n_factors,
	                                 out_pixels != nullptr, block_value, out_w, out_h, out_pixels,
	                                 [&](const pxz_frames &f, const pxz_params &p, size_t, size_t) {
		return pxz_shrink_ladder_frames_device(h, &f, &p, factors, n_factors, (const uint8_t *)h->in.ptr, (float *)h->val.ptr,
		                                       (uint32_t *)h->ow.ptr, (uint32_t *)h->oh.ptr, out_pixels ? (uint8_t *)h->out.ptr : nullptr);
	});
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	return PXZ_OK;
}

int pxz_shrink_image_packed(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                            uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter,
                            float factor, float *block_value, uint32_t *out_w, uint32_t *out_h, uint64_t *packed_len)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	h->packed_len = 0;
	if (!pixels || !block_value || !out_w || !out_h || !packed_len) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	*packed_len = 0;
	const size_t most = (size_t)width * height * channels;  // no tile grows
	size_t n_tiles = 0;
	const int rc = shrink_host_image(h, pixels, width, height, channels, pitch_bytes, pxz_params{block_w, block_h, mode, filter, factor, 0}, 1, true,
	                                 block_value, out_w, out_h, nullptr, [&](const pxz_frames &f, const pxz_params &p, size_t tiles, size_t slot) {
		n_tiles = tiles;
		int rc = ensure(h, h->pk, most);
		if (rc == PXZ_OK) rc = ensure(h, h->pkoff, (tiles + 1) * 8);
		if (rc == PXZ_OK)
			rc = pxz_shrink_frames_device(h, &f, &p, (const uint8_t *)h->in.ptr, (float *)h->val.ptr, (uint32_t *)h->ow.ptr,
			                              (uint32_t *)h->oh.ptr, (uint8_t *)h->out.ptr);
		if (rc == PXZ_OK)
			rc = pxz_pack_tiles_device(h, (uint32_t)tiles, channels, (uint32_t)slot, (const uint32_t *)h->ow.ptr, (const uint32_t *)h->oh.ptr,
			                           (const uint8_t *)h->out.ptr, (uint64_t *)h->pkoff.ptr, (uint8_t *)h->pk.ptr, most);
		return rc;
	});
	if (rc != PXZ_OK) return rc;
	uint64_t total = 0;
	PXZ_HIP(h, hipMemcpyAsync(&total, (const uint64_t *)h->pkoff.ptr + n_tiles, 8, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	if (total > most) return fail(h, PXZ_ERR_HIP, "packed stream longer than the image (%llu > %zu)", (unsigned long long)total, most);
	h->packed_len = total;
	*packed_len = total;
	return PXZ_OK;
}

// pxz_shrink_images / pxz_shrink_images_packed: pxz_shrink_image[_packed] over a list of equally sized host images, as a
// three-stage pipeline over three sets of device buffers -- the upload of image k + 1, the kernels of image k and the
// download of image k - 1 run at the same time (two copy streams driven by two helper threads: a copy from or to pageable
// host memory blocks its caller), so the list costs about one PCIe direction per image instead of the sum of both.
static int shrink_images_impl(pxz_handle *h, const uint8_t *const *pixels, uint32_t n_images, uint32_t width, uint32_t height,
                              uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode,
                              uint32_t filter, float factor, float *const *block_value, uint32_t *const *out_w,
                              uint32_t *const *out_h, uint8_t *const *out_pixels, bool packed, uint64_t capacity,
                              uint64_t *packed_len)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!pixels || !block_value || !out_w || !out_h || n_images == 0 || (packed && (!out_pixels || !packed_len)))
		return fail(h, PXZ_ERR_INVALID_ARG, "null pointer or empty list");
	for (uint32_t k = 0; k < n_images; ++k)
		if (!pixels[k] || !block_value[k] || !out_w[k] || !out_h[k] || (packed && !out_pixels[k]))
			return fail(h, PXZ_ERR_INVALID_ARG, "null pointer in the list (image %u)", k);
	pxz_frames f{width, height, channels, pitch_bytes, 1, 0, 0};
	pxz_params p{block_w, block_h, mode, filter, factor, 0};
	int rc = check_frames(h, &f, &p);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	Grid g;
	(void)make_grid(h, width, height, block_w, block_h, 1, kAnyTiles, &g);  // (the device calls check)
	const size_t tiles = (size_t)g.tiles, slot = (size_t)block_w * block_h * channels;
	const size_t most = (size_t)width * height * channels;  // no tile grows
	const size_t row_bytes = (size_t)width * channels;
	const uint32_t dp = device_pitch_of(width, channels, pitch_bytes);
	const size_t in_bytes = (size_t)dp * (height - 1) + row_bytes;
	const bool want_px = packed || out_pixels != nullptr;
	constexpr int R = HandleScratch::kRing;
	for (int i = 0; i < R; ++i) {
		if ((rc = ensure(h, h->ring_in[i], in_bytes)) != PXZ_OK) return rc;
		if ((rc = ensure(h, h->ring_val[i], tiles * 4)) != PXZ_OK) return rc;
		if ((rc = ensure(h, h->ring_ow[i], tiles * 4)) != PXZ_OK) return rc;
		if ((rc = ensure(h, h->ring_oh[i], tiles * 4)) != PXZ_OK) return rc;
		if (want_px && (rc = ensure(h, h->ring_out[i], tiles * slot)) != PXZ_OK) return rc;
		if (packed && (rc = ensure(h, h->ring_pk[i], most)) != PXZ_OK) return rc;
		if (packed && (rc = ensure(h, h->ring_pkoff[i], (tiles + 1) * 8)) != PXZ_OK) return rc;
	}
	hipStream_t up = nullptr, down = nullptr;
	PXZ_HIP(h, hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
	if (hipStreamCreateWithFlags(&down, hipStreamNonBlocking) != hipSuccess) {
		(void)hipStreamDestroy(up);
		return fail(h, PXZ_ERR_HIP, "hipStreamCreateWithFlags failed");
	}
	std::mutex m;
	std::condition_variable cv;
	uint32_t uploaded = 0, computed = 0, downloaded = 0;
	hipError_t copy_error = hipSuccess;
	bool stop = false;
	const int device = h->device;

	auto upload_fn = [&] {
		(void)hipSetDevice(device);
		for (uint32_t k = 0; k < n_images; ++k) {
			{
				std::unique_lock<std::mutex> lk(m);
				cv.wait(lk, [&] { return stop || k < downloaded + (uint32_t)R; });  // its buffer set is free again
				if (stop) return;
			}
			void *dst = h->ring_in[k % R].ptr;
			hipError_t e = dp == pitch_bytes ? hipMemcpyAsync(dst, pixels[k], in_bytes, hipMemcpyHostToDevice, up)
			                                 : hipMemcpy2DAsync(dst, dp, pixels[k], pitch_bytes, row_bytes, height, hipMemcpyHostToDevice, up);
			if (e == hipSuccess) e = hipStreamSynchronize(up);
			std::lock_guard<std::mutex> lk(m);
			if (e != hipSuccess) {
				copy_error = e;
				stop = true;
			} else {
				uploaded = k + 1;
			}
			cv.notify_all();
			if (stop) return;
		}
	};
	auto download_fn = [&] {
		(void)hipSetDevice(device);
		for (uint32_t k = 0; k < n_images; ++k) {
			{
				std::unique_lock<std::mutex> lk(m);
				cv.wait(lk, [&] { return stop || computed > k; });
				if (stop) return;
			}
			const int i = (int)(k % R);
			hipError_t e = hipMemcpyAsync(block_value[k], h->ring_val[i].ptr, tiles * 4, hipMemcpyDeviceToHost, down);
			if (e == hipSuccess) e = hipMemcpyAsync(out_w[k], h->ring_ow[i].ptr, tiles * 4, hipMemcpyDeviceToHost, down);
			if (e == hipSuccess) e = hipMemcpyAsync(out_h[k], h->ring_oh[i].ptr, tiles * 4, hipMemcpyDeviceToHost, down);
			if (e == hipSuccess && packed) {
				uint64_t total = 0;
				e = hipMemcpyAsync(&total, (const uint64_t *)h->ring_pkoff[i].ptr + tiles, 8, hipMemcpyDeviceToHost, down);
				if (e == hipSuccess) e = hipStreamSynchronize(down);
				packed_len[k] = total;
				if (e == hipSuccess && total <= capacity && total <= most && total)
					e = hipMemcpyAsync(out_pixels[k], h->ring_pk[i].ptr, total, hipMemcpyDeviceToHost, down);
			} else if (e == hipSuccess && out_pixels && out_pixels[k]) {
				e = hipMemcpyAsync(out_pixels[k], h->ring_out[i].ptr, tiles * slot, hipMemcpyDeviceToHost, down);
			}
			if (e == hipSuccess) e = hipStreamSynchronize(down);
			std::lock_guard<std::mutex> lk(m);
			if (e != hipSuccess) {
				copy_error = e;
				stop = true;
			} else {
				downloaded = k + 1;
			}
			cv.notify_all();
			if (stop) return;
		}
	};
	// (a thread that cannot be started must not take the process down: nothing may be thrown across the C boundary)
	std::thread uploader, downloader;
	try {
		uploader = std::thread(upload_fn);
		downloader = std::thread(download_fn);
	} catch (const std::system_error &) {
		{
			std::lock_guard<std::mutex> lk(m);
			stop = true;
		}
		cv.notify_all();
		if (uploader.joinable()) uploader.join();
		(void)hipStreamDestroy(up);
		(void)hipStreamDestroy(down);
		return fail(h, PXZ_ERR_HIP, "could not start the copy threads of the pipelined boundary");
	}
	// this thread: the kernels, on the handle's stream
	rc = PXZ_OK;
	for (uint32_t k = 0; k < n_images && rc == PXZ_OK; ++k) {
		{
			std::unique_lock<std::mutex> lk(m);
			cv.wait(lk, [&] { return stop || uploaded > k; });
			if (stop) break;
		}
		const int i = (int)(k % R);
		pxz_frames fk{width, height, channels, dp, 1, 0, 0};
		pxz_params pk = p;
		if (channels == 4 && host_image_has_transparency(pixels[k], width, height, pitch_bytes)) pk.reserved |= PXZ_HINT_TRANSPARENCY;
		rc = pxz_shrink_frames_device(h, &fk, &pk, (const uint8_t *)h->ring_in[i].ptr, (float *)h->ring_val[i].ptr,
		                              (uint32_t *)h->ring_ow[i].ptr, (uint32_t *)h->ring_oh[i].ptr,
		                              want_px ? (uint8_t *)h->ring_out[i].ptr : nullptr);
		if (rc == PXZ_OK && packed)
			rc = pxz_pack_tiles_device(h, (uint32_t)tiles, channels, (uint32_t)slot, (const uint32_t *)h->ring_ow[i].ptr,
			                           (const uint32_t *)h->ring_oh[i].ptr, (const uint8_t *)h->ring_out[i].ptr,
			                           (uint64_t *)h->ring_pkoff[i].ptr, (uint8_t *)h->ring_pk[i].ptr, most);
		if (rc == PXZ_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, PXZ_ERR_HIP, "hipStreamSynchronize failed");
		std::lock_guard<std::mutex> lk(m);
		if (rc != PXZ_OK) stop = true;
		else computed = k + 1;
		cv.notify_all();
	}
	{
		std::unique_lock<std::mutex> lk(m);
		cv.wait(lk, [&] { return stop || downloaded == n_images; });
		stop = true;  // (lets a helper that is still waiting go)
		cv.notify_all();
	}
	uploader.join();
	downloader.join();
	(void)hipStreamDestroy(up);
	(void)hipStreamDestroy(down);
	if (rc != PXZ_OK) return rc;
	if (copy_error != hipSuccess) return fail(h, PXZ_ERR_HIP, "host copy failed: %s", hipGetErrorString(copy_error));
	if (packed)
		for (uint32_t k = 0; k < n_images; ++k)
			if (packed_len[k] > capacity) return fail(h, PXZ_ERR_BUFFER_TOO_SMALL, "image %u: packed stream of %llu bytes, capacity %llu", k,
			                                          (unsigned long long)packed_len[k], (unsigned long long)capacity);
	return PXZ_OK;
}

int pxz_shrink_images(pxz_handle *h, const uint8_t *const *pixels, uint32_t n_images, uint32_t width, uint32_t height,
                      uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter,
                      float factor, float *const *block_value, uint32_t *const *out_w, uint32_t *const *out_h,
                      uint8_t *const *out_pixels)
{
	return shrink_images_impl(h, pixels, n_images, width, height, channels, pitch_bytes, block_w, block_h, mode, filter, factor,
	                          block_value, out_w, out_h, out_pixels, false, 0, nullptr);
}

int pxz_shrink_images_packed(pxz_handle *h, const uint8_t *const *pixels, uint32_t n_images, uint32_t width, uint32_t height,
                             uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode,
                             uint32_t filter, float factor, float *const *block_value, uint32_t *const *out_w,
                             uint32_t *const *out_h, uint8_t *const *packed, uint64_t packed_capacity, uint64_t *packed_len)
{
	return shrink_images_impl(h, pixels, n_images, width, height, channels, pitch_bytes, block_w, block_h, mode, filter, factor,
	                          block_value, out_w, out_h, packed, true, packed_capacity, packed_len);
}

int pxz_fetch_packed(pxz_handle *h, uint8_t *dst, uint64_t capacity)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!dst && h->packed_len != 0) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if (capacity < h->packed_len) return fail(h, PXZ_ERR_INVALID_ARG, "capacity %llu < packed length %llu",
	                                          (unsigned long long)capacity, (unsigned long long)h->packed_len);
	if (h->packed_len == 0) return PXZ_OK;
	PXZ_HIP(h, hipSetDevice(h->device));
	PXZ_HIP(h, hipMemcpyAsync(dst, h->pk.ptr, h->packed_len, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	return PXZ_OK;
}

int pxz_oklab_pixels_device(pxz_handle *h, const uint8_t *d_rgba, uint32_t n_pixels, float *d_laba)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!d_rgba || !d_laba || n_pixels == 0) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer / no pixels");
	if ((reinterpret_cast<uintptr_t>(d_rgba) & 3u) || (reinterpret_cast<uintptr_t>(d_laba) & 15u))
		return fail(h, PXZ_ERR_INVALID_ARG, "pixels must be 4-byte aligned, the output 16-byte aligned");
	PXZ_HIP(h, hipSetDevice(h->device));
	PXZ_HIP(h, pxz::launch_oklab_pixels(reinterpret_cast<const uint32_t *>(d_rgba), n_pixels, d_laba, h->n_cus, h->stream));
	return PXZ_OK;
}

int pxz_pack_tiles_device(pxz_handle *h, uint32_t n_tiles, uint32_t channels, uint32_t slot_bytes,
                          const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                          uint64_t *d_offsets, uint8_t *d_packed, uint64_t packed_capacity)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!d_tile_w || !d_tile_h || !d_slots || !d_offsets || !d_packed || n_tiles == 0)
		return fail(h, PXZ_ERR_INVALID_ARG, "null pointer / no tiles");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4");
	PXZ_HIP(h, hipSetDevice(h->device));
	const uint32_t n_chunks = (n_tiles + 4095u) / 4096u;
	if ((uint64_t)slot_bytes * 4096ull > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "slot too large for the chunked scan");
	int rc = ensure(h, h->chunks, (size_t)n_chunks * 8u);
	if (rc != PXZ_OK) return rc;
	pxz::PackArgs a{d_tile_w, d_tile_h, nullptr, d_slots, (unsigned long long *)d_offsets, (unsigned long long *)h->chunks.ptr,
	                d_packed, packed_capacity, n_tiles, n_chunks, channels, slot_bytes};
	PXZ_HIP(h, pxz::launch_pack(a, h->stream));
	return PXZ_OK;
}

}  // extern "C"

namespace {
// The writer's scratch (pxz_stream.hip) for n_tiles tiles of bw x bh pixels in c channels, and its limits: the scratch-
// derived part of *a -- slot_bytes, n_tiles, n_chunks; the encoder's units in qscratch; in qmeta perm | rec_len | bins as
// u32, then offsets (n + 1) and chunk totals as u64.
int writer_scratch(pxz_handle *h, uint32_t n_tiles, uint32_t bw, uint32_t bh, uint32_t c, pxz::QoiArgs *a)
{
	const uint64_t slot64 = (uint64_t)bw * bh * c;
	if (slot64 > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "tile too large");
	const uint32_t slot = (uint32_t)slot64;
	if ((slot & 15u) != 0 && c == 4) return fail(h, PXZ_ERR_UNSUPPORTED, "RGBA slots must be 16-byte multiples");
	// a record: 13 + 10 + at most (channels + 1) bytes per pixel + the 8-byte end marker; a chunk of the record scan holds 4096 of them
	const uint32_t px = bw * bh;
	const uint64_t stride = 23ull + (uint64_t)px * (c + 1u) + 8ull;
	if (stride * 4096ull > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "tile too large for the chunked scan");
	const uint32_t n_chunks = (n_tiles + 4095u) / 4096u;
	int rc = ensure(h, h->qscratch, pxz::qoi_scratch_bytes(n_tiles, px, c));
	if (rc != PXZ_OK) return rc;
	const size_t meta_u32 = (size_t)n_tiles * 2 + pxz::qoi_bins_dwords();
	const size_t meta_u32_bytes = (meta_u32 * 4 + 7) & ~(size_t)7;
	if ((rc = ensure_bins(h, h->qmeta, meta_u32_bytes + ((size_t)n_tiles + 1 + n_chunks) * 8, h->qbins_clean)) != PXZ_OK) return rc;
	uint32_t *m32 = (uint32_t *)h->qmeta.ptr;
	unsigned long long *m64 = (unsigned long long *)((uint8_t *)h->qmeta.ptr + meta_u32_bytes);
	a->perm = m32;
	a->rec_len = m32 + n_tiles;
	a->bins = m32 + 2 * (size_t)n_tiles;
	a->scratch = (uint8_t *)h->qscratch.ptr;
	a->offsets = m64;
	a->chunk_totals = m64 + n_tiles + 1;
	a->n_tiles = n_tiles;
	a->n_chunks = n_chunks;
	a->slot_bytes = slot;
	return PXZ_OK;
}
}  // namespace

extern "C" {

int pxz_encode_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, uint32_t filter_byte,
                             const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                             const uint8_t *d_slots, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !params || !d_block_value || !d_tile_w || !d_tile_h || !d_slots || !d_out || !d_file_offsets)
		return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if (frames->channels != 3 && frames->channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4");
	if (params->block_w == 0 || params->block_h == 0 || frames->n_frames == 0) return fail(h, PXZ_ERR_INVALID_ARG, "bad geometry");
	PXZ_HIP(h, hipSetDevice(h->device));
	if (frames->width > kMaxImageSide || frames->height > kMaxImageSide)
		return fail(h, PXZ_ERR_UNSUPPORTED, "image sides above 2^24 are not supported");
	Grid g;
	int rc = make_grid(h, frames->width, frames->height, params->block_w, params->block_h, frames->n_frames, 0xffffffffull, &g);
	if (rc != PXZ_OK) return rc;
	pxz::QoiArgs a{};
	if ((rc = writer_scratch(h, (uint32_t)g.tiles, params->block_w, params->block_h, frames->channels, &a)) != PXZ_OK) return rc;
	a.slots = d_slots;
	a.w = d_tile_w;
	a.h = d_tile_h;
	a.value = d_block_value;
	a.out = d_out;
	a.file_offsets = (unsigned long long *)d_file_offsets;
	a.capacity = out_capacity;
	a.tiles_per_frame = g.tiles_per_frame;
	a.cols = g.cols;
	a.rows = g.rows;
	a.channels = frames->channels;
	a.hdr_bytes = 26u + g.rows * 4u;
	a.width = frames->width;
	a.height = frames->height;
	a.bw = params->block_w;
	a.bh = params->block_h;
	a.filter_byte = filter_byte;
	return launch_on_bins(h, h->qbins_clean, a.bins, [&](bool bins_clean) { return pxz::launch_qoi(a, bins_clean, h->n_cus, h->stream); });
}

int pxz_synth_frames_device(pxz_handle *h, const pxz_frames *frames, uint8_t *d_pixels, uint32_t first_frame_index,
                            uint32_t dist)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !d_pixels || dist > 3) return fail(h, PXZ_ERR_INVALID_ARG, "bad synth arguments");
	if (frames->channels != 3 && frames->channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4");
	if (frames->height > 65535u || frames->n_frames > 65535u) return fail(h, PXZ_ERR_UNSUPPORTED, "frame too tall for the synth grid");
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::SynthArgs s{d_pixels,
	                 pxz::frame_stride_of(*frames),
	                 frames->pitch_bytes, frames->width, frames->height, frames->channels, frames->n_frames,
	                 first_frame_index, dist};
	PXZ_HIP(h, pxz::launch_synth(s, h->stream));
	return PXZ_OK;
}

int pxz_axis_table(uint32_t in_size, uint32_t out_size, uint32_t filter, int32_t *starts, int32_t *sizes,
                   int16_t *coeffs, int32_t *window, int32_t *precision)
{
	if (in_size == 0 || out_size == 0 || filter > 4) return PXZ_ERR_INVALID_ARG;
	pxz::AxisWindows w;
	if (!pxz::build_axis(in_size, out_size, filter, &w, out_size > in_size)) return PXZ_ERR_INVALID_ARG;
	if (window) *window = w.window;
	if (precision) *precision = w.precision;
	if (starts) std::memcpy(starts, w.starts.data(), sizeof(int32_t) * out_size);
	if (sizes) std::memcpy(sizes, w.sizes.data(), sizeof(int32_t) * out_size);
	if (coeffs && !w.coeffs.empty()) std::memcpy(coeffs, w.coeffs.data(), sizeof(int16_t) * w.coeffs.size());
	return PXZ_OK;
}

// diagnostic builds only: the stamps of expand_kernel (behind its status word)
int pxz_debug_read_status(pxz_handle *h, void *dst, size_t offset, size_t bytes)
{
	if (!h || !dst || !h->status.ptr || offset + bytes > h->status.cap) return PXZ_ERR_INVALID_ARG;
	PXZ_HIP(h, hipMemcpy(dst, (const uint8_t *)h->status.ptr + offset, bytes, hipMemcpyDeviceToHost));
	return PXZ_OK;
}

// diagnostic builds only: copy bytes out of the handle's worklist/stamp buffer
int pxz_debug_read_work(pxz_handle *h, void *dst, size_t offset, size_t bytes)
{
	if (!h || !dst || !h->work.ptr || offset + bytes > h->work.cap) return PXZ_ERR_INVALID_ARG;
	PXZ_HIP(h, hipMemcpy(dst, (const uint8_t *)h->work.ptr + offset, bytes, hipMemcpyDeviceToHost));
	return PXZ_OK;
}

int pxz_enable_timing(pxz_handle *h, int on)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	h->timing = on != 0;
	h->timing_stride = on > 1 ? (uint32_t)on : 1u;  // on = n > 1: every n-th step only (an event costs ~2 us of stream time)
	h->timing_count = 0;
	h->events_used = 0;
	return PXZ_OK;
}

// average over the recorded steps of the time from each step's first event to its last (first_kernel: to the event behind
// its first kernel)
static int recorded_ms(pxz_handle *h, bool first_kernel, float *ms)
{
	if (!h || !ms) return PXZ_ERR_INVALID_ARG;
	if (!h->timing || h->events_used == 0) return fail(h, PXZ_ERR_INVALID_ARG, "no timed launches recorded");
	PXZ_HIP(h, hipEventSynchronize(h->events[h->events_used - 1].second));
	double total = 0.0;
	for (size_t i = 0; i < h->events_used; ++i) {
		float t = 0.f;
		PXZ_HIP(h, hipEventElapsedTime(&t, h->events[i].first, first_kernel ? h->mid_events[i] : h->events[i].second));
		total += t;
	}
	*ms = (float)(total / (double)h->events_used);
	return PXZ_OK;
}

// average over the launches recorded since the last call (or since enable)
int pxz_last_kernel_ms(pxz_handle *h, float *ms)
{
	const int rc = recorded_ms(h, false, ms);
	if (rc == PXZ_OK) h->events_used = 0;
	return rc;
}

// the same for the FIRST kernel of each recorded step alone (shrink32/64/16_kernel, or oklab_kernel in shrink_by
// steps): what a per-kernel profile shows for it.  Call before pxz_last_kernel_ms (which resets the record).
int pxz_last_first_kernel_ms(pxz_handle *h, float *ms) { return recorded_ms(h, true, ms); }

int pxz_handle_state(pxz_handle *h, uint32_t state[4])
{
	if (!h || !state) return PXZ_ERR_INVALID_ARG;
	state[0] = h->host_stats ? const_cast<volatile uint32_t *>(h->host_stats)[0] : 0u;
	state[1] = h->host_stats ? const_cast<volatile uint32_t *>(h->host_stats)[1] : 0xffffffffu;
	state[2] = h->last_alpha_kernel;
	state[3] = h->last_alpha_first;
	return PXZ_OK;
}

}  // extern "C"

// ---- batches of differently sized images (pxz_varied.hip) --------------------------------------------------------------
namespace {

// the distinct tile sides a table set is built for, ascending
std::vector<uint32_t> unique_sides(std::vector<uint32_t> sides)
{
	std::sort(sides.begin(), sides.end());
	sides.erase(std::unique(sides.begin(), sides.end()), sides.end());
	return sides;
}

// one image of width x height and its grid as an entry of the per-image table (offset, tile0 and row0 are the caller's)
pxz::VariedImage varied_entry(uint32_t width, uint32_t height, uint32_t pitch, const Grid &g)
{
	pxz::VariedImage im{};
	im.width = width;
	im.height = height;
	im.pitch = pitch;
	im.cols = g.cols;
	im.rows = g.rows;
	im.edge_w = g.edge_w;
	im.edge_h = g.edge_h;
	im.hdr_bytes = 26u + 4u * g.rows;  // mod.rs:47-48
	return im;
}

}  // namespace

namespace pxz_runtime {

// The per-image table of a varied batch, checked image by image before anything is launched.  channels 0: geometry only
// (pxz_varied_layout, the writer), no pitch or tile-size rules.
int varied_plan(pxz_handle *h, const pxz_image_desc *d, uint32_t n, uint32_t bw, uint32_t bh, uint32_t channels, uint32_t mode,
                std::vector<pxz::VariedImage> *images, std::vector<uint32_t> *sides, uint32_t *n_rows)
{
	if (!d) return fail(h, PXZ_ERR_INVALID_ARG, "null image descriptors");
	if (n == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	if (bw == 0 || bh == 0) return fail(h, PXZ_ERR_INVALID_ARG, "zero block size");
	images->resize(n);
	std::vector<uint32_t> all = {bw, bh};
	uint64_t tiles = 0, rows_total = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const pxz_image_desc &g = d[i];
		if (g.reserved != 0) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: reserved field must be 0", i);
		if (g.width == 0 || g.height == 0) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: empty image (%ux%u)", i, g.width, g.height);
		if (g.width > kMaxImageSide || g.height > kMaxImageSide)
			return fail(h, PXZ_ERR_UNSUPPORTED, "image %u: image sides above 2^24 are not supported", i);
		if (channels && (uint64_t)g.pitch_bytes < (uint64_t)g.width * channels)
			return fail(h, PXZ_ERR_INVALID_ARG, "image %u: pitch smaller than a row", i);
		Grid grid;
		(void)make_grid(h, g.width, g.height, bw, bh, 1, kAnyTiles, &grid);
		pxz::VariedImage &im = (*images)[i];
		im = varied_entry(g.width, g.height, g.pitch_bytes, grid);
		im.offset = g.offset_bytes;
		if (channels && mode == PXZ_MODE_SHRINK_DIRECTIONALLY && (im.edge_w < 2 || im.edge_h < 2 || bw < 2 || bh < 2))
			return fail(h, PXZ_ERR_TILE_TOO_SMALL,
			            "image %u: directional detector needs tiles of at least 2x2 px (edge tile is %ux%u); the reference panics here", i,
			            im.edge_w, im.edge_h);
		im.tile0 = (uint32_t)tiles;
		im.row0 = (uint32_t)rows_total;
		tiles += grid.tiles;
		rows_total += im.rows;
		if (tiles > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "image %u: more than 2^32-1 tiles in the batch", i);
		all.push_back(im.edge_w);
		all.push_back(im.edge_h);
	}
	if (sides) *sides = unique_sides(std::move(all));
	if (n_rows) *n_rows = (uint32_t)rows_total;
	return PXZ_OK;
}

}  // namespace pxz_runtime

namespace {

// the per-image table -> handle scratch, through pinned staging that is reused once the previous copy out of it has run
int varied_upload(pxz_handle *h, const std::vector<pxz::VariedImage> &images, const pxz::VariedImage **d_images)
{
	const size_t bytes = images.size() * sizeof(pxz::VariedImage);
	int rc = ensure(h, h->varied, bytes);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, h->varied_images.send(images.data(), bytes, h->varied.ptr, h->stream));
	*d_images = (const pxz::VariedImage *)h->varied.ptr;
	return PXZ_OK;
}

int get_varied_tables(pxz_handle *h, uint32_t filter, const std::vector<uint32_t> &sides, const VariedTables **out)
{
	return cached_tables(h, h->varied_tables, std::make_pair(filter, sides), kTableCacheBound, [&](VariedTables &vt) {
		pxz::VariedTableSet s;
		if (!pxz::build_varied_tables(sides, filter, &s)) return fail(h, PXZ_ERR_INVALID_ARG, "unknown filter %u", filter);
		return upload_tables(h, {{s.dir, &vt.d_dir}, {s.starts, &vt.d_starts}, {s.sizes, &vt.d_sizes}, {s.coeffs, &vt.d_coeffs}}, &vt.mem);
	}, out);
}

// the shrink side of a flat tile space whoever owns its tiles: the block, the outputs, the tables and the thresholds (all that
// pxz_patch_windows_device fills of a VariedArgs: its owners are windows, its tile count theirs, its factor PatchArgs')
void varied_fill_shrink(pxz_handle *h, uint32_t channels, const pxz_params *params, const VariedTables *vt, float *d_block_value,
                        uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, pxz::VariedArgs *a)
{
	a->bw = params->block_w;
	a->bh = params->block_h;
	a->mode = params->mode;
	a->filter = params->filter;
	a->value = d_block_value;
	a->out_w = d_out_w;
	a->out_h = d_out_h;
	a->out_px = d_out_pixels;
	a->slot_bytes = params->block_w * params->block_h * channels;
	a->tile_bytes = (a->slot_bytes + 15u) & ~15u;
	a->dir = vt->d_dir;
	a->starts = vt->d_starts;
	a->sizes = vt->d_sizes;
	a->coeffs = vt->d_coeffs;
	std::memcpy(a->thresholds, h->thresholds, sizeof a->thresholds);
}

// what varied_kernel and varied_ladder_kernel are told about a planned batch (a->images is varied_upload's)
void varied_fill_args(pxz_handle *h, const std::vector<pxz::VariedImage> &images, uint32_t channels, const pxz_params *params,
                      const VariedTables *vt, const uint8_t *d_base, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                      uint8_t *d_out_pixels, pxz::VariedArgs *a)
{
	a->base = d_base;
	a->n_images = (uint32_t)images.size();
	a->n_tiles = varied_n_tiles(images);
	a->factor = params->factor;
	varied_fill_shrink(h, channels, params, vt, d_block_value, d_out_w, d_out_h, d_out_pixels, a);
}

// The varied writer behind both of its entry points, past their null checks.  pxz_encode_varied_frames_device: d_out and
// d_file_offsets given, d_record_bytes null.  pxz_record_bytes_varied_device: d_out null and no capacity -- the same launches,
// which then write the offsets alone -- and the record lengths out of the writer's scratch behind them.
int encode_varied(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels, const pxz_params *params,
                  uint32_t filter_byte, const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                  uint8_t *d_out, uint64_t out_capacity, uint64_t *d_file_offsets, uint32_t *d_record_bytes)
{
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4");
	std::vector<pxz::VariedImage> images;
	uint32_t n_rows = 0;
	int rc = varied_plan(h, descs, n_images, params->block_w, params->block_h, 0, 0, &images, nullptr, &n_rows);
	if (rc != PXZ_OK) return rc;
	const uint32_t n_tiles = varied_n_tiles(images), c = channels;
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::QoiArgs a{};
	if ((rc = writer_scratch(h, n_tiles, params->block_w, params->block_h, c, &a)) != PXZ_OK) return rc;
	pxz::VariedWriterArgs v{};
	if ((rc = varied_upload(h, images, &v.images)) != PXZ_OK) return rc;
	a.slots = d_slots;
	a.w = d_tile_w;
	a.h = d_tile_h;
	a.value = d_block_value;
	a.out = d_out;
	a.file_offsets = (unsigned long long *)d_file_offsets;
	a.capacity = out_capacity;
	// one "frame" of n_tiles tiles and no tile rows of its own: the splice puts record t at hdr_bytes + scan(t), and the
	// per-image headers come from varied_headers_kernel
	a.tiles_per_frame = n_tiles;
	a.cols = 0;
	a.rows = 0;
	a.channels = c;
	a.hdr_bytes = images[0].hdr_bytes;
	a.bw = params->block_w;
	a.bh = params->block_h;
	a.filter_byte = filter_byte;
	v.n_images = n_images;
	v.n_tiles = n_tiles;
	v.n_rows = n_rows;
	v.bw = params->block_w;
	v.bh = params->block_h;
	v.filter_byte = filter_byte;
	v.rec_len = a.rec_len;
	v.offsets = a.offsets;
	v.chunk_totals = a.chunk_totals;
	v.out = d_out;
	v.file_offsets = a.file_offsets;
	v.capacity = out_capacity;
	if (!d_out) {
		// pxz_record_bytes_varied_device: no room, so no byte of a file is written -- the pointer only has to be one
		a.out = v.out = a.scratch;
		if (!d_file_offsets) {
			if ((rc = ensure(h, h->record_offsets, ((size_t)n_images + 1u) * 8u)) != PXZ_OK) return rc;
			a.file_offsets = v.file_offsets = (unsigned long long *)h->record_offsets.ptr;
		}
	}
	if ((rc = launch_on_bins(h, h->qbins_clean, a.bins,
	                         [&](bool bins_clean) { return pxz::launch_qoi_varied(a, v, bins_clean, h->n_cus, h->stream); })) != PXZ_OK)
		return rc;
	if (!d_record_bytes) return PXZ_OK;
	// (the per-image table is still where varied_upload put it: nothing has been uploaded over it since)
	const pxz::RecordBytesArgs rb{v.images, n_images, n_tiles, a.rec_len, d_record_bytes};
	PXZ_HIP(h, pxz::launch_record_bytes(rb, h->stream));
	return PXZ_OK;
}

}  // namespace

extern "C" {

int pxz_varied_layout(const pxz_image_desc *descs, uint32_t n_images, uint32_t block_w, uint32_t block_h, uint64_t *tile_offsets)
{
	if (!tile_offsets) return PXZ_ERR_INVALID_ARG;
	std::vector<pxz::VariedImage> images;
	const int rc = varied_plan(nullptr, descs, n_images, block_w, block_h, 0, 0, &images, nullptr, nullptr);
	if (rc != PXZ_OK) return rc;
	for (uint32_t i = 0; i < n_images; ++i) tile_offsets[i] = images[i].tile0;
	tile_offsets[n_images] = varied_n_tiles(images);
	return PXZ_OK;
}

int pxz_shrink_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, const uint8_t *d_base, float *d_block_value, uint32_t *d_out_w,
                                    uint32_t *d_out_h, uint8_t *d_out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_base || !d_block_value || !d_out_w || !d_out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	int rc = varied_check_params(h, channels, params);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	std::vector<uint32_t> sides;
	if ((rc = varied_plan(h, descs, n_images, params->block_w, params->block_h, channels, params->mode, &images, &sides, nullptr)) != PXZ_OK)
		return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	const VariedTables *vt = nullptr;
	if ((rc = get_varied_tables(h, params->filter, sides, &vt)) != PXZ_OK) return rc;
	pxz::VariedArgs a{};
	if ((rc = varied_upload(h, images, &a.images)) != PXZ_OK) return rc;
	varied_fill_args(h, images, channels, params, vt, d_base, d_block_value, d_out_w, d_out_h, d_out_pixels, &a);
	PXZ_HIP(h, pxz::launch_varied(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

int pxz_shrink_varied_ladder_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                           const pxz_params *params, const float *factors, uint32_t n_factors,
                                           const uint8_t *d_base, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                           uint8_t *d_out_pixels)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!d_base || !d_block_value || !d_out_w || !d_out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	pxz_params p = *params;
	p.factor = 1.0f;  // (a rung's factor enters nothing but its level)
	if ((rc = varied_check_params(h, channels, &p)) != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	std::vector<uint32_t> sides;
	if ((rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, channels, p.mode, &images, &sides, nullptr)) != PXZ_OK) return rc;
	if ((uint64_t)n_factors * varied_n_tiles(images) > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	// (cannot happen within the tile limit above; the kernel's own layout has the last word)
	if (pxz::varied_ladder_lds_limit_bytes(p.mode, p.block_w, p.block_h, channels) > 160u * 1024u)
		return fail(h, PXZ_ERR_UNSUPPORTED, "a %ux%u tile and its resampled images do not fit in LDS", p.block_w, p.block_h);
	PXZ_HIP(h, hipSetDevice(h->device));
	const VariedTables *vt = nullptr;
	if ((rc = get_varied_tables(h, p.filter, sides, &vt)) != PXZ_OK) return rc;
	pxz::VariedLadderArgs a{};
	if ((rc = varied_upload(h, images, &a.v.images)) != PXZ_OK) return rc;
	varied_fill_args(h, images, channels, &p, vt, d_base, d_block_value, d_out_w, d_out_h, d_out_pixels, &a.v);
	a.n_factors = n_factors;
	std::memcpy(a.factors, factors, n_factors * sizeof(float));
	PXZ_HIP(h, pxz::launch_varied_ladder(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

int pxz_encode_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, uint32_t filter_byte, const float *d_block_value,
                                    const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_out,
                                    uint64_t out_capacity, uint64_t *d_file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params || !d_block_value || !d_tile_w || !d_tile_h || !d_slots || !d_out || !d_file_offsets)
		return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	return encode_varied(h, descs, n_images, channels, params, filter_byte, d_block_value, d_tile_w, d_tile_h, d_slots, d_out, out_capacity,
	                     d_file_offsets, nullptr);
}

int pxz_record_bytes_varied_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                   const pxz_params *params, const float *d_block_value, const uint32_t *d_tile_w,
                                   const uint32_t *d_tile_h, const uint8_t *d_slots, uint32_t *d_record_bytes, uint64_t *d_file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params || !d_block_value || !d_tile_w || !d_tile_h || !d_slots || !d_record_bytes) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	return encode_varied(h, descs, n_images, channels, params, 0, d_block_value, d_tile_w, d_tile_h, d_slots, nullptr, 0, d_file_offsets, d_record_bytes);
}

}  // extern "C"

// ---- decode side of varied batches (varied_index_kernel in pxz_stream.hip, pxz_varied_expand.hip) -------------------------
namespace {

// a wave's image of tile_dw dwords, with the images' first tiles beside it, exceeds LDS
bool varied_image_beyond_lds(uint32_t tile_dw) { return (uint64_t)tile_dw * 4u + 8192u > 160u * 1024u; }
// dwords of one staged window for tables whose widest window has max_window taps
uint32_t varied_window_dw(uint32_t max_window) { return 1u + (max_window + 1u) / 2u; }

// lds_bw x lds_bh (0: no such limit): the block of a caller whose wave's image has to fit LDS; a set that does not let it is
// refused once it is built, before anything is uploaded or cached
int get_varied_expand_tables(pxz_handle *h, uint32_t filter, const std::vector<uint32_t> &sides, const VariedExpandTables **out,
                             uint32_t lds_bw = 0, uint32_t lds_bh = 0)
{
	return cached_tables(h, h->varied_expand_tables, std::make_pair(filter, sides), kTableCacheBound, [&](VariedExpandTables &vt) {
		pxz::VariedExpandTableSet s;
		if (!pxz::build_varied_expand_tables(sides, filter, &s)) return fail(h, PXZ_ERR_INVALID_ARG, "unknown filter %u", filter);
		if (lds_bw && varied_image_beyond_lds(pxz::varied_expand_tile_dw(lds_bw, lds_bh, varied_window_dw(s.max_window))))
			return fail(h, PXZ_ERR_UNSUPPORTED, "a wave keeps a %ux%u tile and its windows in LDS: they exceed what a block has", lds_bw, lds_bh);
		vt.stride = s.stride;
		vt.max_window = s.max_window;
		return upload_tables(h, {{s.slot, &vt.d_slot}, {s.dir, &vt.d_dir}, {s.starts, &vt.d_starts}, {s.sizes, &vt.d_sizes}, {s.coeffs, &vt.d_coeffs}}, &vt.mem);
	}, out);
}

// where the per-image flags of a varied decode-side call go: the caller's array, or handle scratch when it passed none; zeroed
int varied_flags(pxz_handle *h, uint32_t *d_image_flags, uint32_t n_images, uint32_t **out)
{
	if (!d_image_flags) {
		const int rc = ensure(h, h->varied_flags, (size_t)n_images * 4u);
		if (rc != PXZ_OK) return rc;
		d_image_flags = (uint32_t *)h->varied_flags.ptr;
	}
	PXZ_HIP(h, hipMemsetAsync(d_image_flags, 0, (size_t)n_images * 4u, h->stream));
	*out = d_image_flags;
	return PXZ_OK;
}

// the optional per-owner flags of an expand-side call (null: the caller wants none), zeroed on the stream
int zero_owner_flags(pxz_handle *h, uint32_t *d_flags, size_t n_owners)
{
	if (d_flags) PXZ_HIP(h, hipMemsetAsync(d_flags, 0, n_owners * 4u, h->stream));
	return PXZ_OK;
}

// What the kernels that resize stored tiles of a flat tile space back to their full sizes share (TileResizeArgs): the block,
// the tables of the call's tile sides, and the LDS image of one wave.  lds_only: the caller's kernel has no HBM form, and a
// wave's image beyond LDS is refused -- when the set is built, and for a cached set that a caller with another block of the
// same sides left.
template <class Args>  // TileResizeArgs, or DistortionArgs (which names the same fields)
int put_varied_expand_tables(pxz_handle *h, const pxz_params &p, uint32_t channels, const std::vector<uint32_t> &sides, Args *a,
                             bool lds_only = false)
{
	const VariedExpandTables *vt = nullptr;
	const int rc = get_varied_expand_tables(h, p.filter, sides, &vt, lds_only ? p.block_w : 0u, lds_only ? p.block_h : 0u);
	if (rc != PXZ_OK) return rc;
	a->bw = p.block_w;
	a->bh = p.block_h;
	a->slot_bytes = p.block_w * p.block_h * channels;
	a->filter = p.filter;
	a->slot = vt->d_slot;
	a->dir = vt->d_dir;
	a->stride = vt->stride;
	a->starts = vt->d_starts;
	a->sizes = vt->d_sizes;
	a->coeffs = vt->d_coeffs;
	a->wdw = varied_window_dw(vt->max_window);
	a->tile_dw = pxz::varied_expand_tile_dw(a->bw, a->bh, a->wdw);
	if (lds_only && varied_image_beyond_lds(a->tile_dw))
		return fail(h, PXZ_ERR_UNSUPPORTED, "a wave keeps a %ux%u tile of %u channels and its windows in LDS: %llu bytes exceed what a block has", a->bw,
		            a->bh, channels, (unsigned long long)a->tile_dw * 4u);
	return PXZ_OK;
}

// the decode side's status word, zeroed on the stream
int fresh_status(pxz_handle *h, uint32_t **status)
{
	const int rc = ensure(h, h->status, 256);
	if (rc != PXZ_OK) return rc;
	*status = (uint32_t *)h->status.ptr;
	PXZ_HIP(h, hipMemsetAsync(*status, 0, 8, h->stream));
	return PXZ_OK;
}

// what every expand-side launch is given to report into: the status word and the optional per-owner flags, both zeroed on the
// stream in this order; *flags_arg is the launch's field for the flags
int fresh_status_and_flags(pxz_handle *h, uint32_t **status, uint32_t *d_flags, size_t n_owners, uint32_t **flags_arg)
{
	int rc = fresh_status(h, status);
	if (rc == PXZ_OK) rc = zero_owner_flags(h, d_flags, n_owners);
	*flags_arg = d_flags;
	return rc;
}

// the stored tiles a launch reads: their count, stored sizes and slots
struct StoredTiles {
	const uint32_t *w, *h;
	const uint8_t *slots;
};
template <class Args>  // TileResizeArgs, or a struct that names the same fields
void put_stored_tiles(Args *a, uint32_t n_tiles, const StoredTiles &tiles)
{
	a->n_tiles = n_tiles;
	a->tile_w = tiles.w;
	a->tile_h = tiles.h;
	a->slots = tiles.slots;
}

// The reader's arguments for a flat tile space of n_tiles tiles over n_images files: one "frame" of n_tiles tiles, no
// geometry of its own (every image, or every window, carries its own).  Sets the device and carves the reader's scratch.
int flat_decode_args(pxz_handle *h, const pxz_params &p, uint32_t channels, uint32_t n_images, uint32_t n_tiles, const uint8_t *d_files,
                     const uint64_t *d_file_offsets, float *d_block_value, uint32_t *d_tile_w, uint32_t *d_tile_h, uint8_t *d_slots,
                     pxz::DecodeArgs *a)
{
	if ((uint64_t)p.block_w * p.block_h * channels > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "tile too large");
	PXZ_HIP(h, hipSetDevice(h->device));
	a->files = d_files;
	a->file_offsets = reinterpret_cast<const unsigned long long *>(d_file_offsets);
	a->value = d_block_value;
	a->tile_w = d_tile_w;
	a->tile_h = d_tile_h;
	a->slots = d_slots;
	a->bw = p.block_w;
	a->bh = p.block_h;
	a->n_frames = n_images;  // (the end of the files buffer)
	a->n_tiles = n_tiles;
	a->tiles_per_frame = n_tiles;
	a->channels = channels;
	a->slot_bytes = p.block_w * p.block_h * channels;
	return reader_scratch(h, a);
}

}  // namespace

extern "C" {

int pxz_decode_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, const uint8_t *d_files, const uint64_t *d_file_offsets,
                                    float *d_block_value, uint32_t *d_tile_w, uint32_t *d_tile_h, uint8_t *d_slots,
                                    uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_files || !d_file_offsets || !d_block_value || !d_tile_w || !d_tile_h || !d_slots)
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	const pxz_params p = decode_side_params(params, false);
	std::vector<pxz::VariedImage> images;
	uint32_t n_rows = 0;
	int rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, 0, 0, &images, nullptr, &n_rows);
	if (rc != PXZ_OK) return rc;
	pxz::DecodeArgs a{};
	if ((rc = flat_decode_args(h, p, channels, n_images, varied_n_tiles(images), d_files, d_file_offsets, d_block_value, d_tile_w, d_tile_h, d_slots,
	                           &a)) != PXZ_OK)
		return rc;
	uint32_t *flags = nullptr;
	if ((rc = varied_flags(h, d_image_flags, n_images, &flags)) != PXZ_OK) return rc;
	const pxz::VariedImage *d_images = nullptr;
	if ((rc = varied_upload(h, images, &d_images)) != PXZ_OK) return rc;
	return launch_on_bins(h, h->dbins_clean, a.bins,
	                      [&](bool bins_clean) { return pxz::launch_decode_varied(a, d_images, n_rows, flags, bins_clean, h->stream); });
}

int pxz_expand_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                    const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_tile_w || !d_tile_h || !d_slots || !d_base) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	std::vector<uint32_t> sides;
	if ((rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, channels, 0, &images, &sides, nullptr)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::VariedExpandArgs a{};
	if ((rc = put_varied_expand_tables(h, p, channels, sides, &a)) != PXZ_OK) return rc;
	a.n_images = n_images;
	put_stored_tiles(&a, varied_n_tiles(images), {d_tile_w, d_tile_h, d_slots});
	a.base = d_base;
	// a wave's image beyond LDS (with the images' first tiles beside it) lives in HBM, one per wave of the grid
	if (varied_image_beyond_lds(a.tile_dw)) {
		const uint64_t waves = 4ull * h->n_cus;
		if ((rc = ensure(h, h->bigscratch, (size_t)waves * a.tile_dw * 4u)) != PXZ_OK) return rc;
		a.big_scratch = (uint32_t *)h->bigscratch.ptr;
		a.big_waves = (uint32_t)waves;
	}
	if ((rc = fresh_status_and_flags(h, &a.status, d_image_flags, n_images, &a.image_flags)) != PXZ_OK) return rc;
	if ((rc = varied_upload(h, images, &a.images)) != PXZ_OK) return rc;
	PXZ_HIP(h, pxz::launch_varied_expand(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

}  // extern "C"

// ---- the archive calls: stored tiles in, stored tiles out.  Re-shrink (pxz_reshrink.hip, pxz_reshrink_ladder.hip): the reference
// CLI's pix_to_pix (src/bin/main.rs:233-265); re-tile (pxz_retile.hip, pxz_retile_ladder.hip): pix_to_pix with -b, a block size
// that changes; their distortions stand further down, behind the fit.  DESIGN.md 8u has the shape of this path. -------------
namespace {

// one table set of a size query: the expand tables of `filter` for a block alone (no edges: a query knows of no image)
struct BlockTables {
	uint32_t bw, bh, filter;
};

// The size query of an archive kernel: its footprint with windows of 1 dword -- beyond the limit then, it is beyond it whatever
// the windows take -- else with the real windows of its tables (set: the distortions' second table set, else null).
template <class Footprint>
int archive_lds_query(const Footprint &bytes, const BlockTables &expand, const BlockTables *set, uint32_t *lds_bytes)
{
	uint64_t v = bytes(1u, 1u);
	if (v <= kLdsPerCu) {
		const BlockTables *const of[2] = {&expand, set};
		uint32_t wdw[2] = {1u, 1u};
		for (int k = 0; k < 2 && of[k]; ++k) {
			pxz::VariedExpandTableSet s;
			if (!pxz::build_varied_expand_tables(unique_sides({of[k]->bw, of[k]->bh}), of[k]->filter, &s)) return PXZ_ERR_INVALID_ARG;
			wdw[k] = varied_window_dw(s.max_window);
		}
		v = bytes(wdw[0], wdw[1]);
	}
	*lds_bytes = (uint32_t)std::min<uint64_t>(v, 0xffffffffull);
	return PXZ_OK;
}

// what every archive call is handed about its batch
struct ArchiveBatch {
	const pxz_image_desc *descs;
	uint32_t n_images, channels;
	bool retile;               // the stored tiles that come in have a block of their own:
	uint32_t src_bw, src_bh;   //   theirs (not read otherwise: they have params')
	const pxz_params *params;  // the block of what goes out (a distortion: of the sets)
	uint32_t expand_filter;
};

// A planned archive batch: its images in the layout of params' block (the destination: what goes out, or the sets) and, for a
// re-tile, in the layout of the source block (the stored tiles that come in).
struct ArchivePlan {
	std::vector<pxz::VariedImage> images, src_images;
	std::vector<uint32_t> sides, src_sides;
	bool retile = false;
	// the layout of the stored tiles that come in
	const std::vector<uint32_t> &in_sides() const { return retile ? src_sides : sides; }
	uint32_t n_tiles() const { return varied_n_tiles(images); }
	uint32_t n_in_tiles() const { return varied_n_tiles(retile ? src_images : images); }
};

// The planning step of every archive call, from the check of the descriptors on: the layouts for p's block and mode (p: the
// call's params as it reads them) and for the source block, and the rule that n_sets (rungs or sets: `noun`) of the
// destination's tiles can be counted.
int archive_plan(pxz_handle *h, const ArchiveBatch &b, const pxz_params &p, uint32_t n_sets, const char *noun, ArchivePlan *plan)
{
	if (!b.descs) return fail(h, PXZ_ERR_INVALID_ARG, "null image descriptors");
	if (b.n_images == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	// (of an image only its size is read, and that reserved is 0: stored tiles have no pitch and no place)
	std::vector<pxz_image_desc> sized(b.n_images);
	for (uint32_t i = 0; i < b.n_images; ++i)
		sized[i] = pxz_image_desc{b.descs[i].width, b.descs[i].height, b.descs[i].width * b.channels, b.descs[i].reserved, 0};
	plan->retile = b.retile;
	int rc = varied_plan(h, sized.data(), b.n_images, p.block_w, p.block_h, b.channels, p.mode, &plan->images, &plan->sides, nullptr);
	if (rc != PXZ_OK) return rc;
	if (b.retile && (rc = varied_plan(h, sized.data(), b.n_images, b.src_bw, b.src_bh, 0, 0, &plan->src_images, &plan->src_sides, nullptr)) != PXZ_OK)
		return rc;
	if ((uint64_t)n_sets * plan->n_tiles() > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u %s", n_sets, noun);
	return PXZ_OK;
}

// the per-image tables of a plan in ONE upload: the destination layout's, then (re-tile) the source layout's behind it
int archive_upload(pxz_handle *h, const ArchivePlan &plan, const pxz::VariedImage **d_images, const pxz::VariedImage **d_src_images)
{
	*d_src_images = nullptr;
	if (!plan.retile) return varied_upload(h, plan.images, d_images);
	std::vector<pxz::VariedImage> both = plan.images;
	both.insert(both.end(), plan.src_images.begin(), plan.src_images.end());
	const int rc = varied_upload(h, both, d_images);
	if (rc == PXZ_OK) *d_src_images = *d_images + plan.images.size();
	return rc;
}

// the expand side of an archive call: the geometry and filter the stored tiles that come in are expanded with
pxz_params archive_expand_params(const ArchiveBatch &b, const pxz_params &p)
{
	pxz_params xp = p;
	if (b.retile) {
		xp.block_w = b.src_bw;
		xp.block_h = b.src_bh;
	}
	xp.filter = b.expand_filter;
	return xp;
}

// Two expand table sets for one launch: r for (xp, r_sides), u for (p, u_sides).
// Both sets live in one bounded cache, and a set that is built into a full cache empties it first: r's set may have gone
// with it.  Asked for again it is found, or built into a cache that holds the sets' tables alone -- both stay.  (Sets of one
// filter and the same sides are one set: nothing to ask again.)
int put_both_expand_tables(pxz_handle *h, uint32_t channels, const pxz_params &xp, const std::vector<uint32_t> &r_sides, const pxz_params &p,
                           const std::vector<uint32_t> &u_sides, pxz::TileResizeArgs *r, pxz::TileResizeArgs *u)
{
	int rc = put_varied_expand_tables(h, xp, channels, r_sides, r);
	if (rc == PXZ_OK) rc = put_varied_expand_tables(h, p, channels, u_sides, u);
	if (rc == PXZ_OK && (xp.filter != p.filter || r_sides != u_sides)) rc = put_varied_expand_tables(h, xp, channels, r_sides, r);
	return rc;
}

// The four tile-to-tile calls behind one body, from the check of the device pointers on (h, params and the ladder's factors are
// checked by the entry points).  b.retile: re-tile, else re-shrink; factors == nullptr: the one-factor call (params->factor;
// n_factors is not read), else the ladder (n_factors rungs, outputs rung-major in the destination layout).  LadderArgs is the
// ladder's struct of the family; the one-factor call launches its .r.  admit(wdw): the family's footprint against LDS under
// its own text; launch(la, d_src_images): the family's launch (the source layout's table is a field of the re-tile alone).
//
// Two things differ between the families without a reason that this file knows; they are inherited, and decided here only:
//  - the re-tile holds its block against the varied calls' rule (varied_check_params: block_w*block_h*channels within 64 KB),
//    the re-shrink does not.  The rule refuses nothing that the footprints admit (both keep a plane of block_w*block_h dwords
//    within 64 KB: kRetileMaxPlaneBytes, kReshrinkMaxPlaneBytes), so what it changes is the text, and that it is reported
//    before a zero source block or a bad expand_filter.
//  - v.tile_bytes is one plane of dwords in every call but the re-shrink ladder, which keeps varied_fill_args' value.  Of the
//    kernels launched from here reshrink_kernel alone reads the field.
template <class LadderArgs, class Admit, class Launch>
int archive_resize(pxz_handle *h, const ArchiveBatch &b, const float *factors, uint32_t n_factors, const StoredTiles &in, float *d_block_value,
                   uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags, Admit admit, Launch launch)
{
	if (!in.w || !in.h || !in.slots || !d_block_value || !d_out_w || !d_out_h) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	const bool ladder = factors != nullptr;
	pxz_params p = *b.params;
	if (ladder) p.factor = 1.0f;  // (a rung's factor enters nothing but its level)
	int rc;
	if (b.retile) {
		if ((rc = varied_check_params(h, b.channels, &p)) != PXZ_OK) return rc;
		if (b.src_bw == 0 || b.src_bh == 0) return fail(h, PXZ_ERR_INVALID_ARG, "zero source block size");
	} else {
		if (b.channels != 3 && b.channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", b.channels);
		if ((rc = check_params(h, &p)) != PXZ_OK) return rc;
	}
	if (b.expand_filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "expand_filter must be 0..4, got %u", b.expand_filter);
	if ((rc = admit(1u)) != PXZ_OK) return rc;
	ArchivePlan plan;
	if ((rc = archive_plan(h, b, p, ladder ? n_factors : 1u, "rungs", &plan)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	const VariedTables *vt = nullptr;
	if ((rc = get_varied_tables(h, p.filter, plan.sides, &vt)) != PXZ_OK) return rc;
	LadderArgs la{};
	auto &a = la.r;
	if ((rc = put_varied_expand_tables(h, archive_expand_params(b, p), b.channels, plan.in_sides(), &a.x)) != PXZ_OK) return rc;
	if ((rc = admit(a.x.wdw)) != PXZ_OK) return rc;
	if ((rc = fresh_status_and_flags(h, &a.x.status, d_image_flags, b.n_images, &a.image_flags)) != PXZ_OK) return rc;
	const pxz::VariedImage *d_src_images = nullptr;
	if ((rc = archive_upload(h, plan, &a.v.images, &d_src_images)) != PXZ_OK) return rc;
	varied_fill_args(h, plan.images, b.channels, &p, vt, nullptr, d_block_value, d_out_w, d_out_h, d_out_pixels, &a.v);
	if (b.retile || !ladder) a.v.tile_bytes = (p.block_w * p.block_h * 4u + 15u) & ~15u;  // one plane: a dword per pixel while the tile is put together
	put_stored_tiles(&a.x, plan.n_in_tiles(), in);
	if (ladder) {
		la.n_factors = n_factors;
		std::memcpy(la.factors, factors, n_factors * sizeof(float));
	}
	return launch(la, d_src_images);
}

int reshrink_varied(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels, const pxz_params *params,
                    uint32_t expand_filter, const float *factors, uint32_t n_factors, const StoredTiles &in, float *d_block_value, uint32_t *d_out_w,
                    uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	const ArchiveBatch b{descs, n_images, channels, false, 0u, 0u, params, expand_filter};
	return archive_resize<pxz::ReshrinkLadderArgs>(
	    h, b, factors, n_factors, in, d_block_value, d_out_w, d_out_h, d_out_pixels, d_image_flags,
	    [&](uint32_t wdw) { return reshrink_check_block(h, params->mode, params->block_w, params->block_h, factors ? channels : 0u, wdw); },
	    [&](const pxz::ReshrinkLadderArgs &a, const pxz::VariedImage *) {
		    if (factors) PXZ_HIP(h, pxz::launch_reshrink_ladder(a, channels, h->n_cus, h->stream));
		    else PXZ_HIP(h, pxz::launch_reshrink(a.r, channels, h->n_cus, h->stream));
		    return (int)PXZ_OK;
	    });
}

int retile_varied(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels, uint32_t src_block_w, uint32_t src_block_h,
                  const pxz_params *params, uint32_t expand_filter, const float *factors, uint32_t n_factors, const StoredTiles &in,
                  float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	const ArchiveBatch b{descs, n_images, channels, true, src_block_w, src_block_h, params, expand_filter};
	return archive_resize<pxz::RetileLadderArgs>(
	    h, b, factors, n_factors, in, d_block_value, d_out_w, d_out_h, d_out_pixels, d_image_flags,
	    [&](uint32_t wdw) {
		    if (beyond_lds(retile_footprint(params->mode, src_block_w, src_block_h, params->block_w, params->block_h, factors ? channels : 0u), wdw))
			    return fail(h, PXZ_ERR_UNSUPPORTED,
			                "a re-tile keeps a %ux%u tile image (a dword per pixel), the staged parts of %ux%u source tiles and the source windows in LDS: "
			                "they exceed a block's 160 KB (%s)", params->block_w, params->block_h, src_block_w, src_block_h,
			                factors ? "pxz_retile_ladder_lds_bytes" : "pxz_retile_lds_bytes");
		    return (int)PXZ_OK;
	    },
	    [&](pxz::RetileLadderArgs &la, const pxz::VariedImage *d_src_images) {
		    pxz::RetileArgs &a = la.r;
		    a.src_images = d_src_images;
		    if (factors) PXZ_HIP(h, pxz::launch_retile_ladder(la, channels, h->n_cus, h->stream));
		    else PXZ_HIP(h, pxz::launch_retile(a, channels, h->n_cus, h->stream));
		    return (int)PXZ_OK;
	    });
}

}  // namespace

extern "C" {

int pxz_reshrink_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t expand_filter, uint32_t *lds_bytes)
{
	if (!lds_bytes || block_w == 0 || block_h == 0 || mode > 1 || expand_filter > 4) return PXZ_ERR_INVALID_ARG;
	return archive_lds_query(reshrink_footprint(mode, block_w, block_h, 0u), {block_w, block_h, expand_filter}, nullptr, lds_bytes);
}

int pxz_reshrink_ladder_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t mode, uint32_t expand_filter,
                                  uint32_t *lds_bytes)
{
	if (!lds_bytes || block_w == 0 || block_h == 0 || (channels != 3 && channels != 4) || mode > 1 || expand_filter > 4) return PXZ_ERR_INVALID_ARG;
	return archive_lds_query(reshrink_footprint(mode, block_w, block_h, channels), {block_w, block_h, expand_filter}, nullptr, lds_bytes);
}

int pxz_reshrink_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                      const pxz_params *params, uint32_t expand_filter, const uint32_t *d_tile_w,
                                      const uint32_t *d_tile_h, const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w,
                                      uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	return reshrink_varied(h, descs, n_images, channels, params, expand_filter, nullptr, 0u, {d_tile_w, d_tile_h, d_slots}, d_block_value, d_out_w,
	                       d_out_h, d_out_pixels, d_image_flags);
}

int pxz_reshrink_varied_ladder_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                             const pxz_params *params, uint32_t expand_filter, const float *factors,
                                             uint32_t n_factors, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                             const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                             uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	const int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	return reshrink_varied(h, descs, n_images, channels, params, expand_filter, factors, n_factors, {d_tile_w, d_tile_h, d_slots}, d_block_value,
	                       d_out_w, d_out_h, d_out_pixels, d_image_flags);
}

int pxz_retile_lds_bytes(uint32_t src_block_w, uint32_t src_block_h, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t expand_filter,
                         uint32_t *lds_bytes)
{
	if (!lds_bytes || src_block_w == 0 || src_block_h == 0 || block_w == 0 || block_h == 0 || mode > 1 || expand_filter > 4)
		return PXZ_ERR_INVALID_ARG;
	return archive_lds_query(retile_footprint(mode, src_block_w, src_block_h, block_w, block_h, 0u), {src_block_w, src_block_h, expand_filter}, nullptr,
	                         lds_bytes);
}

int pxz_retile_ladder_lds_bytes(uint32_t src_block_w, uint32_t src_block_h, uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t mode,
                                uint32_t expand_filter, uint32_t *lds_bytes)
{
	if (!lds_bytes || src_block_w == 0 || src_block_h == 0 || block_w == 0 || block_h == 0 || (channels != 3 && channels != 4) || mode > 1 ||
	    expand_filter > 4)
		return PXZ_ERR_INVALID_ARG;
	return archive_lds_query(retile_footprint(mode, src_block_w, src_block_h, block_w, block_h, channels), {src_block_w, src_block_h, expand_filter},
	                         nullptr, lds_bytes);
}

int pxz_retile_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    uint32_t src_block_w, uint32_t src_block_h, const pxz_params *params, uint32_t expand_filter,
                                    const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, float *d_block_value,
                                    uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	return retile_varied(h, descs, n_images, channels, src_block_w, src_block_h, params, expand_filter, nullptr, 0u, {d_tile_w, d_tile_h, d_slots},
	                     d_block_value, d_out_w, d_out_h, d_out_pixels, d_image_flags);
}

int pxz_retile_varied_ladder_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                           uint32_t src_block_w, uint32_t src_block_h, const pxz_params *params, uint32_t expand_filter,
                                           const float *factors, uint32_t n_factors, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                           const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                           uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	const int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	return retile_varied(h, descs, n_images, channels, src_block_w, src_block_h, params, expand_filter, factors, n_factors,
	                     {d_tile_w, d_tile_h, d_slots}, d_block_value, d_out_w, d_out_h, d_out_pixels, d_image_flags);
}

}  // extern "C"

// ---- rate and distortion (pxz_distortion.hip) -----------------------------------------------------------------------------
namespace {

// Both distortion calls behind their checks: a planned flat tile space (a varied batch, or n_frames equal entries), n_sets
// stored versions of its tiles.  One table copy, three memsets and one launch, whatever the batch holds.
int distortion_launch(pxz_handle *h, const std::vector<pxz::VariedImage> &images, const std::vector<uint32_t> &sides, uint32_t channels,
                      const pxz_params &p, uint32_t n_sets, const uint8_t *d_base, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                      const uint8_t *d_slots, uint64_t *d_tile_sse, uint64_t *d_image_sse, uint32_t *d_image_flags)
{
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::DistortionArgs a{};
	int rc = put_varied_expand_tables(h, p, channels, sides, &a, true);
	if (rc != PXZ_OK) return rc;
	a.n_images = (uint32_t)images.size();
	a.n_sets = n_sets;
	put_stored_tiles(&a, varied_n_tiles(images), {d_tile_w, d_tile_h, d_slots});
	a.base = d_base;
	a.tile_sse = reinterpret_cast<unsigned long long *>(d_tile_sse);
	a.image_sse = reinterpret_cast<unsigned long long *>(d_image_sse);
	if ((rc = fresh_status_and_flags(h, &a.status, d_image_flags, images.size(), &a.image_flags)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipMemsetAsync(d_image_sse, 0, (size_t)n_sets * images.size() * channels * 8u, h->stream));
	if ((rc = varied_upload(h, images, &a.images)) != PXZ_OK) return rc;
	PXZ_HIP(h, pxz::launch_distortion(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

}  // namespace

extern "C" {

int pxz_distortion_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, uint32_t n_sets,
                                 const uint8_t *d_pixels, const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                                 uint64_t *d_tile_sse, uint64_t *d_frame_sse)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!frames || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null descriptor");
	const pxz_params p = decode_side_params(params, true);
	int rc = check_frames(h, frames, &p);
	if (rc != PXZ_OK) return rc;
	if (n_sets == 0) return fail(h, PXZ_ERR_INVALID_ARG, "n_sets must be at least 1");
	if (!d_pixels || !d_tile_w || !d_tile_h || !d_slots || !d_frame_sse) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if ((uint64_t)p.block_w * p.block_h * frames->channels > kVariedMaxTileBytes)
		return fail(h, PXZ_ERR_UNSUPPORTED, "every tile is staged in LDS: block_w*block_h*channels must not exceed %llu bytes",
		            (unsigned long long)kVariedMaxTileBytes);
	Grid g;
	if ((rc = make_grid(h, frames->width, frames->height, p.block_w, p.block_h, frames->n_frames, 0xffffffffull, &g)) != PXZ_OK) return rc;
	// the batch as n_frames equal entries of the per-image table
	std::vector<pxz::VariedImage> images(frames->n_frames, varied_entry(frames->width, frames->height, frames->pitch_bytes, g));
	const uint64_t stride = frames->n_frames > 1 ? frames->frame_stride_bytes : 0;
	for (uint32_t f = 0; f < frames->n_frames; ++f) {
		images[f].offset = f * stride;
		images[f].tile0 = f * g.tiles_per_frame;
		images[f].row0 = f * g.rows;
	}
	const std::vector<uint32_t> sides = unique_sides({p.block_w, p.block_h, g.edge_w, g.edge_h});
	return distortion_launch(h, images, sides, frames->channels, p, n_sets, d_pixels, d_tile_w, d_tile_h, d_slots, d_tile_sse, d_frame_sse,
	                         nullptr);
}

int pxz_distortion_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                        const pxz_params *params, const uint8_t *d_base, const uint32_t *d_tile_w,
                                        const uint32_t *d_tile_h, const uint8_t *d_slots, uint64_t *d_tile_sse, uint64_t *d_image_sse,
                                        uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_base || !d_tile_w || !d_tile_h || !d_slots || !d_image_sse) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	std::vector<uint32_t> sides;
	if ((rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, channels, 0, &images, &sides, nullptr)) != PXZ_OK) return rc;
	return distortion_launch(h, images, sides, channels, p, 1, d_base, d_tile_w, d_tile_h, d_slots, d_tile_sse, d_image_sse, d_image_flags);
}

// ---- fit to a budget: one rung per image, chosen and gathered on the device (pxz_fit.h, pxz_fit.hip) ----------------------
int pxz_fit_select(uint32_t n_images, uint32_t n_factors, uint32_t channels, uint32_t criterion, const uint64_t *targets,
                   const uint64_t *file_bytes, const uint64_t *sse, uint32_t *choice, uint32_t *fit_flags)
{
	if (!targets || !file_bytes || !sse || !choice || !fit_flags) return PXZ_ERR_INVALID_ARG;
	const int rc = fit_check(nullptr, n_images, n_factors, channels, criterion);
	if (rc != PXZ_OK) return rc;
	const uint64_t n = n_images;
	for (uint64_t i = 0; i < n; ++i) {
		const pxz::FitPick p = pxz::fit_pick(
			n_factors, criterion, targets[i], [&](uint32_t r) { return file_bytes[r * n + i]; },
			[&](uint32_t r) {
				uint64_t sum = 0;
				for (uint32_t c = 0; c < channels; ++c) sum += sse[(r * n + i) * channels + c];
				return sum;
			});
		choice[i] = p.choice;
		fit_flags[i] = p.flags;
	}
	return PXZ_OK;
}

int pxz_fit_varied_ladder_device(pxz_handle *h, uint32_t n_images, uint32_t n_factors, uint32_t channels, uint32_t criterion,
                                 const uint64_t *targets, const uint64_t *d_file_offsets, const uint64_t *d_image_sse,
                                 uint32_t *d_choice, uint32_t *d_fit_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!targets) return fail(h, PXZ_ERR_INVALID_ARG, "null targets");
	if (!d_file_offsets || !d_image_sse || !d_choice || !d_fit_flags) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	int rc = fit_check(h, n_images, n_factors, channels, criterion);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	const size_t bytes = (size_t)n_images * 8u;
	if ((rc = ensure(h, h->fit, bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, h->fit_targets.send(targets, bytes, h->fit.ptr, h->stream));
	pxz::FitArgs a{};
	a.n_images = n_images;
	a.n_factors = n_factors;
	a.channels = channels;
	a.criterion = criterion;
	a.targets = (const unsigned long long *)h->fit.ptr;
	a.file_offsets = (const unsigned long long *)d_file_offsets;
	a.image_sse = (const unsigned long long *)d_image_sse;
	a.choice = d_choice;
	a.flags = d_fit_flags;
	PXZ_HIP(h, pxz::launch_fit_select(a, h->stream));
	return PXZ_OK;
}

int pxz_gather_varied_rungs_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                   const pxz_params *params, uint32_t n_factors, const uint32_t *d_choice, const float *d_block_value,
                                   const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, float *d_out_value,
                                   uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (n_factors == 0 || n_factors > PXZ_VARIED_LADDER_MAX_RUNGS)
		return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", PXZ_VARIED_LADDER_MAX_RUNGS, n_factors);
	if (!d_choice || !d_block_value || !d_tile_w || !d_tile_h || !d_out_value || !d_out_w || !d_out_h || (d_out_pixels && !d_slots))
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	std::vector<pxz::VariedImage> images;
	// (mode 0: no detector runs here, so no tile is too small for one)
	int rc = varied_plan(h, descs, n_images, params->block_w, params->block_h, channels, 0, &images, nullptr, nullptr);
	if (rc != PXZ_OK) return rc;
	const uint64_t slot = (uint64_t)params->block_w * params->block_h * channels;
	if (slot > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "a slot of %ux%u px takes more than 2^32-1 bytes", params->block_w, params->block_h);
	if ((uint64_t)n_factors * varied_n_tiles(images) > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::GatherArgs a{};
	if ((rc = varied_upload(h, images, &a.images)) != PXZ_OK) return rc;
	a.n_images = n_images;
	a.n_tiles = varied_n_tiles(images);
	a.n_factors = n_factors;
	a.slot_bytes = (uint32_t)slot;
	a.choice = d_choice;
	a.value = (const uint32_t *)d_block_value;
	a.w = d_tile_w;
	a.h = d_tile_h;
	a.slots = d_slots;
	a.out_value = (uint32_t *)d_out_value;
	a.out_w = d_out_w;
	a.out_h = d_out_h;
	a.out_slots = d_out_pixels;
	a.image_flags = d_image_flags;
	PXZ_HIP(h, pxz::launch_gather_rungs(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

// ---- fit to a budget per tile: one rung per tile under a target per group of images (pxz_tilefit.h, pxz_tilefit.hip) -------
int pxz_fit_tiles_select(uint32_t n_groups, const uint64_t *group_tile_offsets, const uint64_t *group_fixed_bytes, uint32_t n_factors,
                         uint32_t channels, uint32_t criterion, const uint64_t *targets, const uint32_t *tile_bytes, const uint64_t *tile_sse,
                         uint32_t *tile_choice, uint64_t *group_lambda, uint64_t *group_bytes, uint64_t *group_sse, uint32_t *group_flags)
{
	if (!group_tile_offsets || !group_fixed_bytes || !targets || !tile_bytes || !tile_sse || !tile_choice || !group_lambda || !group_bytes ||
	    !group_sse || !group_flags)
		return PXZ_ERR_INVALID_ARG;
	const int rc = fit_check(nullptr, n_groups, n_factors, channels, criterion);  // (n_groups 0: "empty", as no images there)
	if (rc != PXZ_OK) return rc;
	if (group_tile_offsets[0] != 0) return PXZ_ERR_INVALID_ARG;
	for (uint32_t g = 0; g < n_groups; ++g)
		if (group_tile_offsets[g + 1u] <= group_tile_offsets[g]) return PXZ_ERR_INVALID_ARG;  // (a group has a tile)
	const uint64_t tiles = group_tile_offsets[n_groups];
	if (tiles * n_factors > 0xffffffffull) return PXZ_ERR_UNSUPPORTED;
	std::vector<uint64_t> cand(tiles * n_factors);
	for (uint64_t k = 0; k < cand.size(); ++k) cand[k] = pxz::tilefit_pack(tile_bytes[k], tile_sse + k * channels, channels);
	for (uint32_t g = 0; g < n_groups; ++g) {
		const uint64_t t0 = group_tile_offsets[g];
		const pxz::TileFitGroup r = pxz::tilefit_group(
			n_factors, criterion, targets[g], group_fixed_bytes[g], group_tile_offsets[g + 1u] - t0,
			[&](uint32_t rung, uint64_t t) { return cand[rung * tiles + t0 + t]; }, tile_choice + t0);
		group_lambda[g] = r.lambda;
		group_bytes[g] = r.bytes;
		group_sse[g] = r.sse;
		group_flags[g] = r.flags;
	}
	return PXZ_OK;
}

int pxz_fit_varied_tiles_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels, const pxz_params *params,
                                const uint32_t *group_first, uint32_t n_groups, uint32_t n_factors, uint32_t criterion, const uint64_t *targets,
                                const uint32_t *d_record_bytes, const uint64_t *d_tile_sse, uint32_t *d_tile_choice, uint64_t *d_group_lambda,
                                uint64_t *d_group_bytes, uint64_t *d_group_sse, uint32_t *d_group_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!targets) return fail(h, PXZ_ERR_INVALID_ARG, "null targets");
	if (!d_record_bytes || !d_tile_sse || !d_tile_choice || !d_group_lambda || !d_group_bytes || !d_group_sse || !d_group_flags)
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	int rc = fit_check(h, n_images, n_factors, channels, criterion);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	if ((rc = varied_plan(h, descs, n_images, params->block_w, params->block_h, channels, 0, &images, nullptr, nullptr)) != PXZ_OK) return rc;
	// a tile's error stays below 2^32 (tilefit_pack) while it has at most 65536 samples: 65536 * 255^2 < 2^32
	if ((uint64_t)params->block_w * params->block_h * channels > 65536u)
		return fail(h, PXZ_ERR_UNSUPPORTED, "the per-tile fit keeps a tile's squared error in 32 bits: block_w*block_h*channels must not exceed 65536");
	const uint32_t n_tiles = varied_n_tiles(images);
	if ((uint64_t)n_factors * n_tiles > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	if ((rc = tile_groups_check(h, group_first, n_groups, n_images)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	// the groups' table as the kernels read it: targets | fixed bytes | first tiles (n_groups + 1)
	const size_t G = n_groups, K = n_factors;
	const size_t table_bytes = up256(16u * G + 4u * (G + 1u));
	std::vector<uint8_t> table(table_bytes);
	uint64_t *t_targets = reinterpret_cast<uint64_t *>(table.data()), *t_fixed = t_targets + G;
	uint32_t *t_tile0 = reinterpret_cast<uint32_t *>(t_fixed + G);
	for (uint32_t g = 0; g < n_groups; ++g) {
		const uint32_t i0 = group_first ? group_first[g] : g, i1 = group_first ? group_first[g + 1u] : g + 1u;
		t_targets[g] = targets[g];
		t_fixed[g] = 0;
		for (uint32_t i = i0; i < i1; ++i) t_fixed[g] += images[i].hdr_bytes;
		t_tile0[g] = images[i0].tile0;
	}
	t_tile0[n_groups] = n_tiles;
	// behind it, zeroed: the steps' totals, the totals at lambda*, the uniform totals, the groups' bits; then what the kernels
	// write before they read it: the intervals, the uniform rungs, the tiles' groups, the packed candidates
	const size_t zero_u64 = (size_t)pxz::kTileFitSteps * G + 2u * G + 3u * K * G;
	const size_t zero_bytes = zero_u64 * 8u + up256(4u * G);
	const size_t interval_at = table_bytes + zero_bytes, uni_rung_at = interval_at + 32u * G;
	const size_t tile_group_at = uni_rung_at + up256(4u * G), cand_at = tile_group_at + up256(4u * (size_t)n_tiles);
	if ((rc = ensure(h, h->tilefit, cand_at + 8u * K * n_tiles)) != PXZ_OK) return rc;
	uint8_t *d = (uint8_t *)h->tilefit.ptr;
	PXZ_HIP(h, h->tilefit_table.send(table.data(), table_bytes, d, h->stream));
	PXZ_HIP(h, hipMemsetAsync(d + table_bytes, 0, zero_bytes, h->stream));
	pxz::TileFitArgs a{};
	a.n_tiles = n_tiles;
	a.n_groups = n_groups;
	a.n_factors = n_factors;
	a.channels = channels;
	a.criterion = criterion;
	a.targets = (const unsigned long long *)d;
	a.fixed = a.targets + G;
	a.group_tile0 = (const uint32_t *)(a.fixed + G);
	a.acc = (unsigned long long *)(d + table_bytes);
	a.tot = a.acc + (size_t)pxz::kTileFitSteps * G;
	a.uni = a.tot + 2u * G;
	a.group_bits = (uint32_t *)(a.uni + 3u * K * G);
	a.interval = (unsigned long long *)(d + interval_at);
	a.uni_rung = (uint32_t *)(d + uni_rung_at);
	a.tile_group = (uint32_t *)(d + tile_group_at);
	a.cand = (unsigned long long *)(d + cand_at);
	a.record_bytes = d_record_bytes;
	a.tile_sse = (const unsigned long long *)d_tile_sse;
	a.tile_choice = d_tile_choice;
	a.group_lambda = (unsigned long long *)d_group_lambda;
	a.group_bytes = (unsigned long long *)d_group_bytes;
	a.group_sse = (unsigned long long *)d_group_sse;
	a.group_flags = d_group_flags;
	PXZ_HIP(h, pxz::launch_tilefit(a, h->stream));
	return PXZ_OK;
}

int pxz_gather_varied_tile_rungs_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                        const pxz_params *params, uint32_t n_factors, const uint32_t *d_tile_choice,
                                        const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                                        float *d_out_value, uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (n_factors == 0 || n_factors > PXZ_VARIED_LADDER_MAX_RUNGS)
		return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", PXZ_VARIED_LADDER_MAX_RUNGS, n_factors);
	if (!d_tile_choice || !d_block_value || !d_tile_w || !d_tile_h || !d_out_value || !d_out_w || !d_out_h || (d_out_pixels && !d_slots))
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	std::vector<pxz::VariedImage> images;
	int rc = varied_plan(h, descs, n_images, params->block_w, params->block_h, channels, 0, &images, nullptr, nullptr);
	if (rc != PXZ_OK) return rc;
	const uint64_t slot = (uint64_t)params->block_w * params->block_h * channels;
	if (slot > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "a slot of %ux%u px takes more than 2^32-1 bytes", params->block_w, params->block_h);
	if ((uint64_t)n_factors * varied_n_tiles(images) > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::GatherArgs a{};
	if ((rc = varied_upload(h, images, &a.images)) != PXZ_OK) return rc;
	if ((rc = zero_owner_flags(h, d_image_flags, n_images)) != PXZ_OK) return rc;
	a.n_images = n_images;
	a.n_tiles = varied_n_tiles(images);
	a.n_factors = n_factors;
	a.slot_bytes = (uint32_t)slot;
	a.choice = d_tile_choice;
	a.value = (const uint32_t *)d_block_value;
	a.w = d_tile_w;
	a.h = d_tile_h;
	a.slots = d_slots;
	a.out_value = (uint32_t *)d_out_value;
	a.out_w = d_out_w;
	a.out_h = d_out_h;
	a.out_slots = d_out_pixels;
	a.image_flags = d_image_flags;
	PXZ_HIP(h, pxz::launch_gather_tile_rungs(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

}  // extern "C"

// ---- fit an archive to a budget, at its own block size or a new one: the error of re-shrunk or re-tiled tiles against the
// archive's own (pxz_reshrink_distortion.hip, pxz_retile_distortion.hip) ------------------------------------------------------
namespace {

// Both archive distortions behind one body, from the check of the device pointers on: the archive's stored tiles (ref; b.retile:
// in the layout of the source block) against n_sets stored versions (sets) of the tiles of params' block.  Args is the
// kernel's struct; admit(wdw_ref, wdw_set): its footprint against LDS under its own text; launch(a, d_src_images): its launch.
template <class Args, class Admit, class Launch>
int archive_distortion(pxz_handle *h, const ArchiveBatch &b, uint32_t n_sets, const StoredTiles &ref, const StoredTiles &sets, uint64_t *d_tile_sse,
                       uint64_t *d_image_sse, uint32_t *d_image_flags, Admit admit, Launch launch)
{
	if (!ref.w || !ref.h || !ref.slots || !sets.w || !sets.h || !sets.slots || !d_image_sse) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	const uint32_t n_images = b.n_images, channels = b.channels;
	const pxz_params p = decode_side_params(b.params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	if (b.retile && (b.src_bw == 0 || b.src_bh == 0)) return fail(h, PXZ_ERR_INVALID_ARG, "zero source block size");
	if (n_sets == 0) return fail(h, PXZ_ERR_INVALID_ARG, "n_sets must be at least 1");
	if (b.expand_filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "expand_filter must be 0..4, got %u", b.expand_filter);
	// (each call's own order: the re-tile holds its blocks against LDS before it looks at the batch, the re-shrink behind that)
	if (b.retile && (rc = admit(1u, 1u)) != PXZ_OK) return rc;
	ArchivePlan plan;
	if ((rc = archive_plan(h, b, p, n_sets, "sets", &plan)) != PXZ_OK) return rc;
	if (!b.retile && (rc = admit(1u, 1u)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	Args a{};
	if ((rc = put_both_expand_tables(h, channels, archive_expand_params(b, p), plan.in_sides(), p, plan.sides, &a.r, &a.u)) != PXZ_OK) return rc;
	if ((rc = admit(a.r.wdw, a.u.wdw)) != PXZ_OK) return rc;
	a.n_images = n_images;
	a.n_tiles = plan.n_tiles();
	a.n_sets = n_sets;
	put_stored_tiles(&a.r, plan.n_in_tiles(), ref);
	put_stored_tiles(&a.u, a.n_tiles, sets);
	a.tile_sse = reinterpret_cast<unsigned long long *>(d_tile_sse);
	a.image_sse = reinterpret_cast<unsigned long long *>(d_image_sse);
	if ((rc = fresh_status_and_flags(h, &a.r.status, d_image_flags, n_images, &a.image_flags)) != PXZ_OK) return rc;
	a.u.status = a.r.status;
	PXZ_HIP(h, hipMemsetAsync(d_image_sse, 0, (size_t)n_sets * n_images * channels * 8u, h->stream));
	const pxz::VariedImage *d_src_images = nullptr;
	if ((rc = archive_upload(h, plan, &a.images, &d_src_images)) != PXZ_OK) return rc;
	return launch(a, d_src_images);
}

}  // namespace

extern "C" {

int pxz_reshrink_distortion_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t expand_filter, uint32_t filter_up,
                                      uint32_t *lds_bytes)
{
	if (!lds_bytes || block_w == 0 || block_h == 0 || (channels != 3 && channels != 4) || expand_filter > 4 || filter_up > 4)
		return PXZ_ERR_INVALID_ARG;
	const BlockTables set{block_w, block_h, filter_up};
	return archive_lds_query(reshrink_distortion_footprint(block_w, block_h), {block_w, block_h, expand_filter}, &set, lds_bytes);
}

int pxz_reshrink_distortion_varied_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                          const pxz_params *params, uint32_t expand_filter, uint32_t n_sets, const uint32_t *d_ref_w,
                                          const uint32_t *d_ref_h, const uint8_t *d_ref_slots, const uint32_t *d_tile_w,
                                          const uint32_t *d_tile_h, const uint8_t *d_slots, uint64_t *d_tile_sse, uint64_t *d_image_sse,
                                          uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	const ArchiveBatch b{descs, n_images, channels, false, 0u, 0u, params, expand_filter};
	return archive_distortion<pxz::ReshrinkDistortionArgs>(
	    h, b, n_sets, {d_ref_w, d_ref_h, d_ref_slots}, {d_tile_w, d_tile_h, d_slots}, d_tile_sse, d_image_sse, d_image_flags,
	    [&](uint32_t wdw_ref, uint32_t wdw_set) {
		    const auto bytes = reshrink_distortion_footprint(params->block_w, params->block_h);
		    if (beyond_lds(bytes, wdw_ref, wdw_set))
			    return fail(h, PXZ_ERR_UNSUPPORTED,
			                "a wave keeps three planes of block_w*block_h dwords and the windows of both axes in LDS: %llu bytes exceed the %u a block has (%ux%u)",
			                (unsigned long long)bytes(wdw_ref, wdw_set), kLdsPerCu, params->block_w, params->block_h);
		    return (int)PXZ_OK;
	    },
	    [&](pxz::ReshrinkDistortionArgs &a, const pxz::VariedImage *) {
		    a.wdw = std::max(a.r.wdw, a.u.wdw);
		    a.tile_dw = pxz::reshrink_distortion_tile_dw(params->block_w, params->block_h, a.wdw);
		    PXZ_HIP(h, pxz::launch_reshrink_distortion(a, channels, h->n_cus, h->stream));
		    return (int)PXZ_OK;
	    });
}

int pxz_retile_distortion_lds_bytes(uint32_t src_block_w, uint32_t src_block_h, uint32_t block_w, uint32_t block_h, uint32_t channels,
                                    uint32_t expand_filter, uint32_t filter_up, uint32_t *lds_bytes)
{
	if (!lds_bytes || src_block_w == 0 || src_block_h == 0 || block_w == 0 || block_h == 0 || (channels != 3 && channels != 4) || expand_filter > 4 ||
	    filter_up > 4)
		return PXZ_ERR_INVALID_ARG;
	const BlockTables set{block_w, block_h, filter_up};
	return archive_lds_query(retile_distortion_footprint(src_block_w, src_block_h, block_w, block_h), {src_block_w, src_block_h, expand_filter}, &set,
	                         lds_bytes);
}

int pxz_retile_distortion_varied_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                        uint32_t src_block_w, uint32_t src_block_h, const pxz_params *params, uint32_t expand_filter,
                                        uint32_t n_sets, const uint32_t *d_ref_w, const uint32_t *d_ref_h, const uint8_t *d_ref_slots,
                                        const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, uint64_t *d_tile_sse,
                                        uint64_t *d_image_sse, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	const ArchiveBatch b{descs, n_images, channels, true, src_block_w, src_block_h, params, expand_filter};
	return archive_distortion<pxz::RetileDistortionArgs>(
	    h, b, n_sets, {d_ref_w, d_ref_h, d_ref_slots}, {d_tile_w, d_tile_h, d_slots}, d_tile_sse, d_image_sse, d_image_flags,
	    [&](uint32_t wdw_src, uint32_t wdw_set) {
		    if (beyond_lds(retile_distortion_footprint(src_block_w, src_block_h, params->block_w, params->block_h), wdw_src, wdw_set))
			    return fail(h, PXZ_ERR_UNSUPPORTED,
			                "the distortion of re-tiled tiles keeps two %ux%u tile images (a dword per pixel) and the staged parts and windows of %ux%u source "
			                "tiles, or of a whole stored %ux%u tile, in LDS: they exceed a block's 160 KB (pxz_retile_distortion_lds_bytes)",
			                params->block_w, params->block_h, src_block_w, src_block_h, params->block_w, params->block_h);
		    return (int)PXZ_OK;
	    },
	    [&](pxz::RetileDistortionArgs &a, const pxz::VariedImage *d_src_images) {
		    a.src_images = d_src_images;
		    PXZ_HIP(h, pxz::launch_retile_distortion(a, channels, h->n_cus, h->stream));
		    return (int)PXZ_OK;
	    });
}

}  // extern "C"

// ---- pixel windows of files (window_index_kernel in pxz_stream.hip, pxz_window.hip) ---------------------------------------
namespace pxz_runtime {

// The per-window table of a call, checked window by window before anything is launched.  channels 0: geometry only
// (pxz_window_layout, the decode stage), no pitch rule.  sides: the block sides and the edge sizes of the images the windows
// touch (what the expand tables are built for).
int window_plan(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *w, uint32_t n_windows, uint32_t bw,
                uint32_t bh, uint32_t channels, std::vector<pxz::WindowEntry> *entries, std::vector<uint32_t> *sides, uint32_t *n_rows)
{
	if (!w) return fail(h, PXZ_ERR_INVALID_ARG, "null windows");
	if (n_windows == 0) return fail(h, PXZ_ERR_INVALID_ARG, "no windows");
	std::vector<pxz::VariedImage> images;
	const int rc = varied_plan(h, descs, n_images, bw, bh, 0, 0, &images, nullptr, nullptr);
	if (rc != PXZ_OK) return rc;
	entries->resize(n_windows);
	std::vector<uint32_t> all = {bw, bh};
	uint64_t tiles = 0, rows_total = 0;
	for (uint32_t k = 0; k < n_windows; ++k) {
		const pxz_window &g = w[k];
		if (g.image >= n_images) return fail(h, PXZ_ERR_INVALID_ARG, "window %u: image index %u out of range (%u images)", k, g.image, n_images);
		const pxz::VariedImage &im = images[g.image];
		if (g.width == 0 || g.height == 0) return fail(h, PXZ_ERR_INVALID_ARG, "window %u: empty rectangle (%ux%u)", k, g.width, g.height);
		if ((uint64_t)g.x + g.width > im.width || (uint64_t)g.y + g.height > im.height)
			return fail(h, PXZ_ERR_INVALID_ARG, "window %u: the rectangle %ux%u at (%u, %u) leaves image %u (%ux%u)", k, g.width, g.height, g.x, g.y,
			            g.image, im.width, im.height);
		if (channels && (uint64_t)g.pitch_bytes < (uint64_t)g.width * channels)
			return fail(h, PXZ_ERR_INVALID_ARG, "window %u: pitch smaller than a row", k);
		pxz::WindowEntry &e = (*entries)[k];
		e.offset = g.offset_bytes;
		e.image = g.image;
		e.x = g.x;
		e.y = g.y;
		e.w = g.width;
		e.h = g.height;
		e.pitch = g.pitch_bytes;
		e.c0 = g.x / bw;
		e.r0 = g.y / bh;
		e.ccols = (g.x + g.width - 1u) / bw - e.c0 + 1u;
		e.crows = (g.y + g.height - 1u) / bh - e.r0 + 1u;
		e.img_w = im.width;
		e.img_h = im.height;
		e.cols = im.cols;
		e.rows = im.rows;
		e.edge_w = im.edge_w;
		e.edge_h = im.edge_h;
		e.tile0 = (uint32_t)tiles;
		e.row0 = (uint32_t)rows_total;
		tiles += (uint64_t)e.ccols * e.crows;
		rows_total += e.crows;
		if (tiles > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "window %u: more than 2^32-1 covered tiles in the call", k);
		all.push_back(im.edge_w);
		all.push_back(im.edge_h);
	}
	if (sides) *sides = unique_sides(std::move(all));
	if (n_rows) *n_rows = (uint32_t)rows_total;
	return PXZ_OK;
}

}  // namespace pxz_runtime

namespace {

// the per-window table -> handle scratch, as varied_upload sends the per-image table: one copy
int window_upload(pxz_handle *h, const std::vector<pxz::WindowEntry> &entries, const pxz::WindowEntry **d_windows)
{
	const size_t bytes = entries.size() * sizeof(pxz::WindowEntry);
	int rc = ensure(h, h->windows, bytes);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, h->window_table.send(entries.data(), bytes, h->windows.ptr, h->stream));
	*d_windows = (const pxz::WindowEntry *)h->windows.ptr;
	return PXZ_OK;
}

}  // namespace

extern "C" {

int pxz_window_layout(const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows, uint32_t block_w,
                      uint32_t block_h, uint64_t *tile_offsets)
{
	if (!tile_offsets) return PXZ_ERR_INVALID_ARG;
	std::vector<pxz::WindowEntry> entries;
	const int rc = window_plan(nullptr, descs, n_images, windows, n_windows, block_w, block_h, 0, &entries, nullptr, nullptr);
	if (rc != PXZ_OK) return rc;
	for (uint32_t k = 0; k < n_windows; ++k) tile_offsets[k] = entries[k].tile0;
	tile_offsets[n_windows] = window_n_tiles(entries);
	return PXZ_OK;
}

int pxz_decode_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows,
                              uint32_t channels, const pxz_params *params, const uint8_t *d_files, const uint64_t *d_file_offsets,
                              float *d_block_value, uint32_t *d_tile_w, uint32_t *d_tile_h, uint8_t *d_slots, uint32_t *d_window_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_files || !d_file_offsets || !d_block_value || !d_tile_w || !d_tile_h || !d_slots)
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	const pxz_params p = decode_side_params(params, false);
	std::vector<pxz::WindowEntry> entries;
	uint32_t n_rows = 0;
	int rc = window_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, 0, &entries, nullptr, &n_rows);
	if (rc != PXZ_OK) return rc;
	pxz::DecodeArgs a{};
	if ((rc = flat_decode_args(h, p, channels, n_images, window_n_tiles(entries), d_files, d_file_offsets, d_block_value, d_tile_w, d_tile_h, d_slots,
	                           &a)) != PXZ_OK)
		return rc;
	uint32_t *flags = nullptr;
	if ((rc = varied_flags(h, d_window_flags, n_windows, &flags)) != PXZ_OK) return rc;
	const pxz::WindowEntry *d_windows = nullptr;
	if ((rc = window_upload(h, entries, &d_windows)) != PXZ_OK) return rc;
	return launch_on_bins(h, h->dbins_clean, a.bins, [&](bool bins_clean) {
		return pxz::launch_decode_windows(a, d_windows, n_windows, n_rows, flags, bins_clean, h->stream);
	});
}

int pxz_expand_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows,
                              uint32_t channels, const pxz_params *params, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                              const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_window_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_tile_w || !d_tile_h || !d_slots || !d_base) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::WindowEntry> entries;
	std::vector<uint32_t> sides;
	if ((rc = window_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, channels, &entries, &sides, nullptr)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::WindowExpandArgs a{};
	if ((rc = put_varied_expand_tables(h, p, channels, sides, &a, true)) != PXZ_OK) return rc;
	a.n_windows = n_windows;
	put_stored_tiles(&a, window_n_tiles(entries), {d_tile_w, d_tile_h, d_slots});
	a.base = d_base;
	if ((rc = fresh_status_and_flags(h, &a.status, d_window_flags, n_windows, &a.window_flags)) != PXZ_OK) return rc;
	if ((rc = window_upload(h, entries, &a.windows)) != PXZ_OK) return rc;
	PXZ_HIP(h, pxz::launch_window_expand(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

}  // extern "C"

// ---- decode at reduced scale (pxz_scaled_expand.hip) --------------------------------------------------------------------
namespace pxz_runtime {

// one owner's scale: 2^shift must divide both block sides (who: "image" or "window")
int scaled_check_shift(pxz_handle *h, const char *who, uint32_t index, uint32_t shift, uint32_t bw, uint32_t bh)
{
	if (shift > 31u || (bw & ((1u << shift) - 1u)) != 0u || (bh & ((1u << shift) - 1u)) != 0u)
		return fail(h, PXZ_ERR_INVALID_ARG, "%s %u: the scale 2^%u does not divide the %ux%u block", who, index, shift, bw, bh);
	return PXZ_OK;
}

// a window's corners lie on multiples of its scale, or on the image's right and lower edge
int scaled_check_window(pxz_handle *h, uint32_t index, const pxz_window &w, uint32_t img_w, uint32_t img_h, uint32_t shift)
{
	const uint32_t low = (1u << shift) - 1u;
	const uint32_t x1 = w.x + w.width, y1 = w.y + w.height;
	if ((w.x & low) != 0u || (w.y & low) != 0u || ((x1 & low) != 0u && x1 != img_w) || ((y1 & low) != 0u && y1 != img_h))
		return fail(h, PXZ_ERR_INVALID_ARG, "window %u: the rectangle %ux%u at (%u, %u) does not lie on multiples of the scale 2^%u (or on the image's edge)",
		            index, w.width, w.height, w.x, w.y, shift);
	return PXZ_OK;
}

}  // namespace pxz_runtime

namespace {

// the (target size, largest stored size) pairs of one owner's tiles: the block sides and the image's edges at the owner's scale
void scaled_add_targets(std::map<uint32_t, uint32_t> *most, uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t shift)
{
	for (uint32_t full : {bw, bh, edge_w, edge_h}) {
		uint32_t &m = (*most)[scaled_extent(full, shift)];
		if (full > m) m = full;
	}
}

// dwords of the staged windows of one axis for a call (scaled_window_dw over the block's longer side)
uint32_t scaled_call_window_dw(uint32_t bw, uint32_t bh, uint32_t filter, uint32_t max_shift)
{
	return pxz::scaled_window_dw(bw > bh ? bw : bh, pxz::filter_support(filter), max_shift);
}

// The tables of a scaled call, cached on the handle under (filter, pairs), and with them everything of ScaledExpandArgs that
// does not depend on the owners.  A wave's image beyond LDS is refused here.
int put_scaled_tables(pxz_handle *h, const pxz_params &p, uint32_t channels, const std::map<uint32_t, uint32_t> &most, uint32_t max_shift,
                      pxz::ScaledExpandArgs *a)
{
	a->bw = p.block_w;
	a->bh = p.block_h;
	a->slot_bytes = p.block_w * p.block_h * channels;
	a->filter = p.filter;
	a->win_dw = scaled_call_window_dw(p.block_w, p.block_h, p.filter, max_shift);
	a->tile_dw = pxz::scaled_tile_dw(a->bw, a->bh, a->win_dw);
	if (varied_image_beyond_lds(a->tile_dw))
		return fail(h, PXZ_ERR_UNSUPPORTED, "a wave keeps a %ux%u tile of %u channels and its windows in LDS: %llu bytes exceed what a block has", a->bw,
		            a->bh, channels, (unsigned long long)a->tile_dw * 4u);
	std::vector<uint32_t> flat;
	for (const auto &tm : most) {
		flat.push_back(tm.first);
		flat.push_back(tm.second);
	}
	const ScaledExpandTables *st = nullptr;
	const int rc = cached_tables(h, h->scaled_tables, std::make_pair(p.filter, flat), kTableCacheBound, [&](ScaledExpandTables &t) {
		std::vector<uint32_t> targets, stored;
		for (const auto &tm : most) {
			targets.push_back(tm.first);
			stored.push_back(tm.second);
		}
		pxz::ScaledExpandTableSet s;
		if (!pxz::build_scaled_expand_tables(targets, stored, p.filter, &s)) return fail(h, PXZ_ERR_INVALID_ARG, "unknown filter %u", p.filter);
		t.stride = s.stride;
		t.max_win_dw = s.max_win_dw;
		return upload_tables(h, {{s.slot, &t.d_slot}, {s.dir, &t.d_dir}, {s.mixed, &t.d_mixed}, {s.starts, &t.d_starts}, {s.sizes, &t.d_sizes},
		                         {s.coeffs, &t.d_coeffs}}, &t.mem);
	}, &st);
	if (rc != PXZ_OK) return rc;
	// (the bound of scaled_window_dw holds for every pair a tile of the call can have; a set beyond it would overrun the staging)
	if (st->max_win_dw > a->win_dw)
		return fail(h, PXZ_ERR_INTERNAL, "staged windows of %u dwords exceed the %u the layout has", st->max_win_dw, a->win_dw);
	a->slot = st->d_slot;
	a->dir = st->d_dir;
	a->mixed = st->d_mixed;
	a->stride = st->stride;
	a->starts = st->d_starts;
	a->sizes = st->d_sizes;
	a->coeffs = st->d_coeffs;
	return PXZ_OK;
}

// the per-owner table -> handle scratch, as varied_upload sends the per-image table: one copy
template <class Entry>
int scaled_upload(pxz_handle *h, const std::vector<Entry> &entries, const Entry **d_entries)
{
	const size_t bytes = entries.size() * sizeof(Entry);
	int rc = ensure(h, h->scaled, bytes);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, h->scaled_table.send(entries.data(), bytes, h->scaled.ptr, h->stream));
	*d_entries = (const Entry *)h->scaled.ptr;
	return PXZ_OK;
}

}  // namespace

extern "C" {

int pxz_scaled_size(uint32_t width, uint32_t height, uint32_t block_w, uint32_t block_h, uint32_t scale_log2, uint32_t *out_w, uint32_t *out_h)
{
	if (!out_w || !out_h || width == 0 || height == 0 || block_w == 0 || block_h == 0) return PXZ_ERR_INVALID_ARG;
	if (width > kMaxImageSide || height > kMaxImageSide) return PXZ_ERR_UNSUPPORTED;
	const int rc = scaled_check_shift(nullptr, "image", 0, scale_log2, block_w, block_h);
	if (rc != PXZ_OK) return rc;
	*out_w = scaled_extent(width, scale_log2);
	*out_h = scaled_extent(height, scale_log2);
	return PXZ_OK;
}

int pxz_scaled_axis_table(uint32_t in_size, uint32_t out_size, uint32_t filter, uint32_t other_axis_grows, int32_t *starts, int32_t *sizes,
                          int16_t *coeffs, int32_t *window, int32_t *precision)
{
	if (in_size == 0 || out_size == 0 || filter > 4) return PXZ_ERR_INVALID_ARG;
	pxz::AxisWindows w;
	if (!pxz::build_axis(in_size, out_size, filter, &w, out_size > in_size || other_axis_grows != 0u)) return PXZ_ERR_INVALID_ARG;
	if (window) *window = w.window;
	if (precision) *precision = w.precision;
	if (starts) std::memcpy(starts, w.starts.data(), sizeof(int32_t) * out_size);
	if (sizes) std::memcpy(sizes, w.sizes.data(), sizeof(int32_t) * out_size);
	if (coeffs && !w.coeffs.empty()) std::memcpy(coeffs, w.coeffs.data(), sizeof(int16_t) * w.coeffs.size());
	return PXZ_OK;
}

int pxz_expand_scaled_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t filter, uint32_t max_scale_log2, uint32_t *lds_bytes)
{
	if (!lds_bytes || block_w == 0 || block_h == 0 || filter > 4 || (channels != 3 && channels != 4)) return PXZ_ERR_INVALID_ARG;
	const int rc = scaled_check_shift(nullptr, "image", 0, max_scale_log2, block_w, block_h);
	if (rc != PXZ_OK) return rc;
	const uint32_t tile_dw = pxz::scaled_tile_dw(block_w, block_h, scaled_call_window_dw(block_w, block_h, filter, max_scale_log2));
	*lds_bytes = tile_dw > 0x3fffffffu ? 0xffffffffu : tile_dw * 4u;
	if ((uint64_t)block_w * block_h * channels > kVariedMaxTileBytes || varied_image_beyond_lds(tile_dw)) return PXZ_ERR_UNSUPPORTED;
	return PXZ_OK;
}

int pxz_expand_varied_scaled_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                           const pxz_params *params, const uint32_t *scale_log2, const uint32_t *d_tile_w,
                                           const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_tile_w || !d_tile_h || !d_slots || !d_base) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (!scale_log2) return fail(h, PXZ_ERR_INVALID_ARG, "null scales");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	// (the geometry is the files'; the pitch rule is held against the scaled rows below)
	std::vector<pxz::VariedImage> images;
	if ((rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, 0, 0, &images, nullptr, nullptr)) != PXZ_OK) return rc;
	std::vector<pxz::ScaledImage> entries(n_images);
	std::map<uint32_t, uint32_t> most;
	uint32_t max_shift = 0;
	for (uint32_t i = 0; i < n_images; ++i) {
		const uint32_t k = scale_log2[i];
		if ((rc = scaled_check_shift(h, "image", i, k, p.block_w, p.block_h)) != PXZ_OK) return rc;
		const pxz::VariedImage &im = images[i];
		if ((uint64_t)im.pitch < (uint64_t)scaled_extent(im.width, k) * channels) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: pitch smaller than a row", i);
		entries[i] = pxz::ScaledImage{im.offset, im.tile0, im.pitch, im.cols, im.rows, im.edge_w, im.edge_h, k, 0u};
		scaled_add_targets(&most, p.block_w, p.block_h, im.edge_w, im.edge_h, k);
		if (k > max_shift) max_shift = k;
	}
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::ScaledExpandArgs a{};
	if ((rc = put_scaled_tables(h, p, channels, most, max_shift, &a)) != PXZ_OK) return rc;
	a.n_owners = n_images;
	put_stored_tiles(&a, varied_n_tiles(images), {d_tile_w, d_tile_h, d_slots});
	a.base = d_base;
	if ((rc = fresh_status_and_flags(h, &a.status, d_image_flags, n_images, &a.flags)) != PXZ_OK) return rc;
	if ((rc = scaled_upload(h, entries, &a.images)) != PXZ_OK) return rc;
	PXZ_HIP(h, pxz::launch_scaled_expand(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

int pxz_expand_windows_scaled_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows,
                                     uint32_t channels, const pxz_params *params, const uint32_t *scale_log2, const uint32_t *d_tile_w,
                                     const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_window_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_tile_w || !d_tile_h || !d_slots || !d_base) return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (!scale_log2) return fail(h, PXZ_ERR_INVALID_ARG, "null scales");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	// (the rectangles are full-resolution ones; the pitch rule is held against the scaled rows below)
	std::vector<pxz::WindowEntry> plan;
	if ((rc = window_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, 0, &plan, nullptr, nullptr)) != PXZ_OK) return rc;
	std::vector<pxz::ScaledWindow> entries(n_windows);
	std::map<uint32_t, uint32_t> most;
	uint32_t max_shift = 0;
	for (uint32_t k = 0; k < n_windows; ++k) {
		const uint32_t sh = scale_log2[k];
		const pxz::WindowEntry &e = plan[k];
		if ((rc = scaled_check_shift(h, "window", k, sh, p.block_w, p.block_h)) != PXZ_OK) return rc;
		if ((rc = scaled_check_window(h, k, windows[k], e.img_w, e.img_h, sh)) != PXZ_OK) return rc;
		const uint32_t x0 = e.x >> sh, y0 = e.y >> sh, x1 = scaled_extent(e.x + e.w, sh), y1 = scaled_extent(e.y + e.h, sh);
		if ((uint64_t)e.pitch < (uint64_t)(x1 - x0) * channels) return fail(h, PXZ_ERR_INVALID_ARG, "window %u: pitch smaller than a row", k);
		entries[k] = pxz::ScaledWindow{e.offset, e.tile0, e.pitch, x0, y0, x1, y1, e.c0, e.r0, e.ccols, e.cols, e.rows, e.edge_w, e.edge_h, sh};
		scaled_add_targets(&most, p.block_w, p.block_h, e.edge_w, e.edge_h, sh);
		if (sh > max_shift) max_shift = sh;
	}
	PXZ_HIP(h, hipSetDevice(h->device));
	pxz::ScaledExpandArgs a{};
	if ((rc = put_scaled_tables(h, p, channels, most, max_shift, &a)) != PXZ_OK) return rc;
	a.n_owners = n_windows;
	put_stored_tiles(&a, window_n_tiles(plan), {d_tile_w, d_tile_h, d_slots});
	a.base = d_base;
	if ((rc = fresh_status_and_flags(h, &a.status, d_window_flags, n_windows, &a.flags)) != PXZ_OK) return rc;
	if ((rc = scaled_upload(h, entries, &a.windows)) != PXZ_OK) return rc;
	PXZ_HIP(h, pxz::launch_scaled_expand(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

}  // extern "C"

// ---- patch of pixel windows (pxz_patch.hip): new pixels into the covered tiles of .pixlzr files ----------------------------
namespace pxz_runtime {

// window_plan, and the rule of the patch on top of it: the covered tile rectangles of one image are pairwise disjoint.
// *bad_window (may be null): the first window that covers a tile an earlier window of its image covers, else PXZ_NO_WINDOW.
int patch_plan(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *w, uint32_t n_windows, uint32_t bw, uint32_t bh,
               uint32_t channels, std::vector<pxz::WindowEntry> *entries, std::vector<uint32_t> *sides, uint32_t *bad_window)
{
	if (bad_window) *bad_window = PXZ_NO_WINDOW;
	const int rc = window_plan(h, descs, n_images, w, n_windows, bw, bh, channels, entries, sides, nullptr);
	if (rc != PXZ_OK) return rc;
	// the windows of each image side by side, in the order of the call
	std::vector<uint32_t> order(n_windows);
	for (uint32_t k = 0; k < n_windows; ++k) order[k] = k;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (*entries)[a].image < (*entries)[b].image; });
	uint32_t bad = PXZ_NO_WINDOW, with = 0;
	for (size_t lo = 0; lo < order.size();) {
		size_t hi = lo;
		while (hi < order.size() && (*entries)[order[hi]].image == (*entries)[order[lo]].image) ++hi;
		for (size_t i = lo + 1; i < hi && order[i] < bad; ++i) {
			const pxz::WindowEntry &a = (*entries)[order[i]];
			for (size_t j = lo; j < i; ++j) {
				const pxz::WindowEntry &b = (*entries)[order[j]];
				if (a.c0 < b.c0 + b.ccols && b.c0 < a.c0 + a.ccols && a.r0 < b.r0 + b.crows && b.r0 < a.r0 + a.crows) {
					bad = order[i];
					with = order[j];
					break;
				}
			}
			if (bad == order[i]) break;
		}
		lo = hi;
	}
	if (bad == PXZ_NO_WINDOW) return PXZ_OK;
	if (bad_window) *bad_window = bad;
	return fail(h, PXZ_ERR_INVALID_ARG, "window %u: covers a tile of image %u that window %u covers too (the covered tiles of a patch must be disjoint)",
	            bad, (*entries)[bad].image, with);
}

}  // namespace pxz_runtime

extern "C" {

int pxz_patch_check(const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows, uint32_t block_w,
                    uint32_t block_h, uint64_t *tile_offsets, uint32_t *bad_window)
{
	if (bad_window) *bad_window = PXZ_NO_WINDOW;
	if (!tile_offsets) return PXZ_ERR_INVALID_ARG;
	std::vector<pxz::WindowEntry> entries;
	const int rc = patch_plan(nullptr, descs, n_images, windows, n_windows, block_w, block_h, 0, &entries, nullptr, bad_window);
	if (rc != PXZ_OK) return rc;
	for (uint32_t k = 0; k < n_windows; ++k) tile_offsets[k] = entries[k].tile0;
	tile_offsets[n_windows] = window_n_tiles(entries);
	return PXZ_OK;
}

int pxz_patch_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows,
                             uint32_t channels, const pxz_params *params, uint32_t expand_filter, const uint8_t *d_patch_base,
                             const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w,
                             uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_window_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_patch_base || !d_tile_w || !d_tile_h || !d_slots || !d_block_value || !d_out_w || !d_out_h)
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	const pxz_params p = *params;
	int rc = check_params(h, &p);
	if (rc != PXZ_OK) return rc;
	if (expand_filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "expand_filter must be 0..4, got %u", expand_filter);
	if ((rc = reshrink_check_block(h, p.mode, p.block_w, p.block_h, 0u, 1u)) != PXZ_OK) return rc;
	std::vector<pxz::WindowEntry> entries;
	std::vector<uint32_t> sides;
	if ((rc = patch_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, channels, &entries, &sides, nullptr)) != PXZ_OK) return rc;
	if (p.mode == PXZ_MODE_SHRINK_DIRECTIONALLY)
		for (uint32_t k = 0; k < n_windows; ++k) {
			// the covered tiles' sizes: the block, and the image's edge where the window reaches its last column or row
			const pxz::WindowEntry &e = entries[k];
			const uint32_t least_w = e.c0 + e.ccols == e.cols ? e.edge_w : p.block_w, least_h = e.r0 + e.crows == e.rows ? e.edge_h : p.block_h;
			if (least_w < 2 || least_h < 2 || p.block_w < 2 || p.block_h < 2)
				return fail(h, PXZ_ERR_TILE_TOO_SMALL,
				            "window %u: directional detector needs tiles of at least 2x2 px (a covered edge tile is %ux%u); the reference panics here", k,
				            least_w, least_h);
		}
	PXZ_HIP(h, hipSetDevice(h->device));
	const VariedTables *vt = nullptr;
	if ((rc = get_varied_tables(h, p.filter, sides, &vt)) != PXZ_OK) return rc;
	pxz::PatchArgs a{};
	pxz_params xp = p;
	xp.filter = expand_filter;
	if ((rc = put_varied_expand_tables(h, xp, channels, sides, &a.r.x)) != PXZ_OK) return rc;
	if ((rc = reshrink_check_block(h, p.mode, p.block_w, p.block_h, 0u, a.r.x.wdw)) != PXZ_OK) return rc;
	if ((rc = fresh_status_and_flags(h, &a.r.x.status, d_window_flags, n_windows, &a.window_flags)) != PXZ_OK) return rc;
	if ((rc = window_upload(h, entries, &a.windows)) != PXZ_OK) return rc;
	pxz::VariedArgs &v = a.r.v;
	varied_fill_shrink(h, channels, &p, vt, d_block_value, d_out_w, d_out_h, d_out_pixels, &v);
	v.n_tiles = window_n_tiles(entries);
	v.tile_bytes = (p.block_w * p.block_h * 4u + 15u) & ~15u;  // one plane, as the re-shrink's
	put_stored_tiles(&a.r.x, v.n_tiles, {d_tile_w, d_tile_h, d_slots});
	a.n_windows = n_windows;
	a.patch_base = d_patch_base;
	a.factor[0] = p.factor;
	PXZ_HIP(h, pxz::launch_patch(a, channels, h->n_cus, h->stream));
	return PXZ_OK;
}

int pxz_splice_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows,
                              uint32_t channels, const pxz_params *params, const uint8_t *d_files, const uint64_t *d_file_offsets,
                              const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                              const uint32_t *d_reader_flags, const uint32_t *d_patch_flags, uint8_t *d_out, uint64_t out_capacity,
                              uint64_t *d_out_file_offsets, uint32_t *d_image_flags)
{
	using pxz::SpliceBound;
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!params) return fail(h, PXZ_ERR_INVALID_ARG, "null params");
	if (!d_files || !d_file_offsets || !d_block_value || !d_tile_w || !d_tile_h || !d_slots || !d_out_file_offsets || (!d_out && out_capacity))
		return fail(h, PXZ_ERR_INVALID_ARG, "null device pointer");
	if (channels != 3 && channels != 4) return fail(h, PXZ_ERR_INVALID_ARG, "channels must be 3 or 4, got %u", channels);
	const pxz_params p = decode_side_params(params, false);
	std::vector<pxz::WindowEntry> entries;
	int rc = patch_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, 0, &entries, nullptr, nullptr);
	if (rc != PXZ_OK) return rc;
	const uint32_t n_tiles = window_n_tiles(entries);
	if ((uint64_t)p.block_w * p.block_h * channels > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "tile too large");
	// the reader's scratch as pxz_decode_windows_device laid it out for these windows (reader_scratch)
	if (h->dmeta.cap < (size_t)n_tiles * 16u)
		return fail(h, PXZ_ERR_INVALID_ARG, "the splice reads the record bounds pxz_decode_windows_device leaves: call it with these windows on this handle first");

	// ---- the structure of every new file: its pieces in file order, its touched tile rows
	std::vector<std::vector<uint32_t>> of_image(n_images);
	for (uint32_t k = 0; k < n_windows; ++k) of_image[entries[k].image].push_back(k);
	std::vector<pxz::SplicePiece> pieces;
	std::vector<pxz::SpliceRow> rows;
	std::vector<pxz::SpliceRowPart> parts;
	for (uint32_t i = 0; i < n_images; ++i) {
		const std::vector<uint32_t> &ws = of_image[i];
		if (ws.empty()) {  // no window: the file as it is
			pieces.push_back({{SpliceBound::kFileStart, i, 0}, {SpliceBound::kFileEnd, i, 0}, i, 1u});
			continue;
		}
		const uint32_t any = ws[0], n_rows = entries[any].rows;
		// the header and the line table (the touched rows' lengths are written over their copies), then what lies between the windows
		SpliceBound cursor{SpliceBound::kRow, any, 0};
		pieces.push_back({{SpliceBound::kFileStart, i, 0}, cursor, i, 1u});
		std::map<uint32_t, std::vector<std::pair<uint32_t, uint32_t>>> touched;  // tile row -> (first covered column, window)
		for (uint32_t k : ws)
			for (uint32_t j = 0; j < entries[k].crows; ++j) touched[entries[k].r0 + j].push_back({entries[k].c0, k});
		for (auto &row : touched) {
			const uint32_t r = row.first;
			std::sort(row.second.begin(), row.second.end());
			rows.push_back({i, any, r, (uint32_t)parts.size(), (uint32_t)row.second.size()});
			for (const auto &cw : row.second) {
				const pxz::WindowEntry &e = entries[cw.second];
				const uint32_t j = r - e.r0, t0 = e.tile0 + j * e.ccols, t1 = t0 + e.ccols - 1u;
				const bool at_row_start = cursor.kind == SpliceBound::kRow && cursor.b == r && e.c0 == 0;
				if (!at_row_start) pieces.push_back({cursor, {SpliceBound::kRecStart, t0, 0}, i, 0u});
				pieces.push_back({{SpliceBound::kStageRow, cw.second, j}, {SpliceBound::kStageRow, cw.second, j + 1u}, i, 0u});
				parts.push_back({cw.second, j});
				cursor = e.c0 + e.ccols == e.cols ? SpliceBound{SpliceBound::kRow, any, r + 1u} : SpliceBound{SpliceBound::kRecEnd, t1, 0};
			}
		}
		if (!(cursor.kind == SpliceBound::kRow && cursor.b == n_rows)) pieces.push_back({cursor, {SpliceBound::kFileEnd, i, 0}, i, 0u});
	}
	if (pieces.size() > 0xffffffffull || parts.size() > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 pieces in the spliced files");

	PXZ_HIP(h, hipSetDevice(h->device));
	// ---- the new records: the hulls as a varied batch through the writer, one staging file per window
	std::vector<pxz_image_desc> hulls(n_windows);
	uint64_t stage_cap = 0;
	for (uint32_t k = 0; k < n_windows; ++k) {
		const pxz::WindowEntry &e = entries[k];
		const uint64_t x1 = std::min<uint64_t>((uint64_t)(e.c0 + e.ccols) * p.block_w, e.img_w), y1 = std::min<uint64_t>((uint64_t)(e.r0 + e.crows) * p.block_h, e.img_h);
		const uint32_t hw = (uint32_t)(x1 - (uint64_t)e.c0 * p.block_w), hh = (uint32_t)(y1 - (uint64_t)e.r0 * p.block_h);
		hulls[k] = pxz_image_desc{hw, hh, hw * channels, 0, 0};
		stage_cap += 26u + 4ull * e.crows;
	}
	stage_cap += (uint64_t)n_tiles * (13u + pxz_qoi_bound(p.block_w, p.block_h, channels));
	const size_t n_pieces = pieces.size();
	const uint64_t src_at = 0, len_at = src_at + 8ull * n_pieces, dst_at = len_at + 8ull * n_pieces, so_at = dst_at + 8ull * (n_pieces + 1u),
	               fl_at = so_at + 8ull * ((uint64_t)n_windows + 1u);
	if ((rc = ensure(h, h->splice_work, fl_at + 4ull * n_images)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->splice_stage, stage_cap)) != PXZ_OK) return rc;
	uint8_t *work = (uint8_t *)h->splice_work.ptr;
	uint64_t *d_stage_offsets = (uint64_t *)(work + so_at);
	if ((rc = encode_varied(h, hulls.data(), n_windows, channels, &p, 0u, d_block_value, d_tile_w, d_tile_h, d_slots, (uint8_t *)h->splice_stage.ptr,
	                        stage_cap, d_stage_offsets, nullptr)) != PXZ_OK)
		return rc;

	// ---- the tables up, the splice
	const size_t rows_at = up256(n_pieces * sizeof(pxz::SplicePiece)), parts_at = rows_at + up256(rows.size() * sizeof(pxz::SpliceRow));
	const size_t table_bytes = parts_at + up256(parts.size() * sizeof(pxz::SpliceRowPart));
	std::vector<uint8_t> table(table_bytes);
	std::memcpy(table.data(), pieces.data(), n_pieces * sizeof(pxz::SplicePiece));
	if (!rows.empty()) std::memcpy(table.data() + rows_at, rows.data(), rows.size() * sizeof(pxz::SpliceRow));
	if (!parts.empty()) std::memcpy(table.data() + parts_at, parts.data(), parts.size() * sizeof(pxz::SpliceRowPart));
	if ((rc = ensure(h, h->splice, table_bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, h->splice_table.send(table.data(), table_bytes, h->splice.ptr, h->stream));
	pxz::SpliceArgs s{};
	if ((rc = window_upload(h, entries, &s.windows)) != PXZ_OK) return rc;
	s.n_windows = n_windows;
	s.n_images = n_images;
	s.n_tiles = n_tiles;
	s.n_pieces = (uint32_t)n_pieces;
	s.n_rows = (uint32_t)rows.size();
	s.pieces = (const pxz::SplicePiece *)h->splice.ptr;
	s.rows = (const pxz::SpliceRow *)((const uint8_t *)h->splice.ptr + rows_at);
	s.parts = (const pxz::SpliceRowPart *)((const uint8_t *)h->splice.ptr + parts_at);
	s.files = d_files;
	s.file_offsets = (const unsigned long long *)d_file_offsets;
	s.rec_off = (const unsigned long long *)h->dmeta.ptr;
	s.rec_len = (const uint32_t *)((const uint8_t *)h->dmeta.ptr + (size_t)n_tiles * 8u);
	s.new_w = d_tile_w;
	s.new_h = d_tile_h;
	s.reader_flags = d_reader_flags;
	s.patch_flags = d_patch_flags;
	s.stage = (const uint8_t *)h->splice_stage.ptr;
	s.stage_offsets = (const unsigned long long *)d_stage_offsets;
	s.stage_capacity = stage_cap;
	s.piece_src = (unsigned long long *)(work + src_at);
	s.piece_len = (unsigned long long *)(work + len_at);
	s.piece_dst = (unsigned long long *)(work + dst_at);
	s.image_flags = d_image_flags ? d_image_flags : (uint32_t *)(work + fl_at);
	s.out = d_out;
	s.capacity = out_capacity;
	s.out_file_offsets = (unsigned long long *)d_out_file_offsets;
	PXZ_HIP(h, hipMemsetAsync(s.image_flags, 0, 4ull * n_images, h->stream));
	PXZ_HIP(h, pxz::launch_splice(s, h->n_cus, h->stream));
	return PXZ_OK;
}

}  // extern "C"
