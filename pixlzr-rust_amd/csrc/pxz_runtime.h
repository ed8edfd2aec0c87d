// pxz_runtime.h — what the host runtime (pxz_api.cpp) shares with the host forms (pxz_host_forms.cpp): the handle, the
// error helpers, and the checks and plans that a form runs before it composes the device entry points.  The functions are
// defined in pxz_api.cpp.  Of the handle the host forms touch the scratch buffers, `stream` and `device`, nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/pixlzr_hip.h"
#include "pxz_handle.h"
#include "pxz_internal.h"

namespace pxz_runtime __attribute__((visibility("hidden"))) {  // shared between the library's units, no exported symbols

using pxz::AxisTab;
using pxz::DeviceBuffer;
using pxz::kMaxLevel;
using pxz::PinnedStaging;

// device copy of the down-scaling tables for one (tile geometry, filter): pxz::ShrinkTableSet
struct TableSet {
	DeviceBuffer mem;  // the one allocation behind every device pointer below
	std::vector<AxisTab> tabs;  // host copy, passed by value in the kernel arguments
	uint16_t *d_bounds = nullptr;
	uint32_t *d_coeffs = nullptr;
	int32_t *d_ksums = nullptr;
	uint32_t *d_rows = nullptr;
	uint32_t rows_dw = 0;
	uint32_t *d_mf64 = nullptr;  // 64x64 fast path: matrix-core operand tables (null: not available)
	bool opaque_stays = true;    // a constant-255 alpha comes back as 255 from every window of every table
};

// decode side: up-scaling tables of every source size to the full tile size (expand_kernel): pxz::ExpandTableSet
struct ExpandTables {
	DeviceBuffer mem;  // the one allocation behind every device pointer below
	pxz::ExpandTab *d_dir = nullptr;
	uint16_t *d_starts = nullptr, *d_sizes = nullptr;
	int16_t *d_coeffs = nullptr;
	uint32_t dir_stride = 0;
	uint32_t *d_xmf = nullptr;  // 32x32 tiles, convolutions: matrix-core operand tables (pxz_internal.h: kXmfDw)
	uint32_t *d_xmf16 = nullptr;  // 16x16 tiles, convolutions: the same for expand16_kernel (kXmf16Dw)
	uint32_t *d_xmf64 = nullptr;  // 64x64 tiles, convolutions: the same for expand64_kernel (kXmf64Dw)
};

// tree::process on rectangle lists: every axis table (down with the one filter, back up with the other) of every tile
// size the recursion can reach from one (frame, block, minimum) geometry: pxz::TreeTableSet
struct TreeTables {
	DeviceBuffer mem;  // the one allocation behind every device pointer below
	pxz::TreeAxisEntry *d_dir = nullptr;
	int32_t *d_starts = nullptr, *d_sizes = nullptr;
	int16_t *d_coeffs = nullptr;
	uint32_t n_dir = 0;
};

// batches of differently sized images: the axis tables of every (source size, level) pair of one batch: pxz::VariedTableSet
struct VariedTables {
	DeviceBuffer mem;  // the one allocation behind every device pointer below
	pxz::TreeAxisEntry *d_dir = nullptr;
	int32_t *d_starts = nullptr, *d_sizes = nullptr;
	int16_t *d_coeffs = nullptr;
};

// decode side of varied batches: the up-scaling table of every (full size, stored size) pair of one batch: pxz::VariedExpandTableSet
struct VariedExpandTables {
	DeviceBuffer mem;  // the one allocation behind every device pointer below
	uint32_t *d_slot = nullptr;
	pxz::ExpandTab *d_dir = nullptr;
	uint16_t *d_starts = nullptr, *d_sizes = nullptr;
	int16_t *d_coeffs = nullptr;
	uint32_t stride = 0, max_window = 0;
};

// decode at reduced scale: the axis table of every (target size, stored size) pair of one call: pxz::ScaledExpandTableSet
struct ScaledExpandTables {
	DeviceBuffer mem;  // the one allocation behind every device pointer below
	uint32_t *d_slot = nullptr;
	pxz::ScaledTab *d_dir = nullptr, *d_mixed = nullptr;
	uint16_t *d_starts = nullptr, *d_sizes = nullptr;
	int16_t *d_coeffs = nullptr;
	uint32_t stride = 0, max_win_dw = 0;
};

// The bounded caches hold at most this many table sets: caches, not logs -- varying geometries (tools/fuzz_tree.py, a
// folder of many sizes) must not grow them without bound.
constexpr size_t kTableCacheBound = 16;

// Everything of a handle that pxz_trim gives back: assigning a fresh HandleScratch releases all of it, so a member
// added here can be forgotten neither by pxz_trim nor by pxz_destroy.
struct HandleScratch {
	DeviceBuffer in, val, ow, oh, out, sums, chunks, work, qscratch, qmeta, status, dmeta, okscratch, rgba, slots4, pk, pkoff, tree, xlist, bigscratch;
	uint64_t packed_len = 0;   // bytes of the stream pxz_shrink_image_packed left in `pk` (0: none)
	static constexpr int kRing = 3;  // buffer sets of the pipelined host boundary (pxz_shrink_images*)
	DeviceBuffer ring_in[kRing], ring_val[kRing], ring_ow[kRing], ring_oh[kRing], ring_out[kRing], ring_pk[kRing], ring_pkoff[kRing];
	std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, TreeTables> tree_tables;
	DeviceBuffer tree_rects[2], tree_count;
	DeviceBuffer ladder;              // factor ladder: the raw detector value of every tile, then the rungs' factors
	PinnedStaging ladder_factors;     //   pinned staging of the factors (PXZ_LADDER_MAX_RUNGS floats)
	DeviceBuffer varied, varied_in, varied_out, varied_files;  // varied batches: the per-image table, the host forms' images,
	                                  //   tiles and files
	PinnedStaging varied_images;      // pinned staging of the per-image table
	std::map<std::pair<uint32_t, std::vector<uint32_t>>, VariedTables> varied_tables;  // (filter, tile sides) -> tables
	std::map<std::pair<uint32_t, std::vector<uint32_t>>, VariedExpandTables> varied_expand_tables;  // the same for the decode side
	DeviceBuffer varied_flags;        // per-image flags of a varied decode-side call whose caller passed none
	DeviceBuffer rd;                  // the rate-distortion and fit forms (pxz_host_forms.cpp): the rung table and what goes down with it
	DeviceBuffer windows;             // pixel windows of files: the per-window table
	PinnedStaging window_table;       //   and its pinned staging
	DeviceBuffer window_host;         // the windows form: the files, the covered tiles, the crops and the flags
	std::map<std::pair<uint32_t, std::vector<uint32_t>>, ScaledExpandTables> scaled_tables;  // (filter, target / largest stored size pairs)
	DeviceBuffer scaled;              // decode at reduced scale: the per-owner table
	PinnedStaging scaled_table;       //   and its pinned staging
	DeviceBuffer splice, splice_work, splice_stage;  // pxz_splice_windows_device: the piece, row and part tables; the pieces' offsets, the
	                                  //   images' flags and the staging files' offsets; the staging files (the hulls' records)
	PinnedStaging splice_table;       //   pinned staging of the tables
	DeviceBuffer patch_host;          // the patch form: the files, the patches, the covered tiles, the flags and the new files' offsets
	DeviceBuffer transcode_files, transcode_tiles;  // the transcode and archive forms: the files that come in; their tiles when the block size changes
	DeviceBuffer fit;                 // pxz_fit_varied_ladder_device: the images' targets
	PinnedStaging fit_targets;        //   and their pinned staging
	DeviceBuffer fit_tiles;           // the fit forms: the chosen rungs' tiles
	DeviceBuffer archive_tiles;       // the archive forms: the archive's own tiles (the reference of the distortion call) and the flags of
	                                  //   the reader and the re-shrink
	DeviceBuffer record_offsets;      // pxz_record_bytes_varied_device: the files' offsets of a caller that passed none
	DeviceBuffer tilefit;             // pxz_fit_varied_tiles_device: the groups' table, the packed candidates, intervals and totals
	PinnedStaging tilefit_table;      //   pinned staging of the groups' table (targets, fixed bytes, first tiles)
	DeviceBuffer tilefit_tables;      // the tile-fit forms: every rung's record bytes and per-tile errors
	DeviceBuffer tilefit_down;        //   and what comes down with the files' offsets: the choices and the groups' results
	bool work_ready = false;   // both worklist counters are zero / consistent with work_slot
	const uint32_t *qbins_clean = nullptr;  // the writer's binning counters at this address were left zeroed by the last launch_qoi
	const uint32_t *dbins_clean = nullptr;  // the same for the reader's (launch_decode)
};

}  // namespace pxz_runtime

struct pxz_handle : pxz_runtime::HandleScratch {
	int device = 0;
	uint32_t n_cus = 256;
	hipStream_t stream = nullptr;
	std::string error;
	float thresholds[pxz::kNumThresholds];
	std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, pxz_runtime::TableSet> tables;
	// level breakpoints per (mode, factor bits, bw, bh, edge_w, edge_h)
	struct Breaks { uint32_t b[4][pxz::kMaxLevel]; uint32_t asc[4]; };
	std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, Breaks> breaks;
	std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, pxz_runtime::ExpandTables> expand_tables;
	bool quiet_stats = false;         // the launch being set up writes no kernel-selection statistics (the ladder's detector)
	uint32_t *host_stats = nullptr;  // pinned, device-visible: [0] = tiles with transparency the last finished 32x32 launch saw
	uint32_t *dev_stats = nullptr;   //   (its device-side address); read without synchronisation, steers only the kernel choice
	uint32_t last_alpha_kernel = 0, last_alpha_first = 0;  // what the last launch set up through this handle chose (pxz_handle_state)
	uint32_t work_slot = 0;    // the counter the next 32x32 launch uses
	bool timing = false;
	uint32_t timing_stride = 1, timing_count = 0;  // every stride-th step is bracketed by events
	std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
	std::vector<hipEvent_t> mid_events;  // one per pair: behind the first kernel of the step
	size_t events_used = 0;
};

#define PXZ_HIP(h, call)                                                                      \
	do {                                                                                      \
		hipError_t e_ = (call);                                                               \
		if (e_ != hipSuccess) return pxz_runtime::fail((h), PXZ_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
	} while (0)

namespace pxz_runtime __attribute__((visibility("hidden"))) {

// the next multiple of 256: the alignment of what shares a device allocation
constexpr uint64_t up256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

// sets pxz_last_error (h may be null: a call without a handle) and returns code
int fail(pxz_handle *h, int code, const char *fmt, ...);
int ensure(pxz_handle *h, DeviceBuffer &b, size_t bytes);

int check_params(pxz_handle *h, const pxz_params *p);
int varied_check_params(pxz_handle *h, uint32_t channels, const pxz_params *p);
int check_factors(pxz_handle *h, const float *factors, uint32_t n_factors, uint32_t max_rungs);
int fit_check(pxz_handle *h, uint32_t n_images, uint32_t n_factors, uint32_t channels, uint32_t criterion);
int tile_groups_check(pxz_handle *h, const uint32_t *group_first, uint32_t n_groups, uint32_t n_images);

pxz_params decode_side_params(const pxz_params *params, bool with_filter);
int file_header(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint32_t *block_w, uint32_t *block_h, uint32_t *channels,
                uint32_t *filter_byte, const char **why);
int varied_plan(pxz_handle *h, const pxz_image_desc *d, uint32_t n, uint32_t bw, uint32_t bh, uint32_t channels, uint32_t mode,
                std::vector<pxz::VariedImage> *images, std::vector<uint32_t> *sides, uint32_t *n_rows);
uint32_t varied_n_tiles(const std::vector<pxz::VariedImage> &images);
int window_plan(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *w, uint32_t n_windows, uint32_t bw,
                uint32_t bh, uint32_t channels, std::vector<pxz::WindowEntry> *entries, std::vector<uint32_t> *sides, uint32_t *n_rows);
uint32_t window_n_tiles(const std::vector<pxz::WindowEntry> &entries);
// window_plan with the patch's rule on top: the covered tile rectangles of one image are pairwise disjoint (pxz_patch_check)
int patch_plan(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *w, uint32_t n_windows, uint32_t bw, uint32_t bh,
               uint32_t channels, std::vector<pxz::WindowEntry> *entries, std::vector<uint32_t> *sides, uint32_t *bad_window);
// decode at reduced scale: the rules of one owner's scale (s | block, "image i" / "window k") and a window's alignment, and
// the scaled size of a full-resolution extent
int scaled_check_shift(pxz_handle *h, const char *who, uint32_t index, uint32_t shift, uint32_t bw, uint32_t bh);
int scaled_check_window(pxz_handle *h, uint32_t index, const pxz_window &w, uint32_t img_w, uint32_t img_h, uint32_t shift);
inline uint32_t scaled_extent(uint32_t v, uint32_t shift) { return (uint32_t)(((uint64_t)v + (1ull << shift) - 1u) >> shift); }
int stage_host_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t pitch_bytes,
                     pxz_params *p, uint32_t sets, bool device_px, pxz_frames *f, size_t *tiles, size_t *slot);
int reshrink_check_block(pxz_handle *h, uint32_t mode, uint32_t bw, uint32_t bh, uint32_t rung_channels, uint32_t wdw);
uint64_t reshrink_distortion_bytes(uint32_t bw, uint32_t bh, uint32_t wdw);

}  // namespace pxz_runtime
