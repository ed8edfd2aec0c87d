#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "pxz_internal.h"

namespace pxz {

struct AxisWindows {
	uint32_t in_size = 0, out_size = 0;
	int window = 0, precision = 0;
	std::vector<int32_t> starts, sizes;
	std::vector<int16_t> coeffs;  // out_size * window (empty for Nearest)
};

// filter: FilterType repr(u8) 0..4.  false for an unknown filter.  upscale: the flag PixlzrBlock::resize
// passes to to_fir_resizing_algorithm (block.rs:301-304) -- it only changes the kernel of Triangle.
bool build_axis(uint32_t in_size, uint32_t out_size, uint32_t filter, AxisWindows *out, bool upscale = false);

// thresholds[k] = smallest positive float v with round(log2f(v)) >= -k
bool build_level_thresholds(float *thresholds, int count);

// ---- host images of the device tables (layouts: pxz_internal.h).  The builders never call HIP and return false for an
// unknown filter; empty arrays stay empty (no device copy, a null pointer), the others are never empty.
// the generic kernel's down-scaling tables for one (tile geometry, filter)
struct ShrinkTableSet {
	std::vector<AxisTab> tabs;  // 2 axes x {full, ragged edge} x kMaxLevel, passed by value in the kernel arguments
	std::vector<uint16_t> bounds;
	std::vector<uint32_t> coeffs;
	std::vector<int32_t> ksums;
	std::vector<uint32_t> rows;  // unified rows, the 32x32 / 16x16 operand tables (AxisTab::mf_off), then 32 dwords of padding
	std::vector<uint32_t> mf64;  // 64x64 tiles: shrink64_kernel's operand tables of every level (empty: not available)
	bool opaque_stays = true;    // a constant-255 alpha comes back as 255 from every window of every table
};
bool build_shrink_tables(uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t filter, ShrinkTableSet *out);

// decode side: up-scaling tables of every source size to the full tile size (expand_kernel)
struct ExpandTableSet {
	std::vector<ExpandTab> dir;  // [(axis * 2 + class) * dir_stride + source size]
	uint32_t dir_stride = 0;
	std::vector<uint16_t> starts, sizes;
	std::vector<int16_t> coeffs;
	std::vector<uint32_t> xmf;    // 32x32 tiles, convolutions: kXmfLevels * kXmfDw (empty: not available)
	std::vector<uint32_t> xmf16;  // 16x16 tiles, convolutions: kXmf16Levels * kXmf16Dw
	std::vector<uint32_t> xmf64;  // 64x64 tiles, convolutions: kXmf64Levels * kXmf64Dw
};
bool build_expand_tables(uint32_t bw, uint32_t bh, uint32_t edge_w, uint32_t edge_h, uint32_t filter, ExpandTableSet *out);

// tree::process on rectangle lists: every axis table (down with `filter`, back up with `filter_upscale`) between each tile
// size the recursion over `levels` (block sizes, level by level) reaches in a width x height frame and its reduced sizes
struct TreeTableSet {
	std::vector<TreeAxisEntry> dir;
	std::vector<int32_t> starts, sizes;
	std::vector<int16_t> coeffs;
};
bool build_tree_tables(uint32_t width, uint32_t height, const std::vector<std::pair<uint32_t, uint32_t>> &levels, uint32_t filter,
                       uint32_t filter_upscale, TreeTableSet *out);

// batches of differently sized images (varied_kernel): the down-scaling table of every (source size, level) pair the batch's
// tiles can reach, dir[in * kMaxLevel + m] for in in `sizes` (tile widths and heights: the full block sides and every
// distinct edge) and m = 1 .. kMaxLevel - 1; entries of other sizes, of level 0 and of levels that keep the size are zero.
// One table per (in, out) pair, shared by the levels and axes that reach it.
struct VariedTableSet {
	std::vector<TreeAxisEntry> dir;  // (max(sizes) + 1) * kMaxLevel
	std::vector<int32_t> starts, sizes;
	std::vector<int16_t> coeffs;
};
bool build_varied_tables(const std::vector<uint32_t> &sizes, uint32_t filter, VariedTableSet *out);

// decode side of varied batches (varied_expand_kernel): one up-scaling table per (full size, stored size) pair, for every full
// size in `sizes` (the block sides and each distinct edge width and height of the batch) and stored sizes 1 .. full - 1:
// dir[slot[full] * stride + stored].  Each table is the one build_expand_tables makes for that pair (the same per-axis code);
// one table serves both axes.  Entries of stored == full (a clone) and of sizes that are not in the batch are zero.
struct VariedExpandTableSet {
	std::vector<uint32_t> slot;  // per full size 0 .. max(sizes): its row in dir (0xffffffff: not a size of the batch)
	uint32_t stride = 0;         // max(sizes) + 1
	std::vector<ExpandTab> dir;
	std::vector<uint16_t> starts, sizes;
	std::vector<int16_t> coeffs;
	uint32_t max_window = 0;     // widest window of the set (sizes the kernel's staged windows)
};
bool build_varied_expand_tables(const std::vector<uint32_t> &sizes, uint32_t filter, VariedExpandTableSet *out);

// decode at reduced scale (pxz_scaled_expand.hip): one axis table per (target size, stored size) pair the call can meet -- for
// target targets[i] the stored sizes 1 .. max_stored[i] but the target itself (an axis that keeps its size is not resampled):
// dir[slot[target] * stride + stored], stride = max(max_stored) + 1.  A table whose axis grows is the one
// build_varied_expand_tables makes for the pair; one whose axis shrinks is built without the upscale flag in `dir` and with it
// in `mixed` (the other axis of the tile grows: block.rs:301-304 hands one flag to both) -- another kernel for Triangle, the
// same entry for the other filters.  One table serves both axes.  Entries of pairs the call cannot meet are zero.
struct ScaledExpandTableSet {
	std::vector<uint32_t> slot;  // per target size 0 .. max(targets): its row in dir (0xffffffff: not a target of the call)
	uint32_t stride = 0;
	std::vector<ScaledTab> dir, mixed;
	std::vector<uint16_t> starts, sizes;
	std::vector<int16_t> coeffs;
	uint32_t max_taps = 0;       // widest window of the set as built
	uint32_t max_win_dw = 0;     // most dwords the staged windows of one axis take: max over the tables of target * wdw
};
bool build_scaled_expand_tables(const std::vector<uint32_t> &targets, const std::vector<uint32_t> &max_stored, uint32_t filter,
                                ScaledExpandTableSet *out);
// the support of a filter's kernel in source samples at scale 1 (0: Nearest; Triangle's two kernels share theirs)
uint32_t filter_support(uint32_t filter);

}  // namespace pxz
