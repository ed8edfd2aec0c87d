// pxz_shrink_plan.h — the route of one single-geometry shrink call (pxz_shrink_frames_device, pxz_lod_frames_device, the ladder's
// first stage, process(), tree::process and every host image form), decided ONCE by pure host code: no HIP, no handle.
// run_shrink (pxz_api.cpp) executes a ShrinkRoute; pxz_shrink_plan_check.cpp holds the plan to its rules on the CPU
// (tests/test_shrink_plan_host.py).  Every predicate of the route is defined here once and used by name elsewhere.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/pixlzr_hip.h"
#include "pxz_internal.h"

namespace pxz {

constexpr uint64_t kShrinkLdsLimit = 160u * 1024u;   // LDS of one CU: what a block's tile image is held against
constexpr uint32_t kBigTilePixels = 1u << 20;       // the HBM-resident form's index arithmetic holds below this many pixels per tile
constexpr uint64_t kShrinkMaxTiles = 0xffffffffull;  // tile ids are 32-bit
constexpr uint32_t kAlphaKernelTiles = 2048;         // tiles with transparency past which shrink32a_kernel pays for its launch

// ---- predicates, one copy each ------------------------------------------------------------------------------------------

// bytes between frames; the descriptor's stride only counts in a batch of more than one frame
inline uint64_t frame_stride_of(const pxz_frames &f) { return f.n_frames > 1 ? f.frame_stride_bytes : (uint64_t)f.pitch_bytes * f.height; }
// what decides whether every row of every frame starts on a multiple of 16 (RGBA fast kernels, block-cooperative detector) or of
// 4 (RGB read natively): the low address bits, the pitch, and the stride where there is a second frame
inline uint64_t alignment_bits(uint32_t src_low_bits, const pxz_frames &f) { return src_low_bits | f.pitch_bytes | (f.n_frames > 1 ? f.frame_stride_bytes : 0u); }
inline bool rows_aligned16(uint32_t src_low_bits, const pxz_frames &f) { return (alignment_bits(src_low_bits, f) & 15u) == 0; }
inline bool rows_aligned4(uint32_t src_low_bits, const pxz_frames &f) { return (alignment_bits(src_low_bits, f) & 3u) == 0; }
// the tile sizes with kernels of their own (shrink16/32/64_kernel, the square Oklab detectors), either mode
inline bool square_fast(uint32_t bw, uint32_t bh) { return bw == bh && (bw == 16 || bw == 32 || bw == 64); }
// the tiles the Oklab detector with run-time geometry takes: rows of whole pixel quads, 64 .. 16384 pixels (the squares are among them)
inline bool oklab_shape(uint32_t mode, uint32_t bw, uint32_t bh)
{
	return mode == PXZ_MODE_SHRINK_BY && bw % 4u == 0 && (uint64_t)bw * bh >= 64u && (uint64_t)bw * bh <= 16384u;
}
// ... and only those that have no square detector: what PXZ_NO_OKLAB_GENERAL takes away
inline bool general_oklab(uint32_t mode, uint32_t bw, uint32_t bh, const Knobs &k) { return !square_fast(bw, bh) && oklab_shape(mode, bw, bh) && !k.no_oklab_general; }
// "covers every tile": on RGBA frames of this shape the interior and edge launches of the Oklab detector leave no tile to the
// generic kernel's own detector, whose f32 planes the LDS layout then drops (no_lab).  Any knob that could take a launch away
// says no, and so does a frame smaller than a block: the detector's loads are unconditional (INVARIANT B below).
inline bool oklab_covers_rgba(const pxz_frames &f, const pxz_params &p, const Knobs &k)
{
	return oklab_shape(p.mode, p.block_w, p.block_h) && f.width >= p.block_w && f.height >= p.block_h && !k.no_oklab32 && !k.no_oklab_general &&
	       !k.no_oklab_edges && !k.no_repitch;
}
// waves per tile of the generic kernel (pxz_shrink_generic.hip has waves_per_tile for the launch; the check program compares nothing
// on the device, so the layout carries its own statement of the five steps)
constexpr uint32_t layout_waves(uint32_t px) { return px <= 1024u ? 1u : px <= 2048u ? 2u : px <= 4096u ? 4u : px <= 8192u ? 8u : 16u; }

// ---- the tile grid --------------------------------------------------------------------------------------------------------

struct TileGrid {
	uint32_t cols = 0, rows = 0;
	uint32_t edge_w = 0, edge_h = 0;  // the last column's width, the last row's height
	uint32_t tiles_per_frame = 0;
	uint64_t tiles = 0;               // of all frames
};
// pxz_grid's grid (sides up to 2^24, blocks of at least 1)
inline TileGrid tile_grid(uint32_t width, uint32_t height, uint32_t bw, uint32_t bh, uint32_t n_frames)
{
	TileGrid g;
	g.cols = (uint32_t)(((uint64_t)width + bw - 1u) / bw);
	g.rows = (uint32_t)(((uint64_t)height + bh - 1u) / bh);
	g.edge_w = width - (g.cols - 1) * bw;
	g.edge_h = height - (g.rows - 1) * bh;
	g.tiles_per_frame = g.cols * g.rows;
	g.tiles = (uint64_t)g.cols * g.rows * n_frames;
	return g;
}

// ---- the LDS image of one tile of the generic kernel (and of ladder_kernel, which has no detector planes) ---------------------

struct ShrinkLayout {
	uint32_t rs, plane_dw, hps, tmp_dw, lab_dw, tile_dw;  // as ShrinkArgs
	uint64_t lds_bytes;   // the image and, for more than one wave, the waves' partial sums
	uint32_t big_blocks;  // 0: the image is in LDS; else the blocks of the HBM-resident form, before the cap by the tile count
	bool refused;         // beyond LDS and not runnable from HBM (2^20 pixels or more, PXZ_NO_BIG_TILES)
	bool in_lds() const { return lds_bytes <= kShrinkLdsLimit; }
};
// conv: pixels are wanted and the filter is a convolution; lab: the generic kernel keeps its own detector's f32 planes
ShrinkLayout shrink_layout(uint32_t bw, uint32_t bh, bool conv, bool lab, uint32_t n_cus, const Knobs &k);

// Whether pxz_shrink_ladder_frames_device runs ladder_kernel: shrink_by, and both the kernel's own image (*bare: no detector
// planes) and the single-factor call's (with them, so that one rung alone is sure to run too) are in LDS.  tiles: of the batch.
bool shrink_ladder_in_lds(const pxz_params &p, bool want_pixels, uint64_t tiles, uint32_t n_cus, const Knobs &k, ShrinkLayout *bare);

// ---- the route ------------------------------------------------------------------------------------------------------------

struct ShrinkRequest {
	const pxz_frames *frames;   // (checked by the caller: check_frames)
	const pxz_params *params;
	bool want_pixels;           // tile slots are written
	bool identity;              // the closures of process(): factor 1, scale 1
	uint32_t src_low_bits;      // the low four bits of the frames' device address
	uint32_t n_cus;
	bool have_stats;            // the handle has its pinned statistics
	uint32_t stats[3];          //   [0] tiles with transparency, [1] listed tiles of the last finished launch, [2] its signature
	bool quiet_stats;           // this launch writes no statistics (the ladder's detector)
	bool opaque_stays;          // TableSet::opaque_stays; read only when shrink_plan_needs_opaque_stays says so
};

enum class ShrinkInput : uint32_t { AsGiven, Widened, Repitched };  // Widened: RGBA in h->rgba, slots in h->slots4, narrowed afterwards
enum class ShrinkDetector : uint32_t { None, Rgba, RgbNative };      // the block-cooperative Oklab detector's launches ahead of the shrink

struct ShrinkRegion {  // one ragged edge of the grid through the detector with run-time geometry
	uint32_t id, bit;       // ShrinkArgs::ok_region, its bit in ok_edges
	bool wanted;
	uint32_t count, bands;  // tiles it enumerates, 256-px bands per tile
};

struct ShrinkRoute {
	ShrinkInput input;
	pxz_frames frames;       // what the kernels see (Widened, Repitched: tight RGBA rows of a 16-byte multiple)
	uint32_t channels;
	uint64_t frame_stride;
	size_t rgba_bytes;       // h->rgba for Widened / Repitched, else 0
	size_t slots4_bytes;     // h->slots4 for Widened with pixels, else 0
	TileGrid grid;
	ShrinkLayout layout;
	float factor, scale2;
	// detector
	ShrinkDetector detector;
	uint32_t ok_bands, ok_rows, clone_ahead;
	ShrinkRegion regions[3];
	size_t okscratch_bytes;
	// the fast kernels' region: tile (tx, ty) is theirs iff tx < full_cols && ty < full_rows
	uint32_t full_cols, full_rows;
	// transparency
	uint32_t alpha_kernel, alpha_first, stats_sig, expect_listed;
	bool write_stats;
	// scratch
	size_t sums_bytes, work_bytes, work_total_bytes, bigscratch_bytes;
	uint32_t big_blocks;     // layout.big_blocks capped by the tile count

	uint32_t ok_edges() const { return (regions[0].wanted ? 1u : 0u) | (regions[1].wanted ? 2u : 0u) | (regions[2].wanted ? 4u : 0u); }
};

// Whether the plan will read ShrinkRequest::opaque_stays: an RGB batch on a widenable shape that is not read natively, pixels
// wanted, a convolution -- and no refusal that comes before the tables in the order of checks.
bool shrink_plan_needs_opaque_stays(const ShrinkRequest &q, const Knobs &k);

// PXZ_OK and *route, or the code of the refusal with its text in `text` (the caller's frames and params have passed check_frames).
int shrink_plan(const ShrinkRequest &q, const Knobs &k, ShrinkRoute *route, char *text, size_t text_len);

}  // namespace pxz
