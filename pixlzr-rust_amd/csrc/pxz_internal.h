// pxz_internal.h — structures shared by the host runtime and the gfx950 kernels.
#pragma once
#include <stdint.h>

namespace pxz {

constexpr int kMaxLevel = 18;        // level exponents 0..17 (2^17 > any LDS-resident tile side)
constexpr int kNumThresholds = 32;   // float thresholds for round(log2f(v)) >= -k, k = 0..31
constexpr int kWave = 64;

// One down-scaling table along one axis: in_size -> out_size.
// Convolution (windows padded to whole quads of 4 source samples, zero weights in the padding):
//   bounds[bounds_off + 2*o]     first quad (source index / 4) of output o
//   bounds[bounds_off + 2*o + 1] number of quads
//   coeffs[coeff_off + o*wquads*2 + 2*q + {0,1}]  packed i16 pairs (k0 | k1<<16), (k2 | k3<<16)
//   ksums[ksum_off + o]          sum of the window's weights (constant-input shortcut)
// Nearest: bounds[bounds_off + o] = source index.
struct AxisTab {
	uint32_t bounds_off;
	uint32_t coeff_off;
	uint32_t ksum_off;
	uint32_t rows_off;       // unified rows (fast path): per output row_stride dwords =
	uint32_t row_stride;     //   {first quad, quads, weight sum, 0} + wquads*2 packed pairs, 16-B aligned
	uint16_t out_size;
	uint16_t wquads;
	uint16_t precision;
	uint16_t in_size;
	uint32_t mf_off;         // matrix-core operand table of a 32 -> 16|8 axis (dword offset in the rows blob, 0: none)
};

// Matrix-core operand table of one 32 -> out axis (out = 16 or 8), kMfDwords dwords, see resample_mfma32:
//   [0, 128)    low bytes  of the weights: lane l = (o = l & 15, g = l >> 4), 8 x i8 = K_lo[o][src(g, j)]
//   [128, 256)  high bytes of the weights, same arrangement (K = 256 * K_hi + K_lo, both signed 8-bit)
//   [256, 272)  bias[o]  = 128 * sum_i K[o][i] + 2^(precision - 1)
//   [272, 288)  ksum[o]  = sum_i K[o][i]
//   [288]       1 if clip8(2^(precision-1) + 255 * ksum[o]) == 255 for every o (opaque stays opaque)
// src(g, j) = 4g + j (j < 4), 16 + 4g + (j - 4) (j >= 4): the order in which the first product's
// accumulator registers hand their rows to the second product.
constexpr uint32_t kMfDwords = 292;
// Matrix-core operand table of one 16 -> out axis (out = 8, 4, 2 or 1; resample_group16_mfma): dwords [0..31] the low weight
// bytes, dword o * 4 + g = W[o][4g .. 4g+3] (rows o >= out are zero); [32..63] the high bytes; [64..71] bias = 128 * sum + half;
// [72..79] the weight sums; [80] 1 if a constant-255 alpha convolves to 255 at every output; [81] the precision
constexpr uint32_t kMf16Dwords = 84;

// Layout of the handle's worklist buffer (dwords): [0], [1] the two worklist counters (list B: tiles for the
// generic kernel) used alternately, [2 + 64*s, 2 + 64*s + 64) the tile-ticket counters of shrink64_kernel for
// counter set s, [kWorkA + s] the counters of list A, then list B and list A (n_tiles entries each).
constexpr uint32_t kTicketCounters = 64;
constexpr uint32_t kWorkA = 2 + 2 * kTicketCounters;  // two counters of list A (transparent tiles for shrink32a_kernel)
constexpr uint32_t kWorkList = kWorkA + 2;             // list B starts here (n_tiles entries), list A follows it

// q = n / d as (t + ((n - t) >> sh1)) >> sh2 with t = mulhi(n, mul)  (Granlund-Montgomery)
struct FastDiv {
	uint32_t mul, sh1, sh2;
};

struct ShrinkArgs {
	const uint8_t *src;      // frames, pitch-linear
	uint64_t frame_stride;   // bytes
	uint32_t pitch;          // bytes
	uint32_t width, height;
	uint32_t bw, bh;         // nominal tile size
	uint32_t cols, rows;
	uint32_t tiles_per_frame;
	uint32_t n_tiles;        // n_frames * tiles_per_frame
	FastDiv div_tpf, div_cols;
	uint32_t edge_w, edge_h; // size of the last column / row of tiles
	uint32_t mode, filter;
	float factor;
	// outputs (device); out_px may be null (no resample), out_w/out_h may be null
	uint32_t oklab_given;    // 1: full 32x32 RGBA tiles already carry their Oklab value in sums[] (oklab32_kernel)
	float scale2;            // Oklab mode: value = mean deviation * factor * scale2 (10 = BASE_FACTOR of shrink_by,
	                         //   pixlzr.rs:15,162; 1 with factor 1 = the identity closure of process(), process/mod.rs:107-121)
	FastDiv div_gpf, div_gcols;  // shrink16_kernel: divisors for its 2x2 tile groups (groups per frame, group columns)
	uint32_t n_frames_x_groups;  //   and the number of groups in the batch
	uint32_t ok_bands;       // Oklab detector with run-time geometry: bands (256 pixels) per tile, ceil(w * h / 256)
	uint32_t ok_region;      //   which tiles that launch takes: 0 the full ones, 1 the right column (edge_w x bh), 2 the bottom
	                         //   row (bw x edge_h), 3 the corner tile (edge_w x edge_h)
	uint32_t ok_count;       //   and how many items it enumerates (region 0: n_tiles)
	uint32_t ok_edges;       // consumers: edge regions whose values are in sums[] already (bit 0 right, 1 bottom, 2 corner)
	uint32_t clone_ahead;    // shrink_by, square RGBA tiles (round 4): oklab2_kernel copies every tile it converts into its slot as if it
	                         //   were stored at full size; the fast kernels behind it do not read such tiles again (PXZ_NO_CLONE_AHEAD=1: 0)
	uint32_t *clone_list;    //   64x64: room for the list of the tiles that are NOT stored at full size (8 + n_tiles dwords; clone_split64_kernel)
	uint32_t *ahead_spare;   //   2 KB nobody reads: where that kernel's copy of a band goes when there is no tile behind it
	float *ok_scratch;       // Oklab detector on 64x64 tiles: 16 floats per pixel quad between its passes (HBM)
	const uint32_t *mf64;    // 64x64 fast path: matrix-core operand tables (global memory), see Fast64Args
	uint32_t ok_rows;        // tile rows the block-cooperative Oklab detector takes: full_rows, plus the ragged last row
	                         //   when its height is a whole number of that detector's bands
	uint32_t full_cols, full_rows;  // 32x32 fast path: tile (tx, ty) is eligible iff tx < full_cols && ty < full_rows
	                                //   (full size, 16-byte aligned rows; 0/0 when the batch is not aligned)
	uint32_t alpha_kernel;   // frames with transparency announced (pxz_params.reserved bit 0) or seen by the last launch
	uint32_t alpha_first;    // most tiles of the last launch had transparency: the four-plane kernel takes every tile
	uint32_t finish_scan;    // worklist kernel: 1 = finish every tile the fast kernel completed (scan of all sums); 0 = the fast
	                         //   kernel did that itself, only the tiles of list A are left (when shrink32a_kernel took them)
	uint32_t list_a_too;     // worklist kernel: list A (full tiles with transparency) was not taken by shrink32a_kernel
	void *mid_event;         // host side only: hipEvent_t to record behind the first kernel of the step, or null
	uint32_t *stats;         // pinned host dwords (device address) <- [0] list-A tiles, [1] all listed tiles of this launch; may be null
	uint32_t expect_listed;  // what [1] said after the last finished launch (0xffffffff: unknown): sizes the worklist kernel's grid, nothing else
	uint32_t stats_sig;      // signature of this launch's configuration, written to stats[2] beside the counts: the host only trusts
	                         //   counts whose signature is its next launch's (round 4: a handle that went from 32x32 tiles, nothing
	                         //   listed, to 64x64 frames with a ragged bottom row ran its first launches with an 8-block worklist grid)
	uint32_t *work;          // worklist: [work_slot] = count, [2..] = tile ids (null: all tiles).  The two
	uint32_t work_slot;      //   counters alternate between launches; a launch zeroes the other one
	float *value;            // worklist mode only: the kernel finishes its tiles itself (finish_tile) and,
	float *lod0;             //   after the worklist, the tiles shrink32_kernel completed; each may be null
	float *lod1;
	uint32_t *sums;          // 2 per tile: gradient sums (directional) | f32 value bits (Oklab); -> finish_kernel
	                         //   With clone_ahead, sums[2 t + 1] is oklab2_kernel<AHEAD>'s "tile t was copied into its slot" flag (1).
	                         //   Every other path leaves gradient sums or value bits in that dword (a directional tile whose
	                         //   sum_vr is 1 leaves a 1), and a tile skipped as copied keeps its (value, 1) for the next
	                         //   launch on the handle.  Invariant: a consumer reads the flag only when clone_ahead is set in THIS
	                         //   launch, and only for tiles that oklab2_kernel<AHEAD> took in this launch (tx < full_cols,
	                         //   ty < full_rows <= ok_rows), which writes the flag of every tile it takes.  A tile read as copied
	                         //   without having been copied keeps stale slot bytes and faults nothing (tests/test_gpu_handle_reuse.py).
	uint32_t *out_w;
	uint32_t *out_h;
	uint8_t *out_px;
	uint32_t slot_bytes;     // bw*bh*channels
	// tables (device)
	AxisTab tabs[4 * kMaxLevel];  // [axis 0=x,1=y][cls 0=full,1=edge][kMaxLevel], in the kernarg segment:
	                              // scalar loads, never behind the vector-memory counter
	const uint16_t *bounds;
	const uint32_t *coeffs;
	const int32_t *ksums;
	const uint32_t *trows;   // unified table rows, padded by 32 dwords
	uint32_t tab_dw;         // dwords of trows to keep in LDS (multiple of 4), 0 = too large / unused
	// Level decision: m = #{j < kMaxLevel : key < breaks[cls][j]} (or key >= ... when breaks_asc[cls]),
	// cls = ycls*2 + xcls.  directional: key = integer gradient sum; Oklab: key = bits of the parsed value.
	uint32_t breaks[4][kMaxLevel];
	uint32_t breaks_asc[4];
	// LDS carve-up (dwords per tile): 4 planes of u16 pairs [y][x], 4 transposed planes [ox][y], Oklab scratch
	uint32_t rs;             // plane row stride: round_up(ceil(bw/2), 2), +2 of bank skew when a multiple of 16
	uint32_t plane_dw;       // rs * bh
	uint32_t hps;            // transposed row stride: round_up(ceil(bh/2), 2), +2 of bank skew likewise
	uint32_t tmp_dw;         // ceil(bw/2) * hps   (0 when no convolution)
	uint32_t lab_dw;         // Oklab mode: 3*bw*bh floats (aliases the transposed planes), else 0
	uint32_t tile_dw;        // total dwords per tile incl. over-read slack
	uint32_t *big_scratch;   // tiles whose image exceeds LDS (round 4): big_blocks images of tile_dw dwords in HBM, one per block
	uint32_t big_blocks;     //   of the generic kernel (0: the image is in LDS)
};

// Factor ladder (pxz_shrink_ladder_frames_device, shrink_by): ladder_kernel turns the raw detector value x of every tile into
// the K rungs' values, sizes and slots, staging each tile once and resampling it once per distinct level.  x comes from an
// identity launch of the ordinary flow (factor 1, scale 1, no pixels).  What that launch leaves in the handle is what a
// pxz_lod_frames_device launch leaves: sums[] holds that launch's detector keys (sums[2t] = bits of x; clone_ahead is off
// without pixels, so no "copied" flag of THIS launch is in sums[2t+1], and the next launch rewrites every flag it reads),
// and the worklist counters are zeroed and switched over as after every fast-path launch.  It writes no kernel-selection
// statistics (stats = null): the next single-factor launch sees the counts of the launch before the ladder.  ladder_kernel
// itself touches neither sums[] nor the worklist.  Per-rung data (the factors) are in handle scratch, not in here.
struct LadderArgs {
	const uint8_t *src;      // frames, pitch-linear, as the caller passed them (any alignment, 3 or 4 channels)
	uint64_t frame_stride;
	uint32_t pitch;
	uint32_t bw, bh, cols, rows, tiles_per_frame, n_tiles;
	FastDiv div_tpf, div_cols;
	uint32_t edge_w, edge_h, filter;
	uint32_t n_rungs;        // K, 1 .. 16 (one lane per rung decides it)
	const float *x;          // n_tiles raw detector values: x = sum of deviations / count (the identity closure)
	const float *factors;    // n_rungs factors (device)
	float *value;            // rung-major outputs: index (r * n_tiles + tile), 64-bit
	uint32_t *out_w, *out_h;
	uint8_t *out_px;         //   slots of slot_bytes; null: values and sizes only
	uint32_t slot_bytes;
	uint32_t rs, plane_dw, hps, tmp_dw, tile_dw;  // LDS image of a tile, as ShrinkArgs (no detector planes)
	AxisTab tabs[4 * kMaxLevel];
	const uint16_t *bounds;
	const uint32_t *coeffs;
	const int32_t *ksums;
	uint32_t breaks[4][kMaxLevel];  // shrink_by's level decision (the thresholds' bit patterns, ShrinkArgs::breaks)
	uint32_t breaks_asc[4];
};

// shrink32_kernel and shrink32a_kernel address a lane's share of a tile as (wave-uniform 64-bit pointer) + (32-bit lane
// offset): lane/8 rows (at most 7) + the lane's pixel quad (at most 7 * 16 bytes).  A pitch beyond this (613 MB per row) is
// the host's to catch: such a batch gets no fast path at all (full_cols = full_rows = 0, the generic kernel takes every tile).
constexpr uint32_t kFast32LaneRows = 7, kFast32LaneBytes = 7 * 16;
constexpr bool fast32_lane_offset_fits(uint32_t pitch)
{
	return (uint64_t)kFast32LaneRows * pitch + kFast32LaneBytes <= 0xffffffffull;
}

// Arguments of shrink32_kernel (full 32x32 RGBA tiles only): the subset of ShrinkArgs it needs
struct Fast32Args {
	const uint8_t *src;
	uint64_t frame_stride;
	uint32_t pitch, cols, rows, tiles_per_frame, n_tiles;
	FastDiv div_tpf, div_cols;
	uint32_t n_groups;       // shrink16_kernel: 2x2 groups of tiles, ceil(cols/2) * ceil(rows/2) per frame
	FastDiv div_gpf, div_gcols;
	uint32_t full_cols, full_rows, ok_rows, ok_edges;  // as in ShrinkArgs
	uint32_t filter;
	uint32_t *sums;
	uint32_t *out_w;
	uint32_t *out_h;
	uint8_t *out_px;
	uint32_t *work;
	uint32_t work_slot;
	uint32_t alpha_list;     // 1: full tiles with transparency go to list A (shrink32a_kernel), else to list B (generic kernel)
	const uint32_t *trows;
	uint32_t tab_dw, tile_dw;
	uint32_t chunk_lg;       // tickets deal runs of 2^chunk_lg adjacent tiles
	uint32_t finish_here;    // shrink32_kernel: every block finishes the tiles it completed (value / lod outputs) at its end
	uint32_t all_tiles;      // shrink32a_kernel: every tile of the batch (not list A): the launch that skips shrink32_kernel
	uint32_t narrow;         // shrink32_kernel: 4/2/1-px-wide outputs take resample_mfma32_narrow (0: PXZ_NO_NARROW=1, the round-1 forms)
	uint32_t group16;        // shrink16_kernel: the two-pass tiles of a group go through resample_group16_mfma (0: PXZ_NO_GROUP16=1)
	uint32_t clone_ahead;    // MODE 0: tiles stored at full size are in their slots already (ShrinkArgs::clone_ahead)
	float factor;            //   with these, as the worklist kernel's scan over all tiles would
	float *value, *lod0, *lod1;
	uint32_t breaks[kMaxLevel];
	uint32_t breaks_asc;
	AxisTab tabs[kMaxLevel];
};

// shrink64_kernel: full, aligned, opaque 64x64 RGBA tiles (the reference CLI's default block size), one
// tile per block of four waves.  Matrix-core operand tables live in global memory (mf64):
//   per level with out = 32|16|8|4|2|1:  nblk = max(1, out/16) output blocks, each
//     [lo: 64 lanes x 16 B][hi: 64 lanes x 16 B]   lane (o = l & 15, g = l >> 4): K[16*blk + o][16g .. 16g+15]
//   then bias[32], ksum[32], flag (as in kMfDwords)
struct Fast64Args {
	const uint8_t *src;
	uint64_t frame_stride;
	uint32_t pitch, cols, rows, tiles_per_frame, n_tiles;
	FastDiv div_tpf, div_cols;
	uint32_t full_cols, full_rows, ok_rows, ok_edges;
	uint32_t filter;
	uint32_t *sums;
	uint32_t *out_w;
	uint32_t *out_h;
	uint8_t *out_px;
	uint32_t *work;
	uint32_t work_slot;
	uint32_t clone_ahead;    // MODE 0: tiles stored at full size are in their slots already (ShrinkArgs::clone_ahead)
	uint32_t *clone_list;    //   and, when not null, finished: [0] = how many tiles are left, [8 ..] = which (clone_split64_kernel)
	uint32_t all_tiles;      // ALPHA instance: every tile of the batch (not list A): the launch that skips the opaque instance
	const uint32_t *mf64;
	uint32_t mf_off[kMaxLevel];      // dword offset of the level's table in mf64 (0: none; the blob starts with a pad)
	uint32_t precision[kMaxLevel];
	uint32_t breaks[kMaxLevel];
	uint32_t breaks_asc;
	uint32_t finish_here;    // every block finishes the tiles it completed (value / lod outputs) at its end, as shrink32_kernel does
	float factor;
	float *value, *lod0, *lod1;
};

// Diagnostic switches (PXZ_* environment variables), read ONCE per process -- never on the call path.  Every one of
// them only picks between kernels that produce the same bytes (the tests run both sides); none is part of the ABI.
struct Knobs {
	bool no_alpha_kernel;   // PXZ_NO_ALPHA_KERNEL: tiles with transparency stay on the generic kernel
	bool no_oklab_general;  // PXZ_NO_OKLAB_GENERAL: no run-time-geometry Oklab detector
	bool no_oklab32;        // PXZ_NO_OKLAB32: no block-cooperative Oklab detector at all
	bool no_oklab_edges;    // PXZ_NO_OKLAB_EDGES: ragged edge tiles keep their four-lane chains
	bool no_repitch;        // PXZ_NO_REPITCH: unaligned device batches are staged pixel by pixel
	bool no_widen;          // PXZ_NO_WIDEN: RGB batches never ride the RGBA kernels
	bool no_native_rgb;     // PXZ_NO_NATIVE_RGB: RGB batches are widened to RGBA even where a kernel reads RGB itself
	bool no_alpha_first;    // PXZ_NO_ALPHA_FIRST: transparent batches keep the two-kernel flow (shrink32_kernel lists, shrink32a_kernel takes the list)
	bool no_narrow;         // PXZ_NO_NARROW: 4/2/1-px-wide outputs of 32x32 tiles keep the round-1 resample forms
	bool no_big_tiles;      // PXZ_NO_BIG_TILES: tiles whose image exceeds LDS are refused (PXZ_ERR_UNSUPPORTED), as before round 4
	bool no_group16;        // PXZ_NO_GROUP16: the two-pass tiles of a 16x16 group keep their own dot2 resamples (no block-diagonal matrix-core products)
	bool no_clone_ahead;    // PXZ_NO_CLONE_AHEAD: shrink_by's detector does not copy tiles into their slots ahead of the value (round-3 flow: the shrink kernel reads every tile again)
	bool oklab_v1;          // PXZ_OKLAB_V1: round-1 detector (one chain wave, two barriers per band; 64-px tiles parked in HBM)
	bool no_expand_fast32;    // PXZ_NO_EXPAND_FAST32: expand_kernel keeps its general forms for 32x32 RGBA tiles (no matrix-core convolutions, no shift-indexed Nearest)
	bool tree_rects;        // PXZ_TREE_RECTS: tree::process always goes over rectangle lists (pxz_tree.hip), also where the per-level grids apply
	int wpb;                // PXZ_WPB: waves per block of the persistent kernels (0: default)
	int chunk_lg;           // PXZ_CHUNK_LG: log2 of the ticket run length of shrink32_kernel (-1: default)
	int cus;                // PXZ_CUS: every grid is sized as for a chip of at most this many CUs (0: the device's count); never raises it
};
const Knobs &knobs();

struct LaunchGeom {
	uint32_t blocks, threads, lds_bytes;
};

struct FinishArgs {
	const uint32_t *sums;
	float *value;            // may be null
	float *lod0;             // may be null
	float *lod1;             // may be null
	uint32_t n_tiles, tiles_per_frame, cols, rows, bw, bh, edge_w, edge_h, mode;
	float factor;
};

struct PackArgs {
	const uint32_t *w, *h;        // per tile
	const uint32_t *sizes;        // optional: explicit byte sizes per tile (else w*h*channels)
	const uint8_t *slots;
	unsigned long long *offsets;  // n_tiles + 1
	unsigned long long *chunk_totals;
	uint8_t *packed;
	unsigned long long capacity;
	uint32_t n_tiles, n_chunks, channels, slot_bytes;
};

struct QoiArgs {
	const uint8_t *slots;
	const uint32_t *w, *h;
	const float *value;
	uint32_t *perm;               // tiles ordered by pixel count (largest first)
	uint32_t *bins;               // 64: histogram + cursors
	uint8_t *scratch;             // the encoder's units (pxz_stream.hip: qoi_class_rows), classes in descending order
	uint32_t *rec_len;
	unsigned long long *offsets;  // n_tiles + 1
	unsigned long long *chunk_totals;
	uint8_t *out;
	unsigned long long *file_offsets;  // n_frames + 1
	unsigned long long capacity;
	uint32_t n_tiles, n_chunks, tiles_per_frame, cols, rows;
	uint32_t channels, slot_bytes, hdr_bytes;
	uint32_t width, height, bw, bh, filter_byte;
	uint32_t splice_unit_blocks;  // (set by launch_qoi) the blocks of qoi_splice_kernel below this one take units, the others headers
};

// Decode side (expand_kernel): one table per (axis, size class, source size) of an up-scale to the full
// tile size.  starts/sizes hold one entry per output sample, coeffs out_size * window i16 weights.
struct ExpandTab {
	uint32_t start_off;      // into starts[] / sizes[] (nearest: starts[] is the source index)
	uint32_t coeff_off;      // into coeffs[]
	uint16_t window;
	uint16_t precision;
};

// expand_kernel's matrix-core tables (32x32 tiles, the convolutions): one block of kXmfDw dwords per stored size 2^li,
// li = 0 .. kXmfLevels-1 (1, 2, 4, 8, 16 px -> 32 px; one table serves both axes).  Operand of v_mfma_i32_32x32x16_i8
// for output sample o = lane & 31 and k group kg = lane >> 5: k slot j stands for source sample xmf_src(kg, j).
//   [0, 128)    low bytes of the weights, lane l at dwords 2l, 2l+1      [128, 256)  high bytes (weight = 256 hi + lo, lo signed)
//   [256, 288)  bias per output sample (128 * weight sum + half)           [288, 320)  the same in accumulator order [g][reg]
//   [320]       precision        [321]  1: a one-sample source is copied (every window is the weight 2^precision alone)
constexpr uint32_t kXmfLevels = 5, kXmfDw = 324;
constexpr uint32_t xmf_src(uint32_t kg, uint32_t j) { return j < 4u ? 4u * kg + j : 8u + 4u * kg + (j - 4u); }
constexpr uint32_t xmf_row(uint32_t g, uint32_t reg) { return (reg & 3u) + 8u * (reg >> 2) + 4u * g; }  // accumulator reg -> row

// expand16_kernel's matrix-core tables (16x16 tiles in 2x2 groups, the convolutions): one block of kXmf16Dw dwords per stored size
// 2^li, li = 0 .. kXmf16Levels-1 (1, 2, 4, 8 px -> 16 px; one table serves both axes):
//   [0, 32)   low bytes of the weights: dword o * 2 + kg = K[o][4 kg .. 4 kg + 3] for output sample o < 16 (source samples >= the
//             stored size carry zero)                       [32, 64)  high bytes
//   [64, 80)  bias per output sample (128 * weight sum + half)
//   [80, 96)  the same in accumulator order: [g][r], r < 8, for output sample (r & 3) + 8 (r >> 2) + 4 g
//   [96]      precision
constexpr uint32_t kXmf16Levels = 4, kXmf16Dw = 100;

// expand64_kernel's matrix-core tables (64x64 tiles, the convolutions): one block of kXmf64Dw dwords per stored size 2^li,
// li = 0 .. kXmf64Levels-1 (1 .. 32 px -> 64 px; one table serves both axes).  The 64 outputs are two halves q of 32, the source
// samples steps s of 16 (one step up to 16 px, two at 32):
//   [((q * 2 + s) * 2 + piece) * 128 + 2 l, + 1]   lane l = kg * 32 + o: weight bytes (piece 0 low, 1 high) of output 32 q + o for
//                                                  the source samples 16 s + xmf_src(kg, j), j = 0 .. 7
//   [1024, 1088)  bias per output sample (128 * weight sum + half)
//   [1088, 1152)  the same in accumulator order: [q][g][reg] for output 32 q + xmf_row(g, reg)
//   [1152]        precision
constexpr uint32_t kXmf64Levels = 6, kXmf64Dw = 1156;

struct ExpandArgs {
	const uint32_t *tile_w, *tile_h;  // per tile: stored size
	const uint8_t *slots;             // per tile slot_bytes, tile_w*tile_h*channels valid, tightly packed
	uint8_t *dst;                     // frames, pitch-linear
	uint64_t frame_stride;
	uint32_t pitch, width, height, channels;
	uint32_t bw, bh, cols, rows, tiles_per_frame, n_tiles, edge_w, edge_h;
	uint32_t slot_bytes, filter;
	uint32_t out_channels;            // bytes per pixel in dst (4 with channels == 3: alpha 255 is added, process())
	// tabs[(axis*2 + cls) * dir_stride + in_size], in_size in [1, full]; dir_stride = max(bw, bh) + 1
	const ExpandTab *tabs;
	uint32_t dir_stride;
	const uint16_t *starts, *sizes;
	const int16_t *coeffs;
	uint32_t tile_dw;                 // LDS dwords per wave: source pixels + horizontal-pass result
	const uint32_t *xmf;              // kXmfLevels * kXmfDw dwords, or null (other tile sizes, Nearest, weights beyond 16 bits)
	uint32_t fast32;                  // 0: the general forms only (PXZ_NO_EXPAND_FAST32)
	uint32_t *status;                 // set to 1 when a tile's stored size is 0 or exceeds its full size
	uint32_t quiet_empty;             // 1: tiles of stored size 0 x 0 are simply not written (tree::process: not this level's)
	const uint32_t *xmf16;            // kXmf16Levels * kXmf16Dw dwords (16x16 tiles, a convolution filter), or null
	const uint32_t *xmf64;            // kXmf64Levels * kXmf64Dw dwords (64x64 tiles, a convolution filter), or null
	uint32_t *list;                   // 16x16 flow: tiles expand16_kernel left to expand_kernel (status[1] counts them), or null
	uint32_t list_mode;               // expand_kernel: 1 = take the tiles of `list` (status[1] of them) instead of every tile
	FastDiv div_gpf, div_gcols;       // expand16_kernel: divisors for its 2x2 tile groups (groups per frame, group columns)
	uint32_t *big_scratch;            // tiles whose image exceeds LDS (round 4): one image of tile_dw dwords per wave of the grid in HBM
	uint32_t big_waves;               //   (0: the images are in LDS)
};

// Decode side: .pixlzr files -> tile values, sizes and pixel slots (pixlzr_index_kernel, qoi_decode_kernel)
struct DecodeArgs {
	const uint8_t *files;                   // the files back to back
	const unsigned long long *file_offsets; // n_frames + 1 byte offsets
	float *value;
	uint32_t *tile_w, *tile_h;
	uint8_t *slots;
	unsigned long long *rec_off;            // scratch, per tile: offset of the record's QOI body in files[]
	uint32_t *rec_len;                      // scratch, per tile: length of that body (0: unusable)
	uint32_t *perm, *bins;                  // scratch: tiles ordered by pixel count (as in the encoder), 64 counters
	uint32_t *status;                       // bit 1: malformed file / record
	uint32_t width, height, bw, bh, cols, rows, tiles_per_frame, n_tiles, n_frames, channels, slot_bytes;
	uint32_t edge_w, edge_h;
};

// RGB frames ride the RGBA fast paths: widen to RGBA (alpha 255) on the way in, narrow the tile slots on the way out
struct WidenArgs {
	const uint8_t *src;
	uint8_t *dst;
	uint64_t src_frame_stride, dst_frame_stride;
	uint32_t src_pitch, dst_pitch, width, height, n_frames;
};
struct NarrowArgs {
	const uint8_t *slots4;
	uint8_t *slots3;
	const uint32_t *w, *h;
	uint32_t n_tiles, slot4_bytes, slot3_bytes;
};

// tree::process (src/process/tree.rs:23-83), one level of the quad tree = the regular grid of that level's block size
struct TreeArgs {
	const uint8_t *src;           // the source frames (for the tiles that are handed back unchanged)
	uint8_t *dst;                 // RGBA output frames
	uint64_t src_frame_stride, dst_frame_stride;
	uint32_t src_pitch, dst_pitch, channels;
	const float *value;           // this level's grid: get_block_variance of every tile
	uint32_t *tile_w, *tile_h;    //   reduced sizes; set to 0 for tiles that are not pixelised at this level
	const uint8_t *parent_open;   // previous level's grid: 1 = the tile went on to this level (null at level 0: all tiles)
	uint8_t *open;                // this level's grid: 1 = the tile goes on to the next level
	uint32_t bw, bh, cols, rows, tiles_per_frame, n_tiles, edge_w, edge_h;
	uint32_t parent_cols, parent_tiles_per_frame;
	float threshold;              // |threshold|
	uint32_t positive;            // tree.rs:37: threshold >= 0 (deeper levels: always)
	uint32_t last;                // no further level: a tile that fails the test keeps its pixels (tree.rs:34-36)
};

// tree::process on rectangle lists (pxz_tree.hip): the tiles of one level of the recursion, wherever they lie
struct TreeRect {
	uint32_t x, y;      // origin in the frame
	uint16_t w, h;
	uint32_t frame;
};
// one axis table of the rectangle kernel: windows of `out` samples over `in` samples; up = 1: the table of the way back
// (PixlzrBlock::resize with the upscale flag set, block.rs:301-306)
struct TreeAxisEntry {
	uint16_t in, out;
	uint16_t up, window;
	uint32_t precision;
	uint32_t starts_off;   // into starts[] / sizes[] (Nearest: starts[] is the source index, no sizes / coefficients)
	uint32_t coeff_off;    // into coeffs[]: out * window weights
};
struct TreeRectArgs {
	const uint8_t *src;
	uint8_t *dst;                  // RGBA frames
	uint64_t src_frame_stride, dst_frame_stride;
	uint32_t src_pitch, dst_pitch, channels;
	const TreeRect *rects;
	uint32_t n_rects;
	float threshold;               // |threshold|
	uint32_t positive;             // tree.rs:37 (deeper levels: always)
	uint32_t next_bw, next_bh;     // block of the next level (tree.rs:73)
	uint32_t next_is_leaf;         // ... which is not above the minimum: a tile that goes on keeps its pixels (tree.rs:34-36)
	TreeRect *next_rects;
	uint32_t *next_count;
	uint32_t next_capacity;
	uint32_t filter_down, filter_up;
	const TreeAxisEntry *dir;
	uint32_t n_dir;
	const int32_t *starts;
	const int32_t *sizes;
	const int16_t *coeffs;
	float thresholds[kNumThresholds];
};

// Batches of differently sized images (pxz_shrink_varied_frames_device, pxz_varied.hip): one flat tile space over the
// batch.  Image i owns tiles [tile0, tile0 + cols * rows) and tile rows [row0, row0 + rows) of it.
struct VariedImage {
	uint64_t offset;         // bytes from the batch's base pointer to the image's first pixel
	uint32_t tile0, row0;    // first tile / first tile row of the image in the batch
	uint32_t width, height, pitch;
	uint32_t cols, rows, edge_w, edge_h;
	uint32_t hdr_bytes;      // writer: 26 + 4 * rows (mod.rs:47-48)
};

// One down-scaling table per (source size, level): dir[in * kMaxLevel + m] for every source size in of the batch's tiles
// (the full bw, bh and each distinct edge width and height) and m = 1 .. kMaxLevel - 1, in the TreeAxisEntry format (out is
// reduced_size(in, m); entries with out == in are never read).
struct VariedArgs {
	const uint8_t *base;
	const VariedImage *images;
	uint32_t n_images, n_tiles;
	uint32_t bw, bh, mode, filter;
	float factor;
	float *value;
	uint32_t *out_w, *out_h;
	uint8_t *out_px;         // null: values and sizes only
	uint32_t slot_bytes;
	uint32_t tile_bytes;     // LDS bytes of one tile image (bw * bh * channels, rounded up to 16)
	const TreeAxisEntry *dir;
	const int32_t *starts, *sizes;
	const int16_t *coeffs;
	float thresholds[kNumThresholds];
};

// Varied ladder (pxz_shrink_varied_ladder_frames_device, pxz_varied_ladder.hip): the varied call's arguments (v.factor is
// unused) and the rungs' factors.  Rung r of tile t writes value, sizes and slot r * v.n_tiles + t.
constexpr uint32_t kVariedLadderMaxRungs = 32;  // PXZ_VARIED_LADDER_MAX_RUNGS
struct VariedLadderArgs {
	VariedArgs v;
	uint32_t n_factors;
	float factors[kVariedLadderMaxRungs];
};

// Writer of a varied batch: what the per-image headers need beside QoiArgs (record lengths, their scan, the file offsets)
struct VariedWriterArgs {
	const VariedImage *images;
	uint32_t n_images, n_tiles, n_rows;  // n_rows: tile rows of the whole batch
	uint32_t bw, bh, filter_byte;
	uint32_t *rec_len;
	const unsigned long long *offsets, *chunk_totals;
	uint8_t *out;
	unsigned long long *file_offsets;
	unsigned long long capacity;
};

// What the wave-per-tile kernels of a flat tile space share (varied_expand_kernel, window_expand_kernel; distortion_kernel
// names the same fields in a struct of its own, see DistortionArgs):
// the stored tiles, the block, the up-scaling tables and the LDS image of one wave -- what varied_resize_tile and the tile
// loop read (pxz_device.h), filled by put_varied_expand_tables and the launch.  One table per (full size, stored size):
// dir[slot[full] * stride + stored] (pxz_tables.h: VariedExpandTableSet).
struct TileResizeArgs {
	uint32_t bw, bh, slot_bytes, filter;
	const uint32_t *slot;
	const ExpandTab *dir;
	uint32_t stride;
	const uint16_t *starts, *sizes;
	const int16_t *coeffs;
	uint32_t wdw;                     // dwords of one staged window: 1 + ceil(widest window / 2)
	uint32_t tile_dw;                 // dwords of one wave's image: two tile-sized planes + the windows of both axes
	uint32_t t0_dw;                   // (set by the launch) dwords of the owners' first tiles kept in LDS, 0: read from the table
	uint32_t *status;                 // bit 0: a tile's stored size is 0 or exceeds its full size
	uint32_t n_tiles;
	const uint32_t *tile_w, *tile_h;  // per tile (distortion: per set and tile): stored size
	const uint8_t *slots;             // per tile slot_bytes, tile_w * tile_h * channels valid, tightly packed
};

// Re-shrink of stored tiles (pxz_reshrink_varied_frames_device, pxz_reshrink.hip): the stored tiles of a flat tile space
// expanded to their full sizes in LDS and shrunk again, one tile per block.  v is the shrink side as varied_kernel takes it
// (v.base is unused, v.tile_bytes is one LDS plane of bw * bh dwords, rounded up to 16 bytes); x is the expand side: the tables
// of put_varied_expand_tables, the stored sizes and slots that are read, and the status word (x.tile_dw and x.t0_dw are
// unused: the block's LDS is reshrink_lds', pxz_varied_tile.h).  The outputs of v may be the inputs of x (pxz_reshrink.hip: in place).
struct ReshrinkArgs {
	VariedArgs v;
	TileResizeArgs x;
	uint32_t *image_flags;            // per image 1 for a tile whose stored size is invalid, or null
};

// Re-shrink ladder (pxz_reshrink_varied_ladder_frames_device, pxz_reshrink_ladder.hip): the re-shrink's arguments (r.v.factor
// and r.v.tile_bytes are unused) and the rungs' factors.  Rung q of tile t writes
// value, sizes and slot q * r.v.n_tiles + t; a flagged tile writes 0 x 0 and value bits 0 to every rung.
struct ReshrinkLadderArgs {
	ReshrinkArgs r;
	uint32_t n_factors;
	float factors[kVariedLadderMaxRungs];
};

// Re-tile of stored tiles (pxz_retile_varied_frames_device, pxz_retile.hip): the stored tiles of one layout of a batch brought to
// the tiles of another layout of the same images, one DESTINATION tile per block.  v is the shrink side as varied_kernel takes
// it, for the destination block (v.base is unused, v.tile_bytes is one LDS plane of v.bw * v.bh dwords, rounded up to 16 bytes;
// v.images is the destination layout's table); x is the expand side for the SOURCE block (x.bw, x.bh, x.slot_bytes; the tables of
// put_varied_expand_tables for the source geometry; the stored sizes and slots that are read; the status word; x.tile_dw and
// x.t0_dw are unused: the block's LDS is retile_lds', pxz_varied_tile.h).  Inputs and outputs never alias: the layouts differ.
struct RetileArgs {
	VariedArgs v;
	TileResizeArgs x;
	const VariedImage *src_images;    // the same images in the source layout (entry i: image i), of which tile0, cols, rows and edges are read
	uint32_t *image_flags;            // per image 1 for a source tile whose stored size is invalid, or null
};

// Re-tile ladder (pxz_retile_varied_ladder_frames_device, pxz_retile_ladder.hip): the re-tile's arguments (r.v.factor is not
// read; r.v.value, out_w, out_h, out_px hold n_factors rungs of r.v.n_tiles entries each, rung-major in the destination layout)
// and the rungs' factors, by value.  The block's LDS is retile_ladder_lds' (pxz_varied_tile.h).
struct RetileLadderArgs {
	RetileArgs r;
	uint32_t n_factors;
	float factors[kVariedLadderMaxRungs];
};

// Expand of a varied batch (pxz_expand_varied_frames_device, pxz_varied_expand.hip): the stored tiles of the flat tile space
// back to their places in the images.
struct VariedExpandArgs : TileResizeArgs {
	const VariedImage *images;
	uint32_t n_images;
	uint8_t *base;                    // image i at base + images[i].offset, images[i].pitch between rows
	uint32_t *image_flags;            // per image 1 for a tile whose stored size is invalid, or null
	uint32_t *big_scratch;            // tile images beyond LDS: one of tile_dw dwords per wave of the grid in HBM
	uint32_t big_waves;               //   (0: the images are in LDS)
};

// Squared error of stored tiles against their source (pxz_distortion_frames_device, pxz_distortion_varied_frames_device;
// pxz_distortion.hip): n_sets stored versions of every tile, set-major: set s of tile t is at index s * n_tiles + t of
// tile_w, tile_h and slots.  The wave's image is always in LDS (no HBM form).  NOT derived from TileResizeArgs: it names the
// same fields in the order this kernel was tuned with -- derived, distortion_kernel<4> measured 1.0-1.5 % slower on 64x64 tiles
//  -- and varied_resize_tile and put_varied_expand_tables take either struct.
struct DistortionArgs {
	const VariedImage *images;
	uint32_t n_images, n_tiles, n_sets;
	const uint32_t *tile_w, *tile_h;  // per set and tile: stored size
	const uint8_t *slots;             // per set and tile slot_bytes, tile_w * tile_h * channels valid, tightly packed
	const uint8_t *base;              // the source: image i at base + images[i].offset, images[i].pitch between rows
	uint32_t bw, bh, slot_bytes, filter;
	const uint32_t *slot;
	const ExpandTab *dir;
	uint32_t stride;
	const uint16_t *starts, *sizes;
	const int16_t *coeffs;
	uint32_t wdw, tile_dw;            // as VariedExpandArgs
	uint32_t t0_dw;                   // (set by the launch) dwords of the images' first tiles kept in LDS, 0: read from `images`
	uint32_t *status;                 // bit 0: a tile's stored size is 0 or exceeds its full size
	uint32_t *image_flags;            // per image 1 for the same, or null
	unsigned long long *tile_sse;     // per set, tile and channel (index (s * n_tiles + t) * channels + c), or null; all-ones for a
	                                  //   tile whose stored size is invalid
	unsigned long long *image_sse;    // per set, image and channel (index (s * n_images + i) * channels + c): the sums over the
	                                  //   image's valid tiles, added with atomics (zeroed before the launch)
};

// Squared error of re-shrunk tiles against the archive's own (pxz_reshrink_distortion_varied_device,
// pxz_reshrink_distortion.hip): the flat tile space of `images`, one reference stored tile per tile (r: the archive, expanded
// with expand_filter's tables; r.tile_w / r.tile_h / r.slots hold n_tiles entries) and n_sets stored versions of it, set-major (u:
// the sets, expanded with filter_up's tables; u.tile_w / u.tile_h / u.slots hold n_sets * n_tiles entries).  r and u are what
// put_varied_expand_tables fills; of their launch fields only r.status is read (u.status, both n_tiles, tile_dw and t0_dw are
// unused: this struct's own count).  Outputs as DistortionArgs'.
struct ReshrinkDistortionArgs {
	const VariedImage *images;
	uint32_t n_images, n_tiles, n_sets;
	TileResizeArgs r, u;
	uint32_t wdw;                     // dwords between the staged windows of the wave's region: the wider of r.wdw and u.wdw
	uint32_t tile_dw;                 // dwords of one wave's image (reshrink_distortion_tile_dw, pxz_launch.h)
	uint32_t t0_dw;                   // (set by the launch) dwords of the images' first tiles kept in LDS, 0: read from `images`
	uint32_t *image_flags;            // per image 1 for a reference or set tile whose stored size is invalid, or null
	unsigned long long *tile_sse;     // index (s * n_tiles + t) * channels + c, or null; all-ones for an invalid entry
	unsigned long long *image_sse;    // index (s * n_images + i) * channels + c, added with atomics (zeroed before the launch)
};

// Squared error of re-tiled tiles against the archive they came from (pxz_retile_distortion_varied_device,
// pxz_retile_distortion.hip): the flat tile space of `images`, the DESTINATION layout, one destination tile per block.  r is the
// archive: the SOURCE block (r.bw, r.bh, r.slot_bytes), expand_filter's tables for the source geometry, and the stored sizes and
// slots of the source layout `src_images` (entry i: image i).  u are the n_sets stored versions of every destination tile,
// set-major: the destination block, filter_up's tables, n_sets * n_tiles entries.  r and u are what put_varied_expand_tables
// fills; of their launch fields only r.status is read (the block's LDS is retile_distortion_lds', pxz_varied_tile.h).
// Outputs as DistortionArgs'.
struct RetileDistortionArgs {
	const VariedImage *images, *src_images;
	uint32_t n_images, n_tiles, n_sets;
	TileResizeArgs r, u;
	uint32_t *image_flags;            // per image 1 for a source or set tile whose stored size is invalid, or null
	unsigned long long *tile_sse;     // index (s * n_tiles + t) * channels + c, or null; all-ones for an invalid entry
	unsigned long long *image_sse;    // index (s * n_images + i) * channels + c, added with atomics (zeroed before the launch)
};

// Fit to a budget (pxz_fit_varied_ladder_device, pxz_fit.hip): one rung per image out of what the writer and the distortion
// call left for the descriptors repeated n_factors times.  The rule is fit_pick's (pxz_fit.h).
struct FitArgs {
	uint32_t n_images, n_factors, channels, criterion;
	const unsigned long long *targets;       // per image (handle scratch)
	const unsigned long long *file_offsets;  // n_factors * n_images + 1: file r * n_images + i is [k], [k + 1])
	const unsigned long long *image_sse;     // index (r * n_images + i) * channels + c
	uint32_t *choice, *flags;                // per image: the rung, and bit 0 when no rung met the target
};

// The chosen rungs' tiles as an ordinary varied batch (pxz_gather_varied_rungs_device, pxz_fit.hip): output tile t of image i
// is input tile choice[i] * n_tiles + t (a choice of n_factors or more: the last rung, and bit 1 of the image's flag).
struct GatherArgs {
	const VariedImage *images;
	uint32_t n_images, n_tiles, n_factors;
	uint32_t slot_bytes;
	const uint32_t *choice;
	const uint32_t *value;                   // rung-major inputs (the values as their bits)
	const uint32_t *w, *h;
	const uint8_t *slots;
	uint32_t *out_value, *out_w, *out_h;     // the varied layout of the n_images images
	uint8_t *out_slots;                      // null: values and sizes only
	uint32_t *image_flags;                   // per image 0 or 2, or null
};
// (pxz_gather_varied_tile_rungs_device, pxz_tilefit.hip, fills the same struct: choice then has an entry per output tile, and
// image_flags is zeroed before the launch -- the kernel only sets bit 1)

// The writer's record lengths out of its scratch (pxz_record_bytes_varied_device, pxz_tilefit.hip): rec_len as
// launch_qoi_varied leaves it, the next image's header on every image's last record but the last's.
struct RecordBytesArgs {
	const VariedImage *images;
	uint32_t n_images, n_tiles;
	const uint32_t *rec_len;
	uint32_t *record_bytes;                  // per tile: 13 + the record's length field
};

// Fit to a budget per tile (pxz_fit_varied_tiles_device, pxz_tilefit.hip): one rung per tile under one target per group of
// images.  The rule is pxz_tilefit.h's; everything but the inputs and the outputs is handle scratch.
struct TileFitArgs {
	uint32_t n_tiles, n_groups, n_factors, channels, criterion;
	uint32_t step;                           // (set by the launch) the halving a tilefit_step_kernel runs
	const uint32_t *group_tile0;             // n_groups + 1: group g owns the flat tiles [g], [g + 1])
	const unsigned long long *fixed;         // per group: the headers and line tables of its files
	const unsigned long long *targets;       // per group
	const uint32_t *record_bytes;            // index r * n_tiles + t
	const unsigned long long *tile_sse;      // index (r * n_tiles + t) * channels + c
	unsigned long long *cand;                // index r * n_tiles + t: tilefit_pack of the candidate
	uint32_t *tile_group;                    // per tile
	unsigned long long *interval;            // [2][n_groups][2]: lo, hi; step k reads buffer (k + 1) & 1 and writes k & 1
	unsigned long long *acc;                 // [kTileFitSteps][n_groups]: the group's total at step k's lambda (zeroed)
	unsigned long long *tot;                 // [n_groups][2]: bytes and error at lambda* (zeroed)
	unsigned long long *uni;                 // [n_groups][n_factors][3]: a rung's bytes, error, tiles without it (zeroed)
	uint32_t *group_bits;                    // per group: kTileFitNoCandidate (zeroed)
	uint32_t *uni_rung;                      // per group: the rung all its tiles take, or 0xffffffff
	uint32_t *tile_choice;                   // outputs: per tile
	unsigned long long *group_lambda, *group_bytes, *group_sse;  // per group
	uint32_t *group_flags;
};

// Pixel windows of files (pxz_decode_windows_device, pxz_expand_windows_device): one entry per window of the call.  A window
// covers tile columns [c0, c0 + ccols) and tile rows [r0, r0 + crows) of its image; its covered tiles are numbered row-major
// inside that grid from tile0 on, its covered tile rows from row0 on (pxz_window_layout).  The entry carries its image's
// geometry, so that the kernels read one table.
struct WindowEntry {
	uint64_t offset;                // bytes from the call's base pointer to the window's first output pixel
	uint32_t tile0, row0;           // first covered tile / first covered tile row of the window in the call
	uint32_t image;                 // the file the window reads
	uint32_t x, y, w, h, pitch;     // the pixel rectangle in that image; bytes between OUTPUT rows
	uint32_t c0, r0, ccols, crows;  // the covered tile grid
	uint32_t img_w, img_h, cols, rows, edge_w, edge_h;  // the image: what its header must say, its whole grid
};

// window_expand_kernel (pxz_window.hip): the covered tiles of the call's windows back to their full sizes, and of each the
// part inside its window to the window's output.  The wave's image is always in LDS (no HBM form).
struct WindowExpandArgs : TileResizeArgs {
	const WindowEntry *windows;
	uint32_t n_windows;
	uint8_t *base;                    // window k at base + windows[k].offset, windows[k].pitch between rows
	uint32_t *window_flags;           // per window 1 for a covered tile whose stored size is invalid, or null
};

// patch_kernel (pxz_patch.hip, pxz_patch_windows_device): the covered tiles of the call's windows rebuilt at full size in LDS,
// the windows' new pixels written over them, and each shrunk again, one tile per block.  r is the re-shrink's argument set over
// the windows' flat tile space: r.v the shrink side (r.v.images and r.v.n_images are unused: the owners are the windows;
// r.v.factor is unused: the factor is factor[0], where the shared tail reads it), r.x the expand side, r.image_flags unused.
struct PatchArgs {
	ReshrinkArgs r;
	const WindowEntry *windows;       // offset and pitch describe the INPUT rectangle of new pixels at patch_base
	uint32_t n_windows;
	const uint8_t *patch_base;
	uint32_t *window_flags;           // per window 1 for a covered tile whose stored size is invalid, or null
	float factor[1];
};

// The splice of pxz_splice_windows_device (pxz_patch.hip): old files and the new covered tiles' records -> new files.  The host
// knows the STRUCTURE of every output file -- a list of pieces in file order, each a byte span of the old files or of the staging
// files (the hulls' tiles written by the varied writer, one file per window) -- and the device the LENGTHS: a piece runs between
// two bounds, each of which a kernel turns into a byte offset.
//   kFileStart, kFileEnd  a = image: the old file's first byte / the byte behind its last;
//   kRow                  a = a window of the image, b = tile row r of the IMAGE, 0 .. rows: where row r starts in the old file (the
//                         header, the line table and the lengths of the rows before r); r = rows: where the last row ends;
//   kRecStart, kRecEnd    a = covered tile: the first byte of its old record ("block") / the byte behind its end marker, from rec_off
//                         and rec_len as window_index_kernel left them (rec_off: the first op byte, 23 bytes into the record;
//                         rec_len: the op bytes, 8 bytes of end marker behind them);
//   kStageRow             a = window, b = covered row j, 0 .. crows: where row j of the window's staging file starts.
struct SpliceBound {
	static constexpr uint32_t kFileStart = 0, kFileEnd = 1, kRow = 2, kRecStart = 3, kRecEnd = 4, kStageRow = 5;
	uint32_t kind, a, b;
};
struct SplicePiece {
	SpliceBound lo, hi;          // [lo, hi) of the old files, or of the staging files when lo.kind == kStageRow
	uint32_t image;              // the output file the piece belongs to
	uint32_t first;              // 1: the first piece of its file
};
// one tile row of an image that a window touches: its new length is the old one, minus the old records of the covered tiles of
// each window in it, plus that window's staging row; the windows are parts [part0, part0 + n_parts)
struct SpliceRow {
	uint32_t image, window, row;  // window: any window of the image (it carries the image's geometry)
	uint32_t part0, n_parts;
};
struct SpliceRowPart {
	uint32_t window, crow;        // covered row crow of the window: tiles tile0 + crow * ccols .. + ccols - 1
};
struct SpliceArgs {
	const WindowEntry *windows;
	uint32_t n_windows, n_images, n_tiles, n_pieces, n_rows;
	const SplicePiece *pieces;
	const SpliceRow *rows;
	const SpliceRowPart *parts;
	const uint8_t *files;                          // the old files
	const unsigned long long *file_offsets;        // n_images + 1
	const unsigned long long *rec_off;             // the reader's scratch, per covered tile
	const uint32_t *rec_len;
	const uint32_t *new_w, *new_h;                 // the new covered tiles' stored sizes
	const uint32_t *reader_flags, *patch_flags;    // per window, or null
	const uint8_t *stage;                          // the staging files
	const unsigned long long *stage_offsets;       // n_windows + 1
	unsigned long long stage_capacity;
	unsigned long long *piece_src, *piece_len, *piece_dst;  // per piece (piece_dst: n_pieces + 1); piece_src bit 63: a staging span
	uint32_t *image_flags;                         // per image: the OR of its windows' flags (zeroed before the first kernel)
	uint8_t *out;
	unsigned long long capacity;
	unsigned long long *out_file_offsets;          // n_images + 1
};

// Decode at reduced scale (pxz_expand_varied_scaled_frames_device, pxz_expand_windows_scaled_device; pxz_scaled_expand.hip):
// the stored tiles of a flat tile space resized to ceil(full / 2^shift) on each axis and written at (x0, y0) >> shift, the
// shift being the owner's (an image's, or a window's).
// One axis table per (target size, stored size) pair the call can meet: dir[slot[target] * stride + stored], indexed as
// VariedExpandTableSet's with the target in the place of the full size; `mixed` is the same directory for the axis that
// SHRINKS while the other one grows (the upscale flag set on a down-scaling axis: another kernel for Triangle, the same
// entry as dir's for the other filters).  Entries of stored == target (that axis is not resampled) are zero.
struct ScaledTab {
	uint32_t start_off;      // into starts[] / sizes[] (nearest: starts[] is the source index)
	uint32_t coeff_off;      // into coeffs[]: target * window weights
	uint16_t window;         // weights per output sample in coeffs[]
	uint16_t precision;
	uint16_t taps;           // the widest window of the table as built (clipped to the stored size)
	uint16_t wdw;            // dwords of one staged window: 1 + ceil(taps / 2); Nearest: 1
};
// one image of a scaled varied call: its grid is the FILE's, offset and pitch describe the scaled output
struct ScaledImage {
	uint64_t offset;
	uint32_t tile0, pitch;
	uint32_t cols, rows, edge_w, edge_h;
	uint32_t shift, pad;
};
// one window of a scaled windows call: the covered grid is the full-resolution rectangle's (pxz_window_layout), the rectangle
// itself is kept in scaled pixels, [x0, x1) x [y0, y1) of the scaled image
struct ScaledWindow {
	uint64_t offset;
	uint32_t tile0, pitch;
	uint32_t x0, y0, x1, y1;
	uint32_t c0, r0, ccols, cols, rows, edge_w, edge_h;
	uint32_t shift;
};
struct ScaledExpandArgs {
	uint32_t bw, bh, slot_bytes, filter;
	const uint32_t *slot;
	const ScaledTab *dir, *mixed;
	uint32_t stride;
	const uint16_t *starts, *sizes;
	const int16_t *coeffs;
	uint32_t win_dw;                  // dwords of the staged windows of one axis (scaled_window_dw, pxz_scaled_tile.h)
	uint32_t tile_dw;                 // dwords of one wave's image (scaled_tile_dw)
	uint32_t t0_dw;                   // (set by the launch) dwords of the owners' first tiles kept in LDS, 0: read from the table
	uint32_t *status;                 // bit 0: a tile's stored size is 0 or exceeds its FULL place
	uint32_t n_tiles, n_owners;
	const uint32_t *tile_w, *tile_h;  // per tile: stored size
	const uint8_t *slots;             // per tile slot_bytes, tile_w * tile_h * channels valid, tightly packed
	const ScaledImage *images;        // scaled_expand_kernel's owners
	const ScaledWindow *windows;      // scaled_window_expand_kernel's
	uint8_t *base;                    // owner k at base + offset, pitch between rows
	uint32_t *flags;                  // per owner 1 for a tile whose stored size is invalid, or null
};

struct SynthArgs {
	uint8_t *dst;
	uint64_t frame_stride;
	uint32_t pitch, width, height, channels, n_frames, first_frame, dist;
};

}  // namespace pxz
