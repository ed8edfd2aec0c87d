// pxz_launch.h — the host-callable launchers and size helpers of the kernel units, declared once: pxz_api.cpp calls them and
// every .hip file that defines one includes this header, so the compiler holds each definition against its declaration.
// Default arguments live here only.  launch_with_lds is the launch phrase of the kernels whose dynamic LDS can exceed 64 KB.
#pragma once
#include <hip/hip_runtime.h>

#include "pxz_internal.h"

namespace pxz {
hipError_t launch_shrink(const ShrinkArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
hipError_t launch_synth(const SynthArgs &s, hipStream_t stream);
hipError_t launch_tree_decide(const TreeArgs &a, hipStream_t stream);
hipError_t launch_tree_rects(const TreeRectArgs &a, hipStream_t stream);
hipError_t launch_oklab_pixels(const uint32_t *px, uint32_t n, float *out, uint32_t n_cus, hipStream_t stream);
hipError_t launch_finish(const FinishArgs &f, hipStream_t stream);
bool fast32_applicable(const ShrinkArgs &a, uint32_t channels);
bool fast64_applicable(const ShrinkArgs &a, uint32_t channels);
bool fast16_applicable(const ShrinkArgs &a, uint32_t channels);
hipError_t launch_expand(const ExpandArgs &a, uint32_t n_cus, hipStream_t stream);
hipError_t launch_ladder(const LadderArgs &a, uint32_t channels, uint32_t nw, uint32_t n_cus, hipStream_t stream);
hipError_t launch_decode(const DecodeArgs &a, bool bins_clean, hipStream_t stream);
hipError_t launch_decode_varied(const DecodeArgs &a, const VariedImage *images, uint32_t n_rows, uint32_t *image_flags, bool bins_clean,
                                hipStream_t stream);
// the same over pixel windows: n_windows entries, n_rows covered tile rows and a.n_tiles covered tiles in all, a.n_frames files
hipError_t launch_decode_windows(const DecodeArgs &a, const WindowEntry *windows, uint32_t n_windows, uint32_t n_rows, uint32_t *window_flags,
                                 bool bins_clean, hipStream_t stream);
hipError_t launch_window_expand(const WindowExpandArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
hipError_t launch_varied_expand(const VariedExpandArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
uint32_t varied_expand_tile_dw(uint32_t bw, uint32_t bh, uint32_t wdw);
// the LDS form's grid for n_tiles tiles of n_images images, one wave per tile: *t0_dw = dwords of the images' first tiles a
// block keeps in LDS (0: more images than it holds); threads == 0: one wave's image does not fit
LaunchGeom varied_expand_geom(uint32_t n_images, uint32_t n_tiles, uint32_t tile_dw, uint32_t n_cus, uint32_t *t0_dw);
// decode at reduced scale (pxz_scaled_expand.hip): one launch over a.images, or over a.windows when that is set; the wave's
// image (a.tile_dw: scaled_tile_dw, pxz_scaled_tile.h) is always in LDS, on varied_expand_geom's grid
hipError_t launch_scaled_expand(const ScaledExpandArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
// Dwords of the staged windows of one axis for blocks whose longer side is `side`, tables whose kernel has the given support
// (0: Nearest) and scales 2^0 .. 2^max_shift: at scale 2^k an axis has at most ceil(side / 2^k) output samples of at most
// min(side, 2 * ceil(support * 2^k) + 1) taps each (an up-scaling window: 2 * ceil(support) + 1), a header dword before
// the i16 pairs.
inline uint32_t scaled_window_dw(uint32_t side, uint32_t support, uint32_t max_shift)
{
	uint32_t most = 0;
	for (uint32_t k = 0; k <= max_shift && k < 32u; ++k) {
		const uint32_t outs = (uint32_t)(((uint64_t)side + (1ull << k) - 1u) >> k);
		uint64_t taps = support ? 2ull * ((uint64_t)support << k) + 1u : 1u;
		if (taps > side) taps = side;
		const uint32_t dw = outs * (1u + (support ? ((uint32_t)taps + 1u) / 2u : 0u));
		if (dw > most) most = dw;
	}
	return most;
}

// dwords of one wave's image of scaled_resize_tile (its layout: pxz_scaled_tile.h); 0xffffffff: beyond any LDS
inline uint32_t scaled_tile_dw(uint32_t bw, uint32_t bh, uint32_t win_dw)
{
	const uint64_t dw = (2ull * bw * bh + 2ull * win_dw + bw + 3u) & ~3ull;
	return dw > 0x0fffffffull ? 0xffffffffu : (uint32_t)dw;
}
hipError_t launch_distortion(const DistortionArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
hipError_t launch_widen(const WidenArgs &a, hipStream_t stream);
hipError_t launch_narrow(const NarrowArgs &a, hipStream_t stream);
hipError_t launch_pack(const PackArgs &a, hipStream_t stream);
hipError_t launch_oklab(const ShrinkArgs &a, uint32_t n_cus, hipStream_t stream, uint32_t channels = 4);
hipError_t launch_qoi(const QoiArgs &a, bool bins_clean, uint32_t n_cus, hipStream_t stream);
hipError_t launch_qoi_varied(const QoiArgs &a, const VariedWriterArgs &varied, bool bins_clean, uint32_t n_cus, hipStream_t stream);
hipError_t launch_varied(const VariedArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
hipError_t launch_varied_ladder(const VariedLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
// LDS bytes of one block of varied_ladder_kernel (what the host holds against the CU's 160 KB before it launches)
uint32_t varied_ladder_lds_limit_bytes(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t channels);
hipError_t launch_reshrink(const ReshrinkArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
hipError_t launch_reshrink_ladder(const ReshrinkLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
// LDS bytes of one block of reshrink_kernel (rung_channels 0) or of reshrink_ladder_kernel (rung_channels: the tiles' channel
// count) for blocks of bw x bh whose staged windows take wdw dwords, from the layout function the kernels and their launches
// use (what the host holds against kLdsPerCu before it launches); 0xffffffff: a plane of bw * bh dwords above 64 KB
uint32_t reshrink_lds_bytes(uint32_t mode, uint32_t bw, uint32_t bh, uint32_t rung_channels, uint32_t wdw);
// patch of pixel windows (pxz_patch.hip): one launch whatever the windows; the block's LDS is reshrink_kernel's (rung_channels 0)
hipError_t launch_patch(const PatchArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
// the splice behind it (pxz_patch.hip): five launches whatever the images, windows and pieces; s.image_flags zeroed by the caller
hipError_t launch_splice(const SpliceArgs &s, uint32_t n_cus, hipStream_t stream);
// re-tile (pxz_retile.hip): one launch; and the LDS bytes of one block of retile_kernel for source blocks of sbw x sbh whose staged
// windows take wdw dwords and destination blocks of dbw x dbh, from retile_lds (pxz_varied_tile.h), the layout function the kernel and
// its launch use (what the host holds against kLdsPerCu before it launches); 0xffffffff: a plane of either block above 64 KB
hipError_t launch_retile(const RetileArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
uint32_t retile_lds_bytes(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t wdw);
// re-tile ladder (pxz_retile_ladder.hip): one launch whatever the rungs; and the LDS bytes of one block of retile_ladder_kernel,
// from retile_ladder_lds (pxz_varied_tile.h) with the rungs' channel count, under the conventions of retile_lds_bytes
hipError_t launch_retile_ladder(const RetileLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
uint32_t retile_ladder_lds_bytes(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t channels, uint32_t wdw);
hipError_t launch_reshrink_distortion(const ReshrinkDistortionArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
// Dwords of one wave's image in reshrink_distortion_kernel for blocks of bw x bh whose staged windows take wdw dwords: three
// planes of bw * bh dwords (the reference and varied_resize_tile's two) and the windows of both axes.  The kernel, its launch,
// the entry point's check and the size query all take the layout from here.  0xffffffff: beyond any LDS.
inline uint32_t reshrink_distortion_tile_dw(uint32_t bw, uint32_t bh, uint32_t wdw)
{
	const uint64_t dw = (3ull * bw * bh + (uint64_t)wdw * ((uint64_t)bw + bh) + 3u) & ~3ull;
	return dw > 0x0fffffffull ? 0xffffffffu : (uint32_t)dw;
}
// re-tile distortion (pxz_retile_distortion.hip): one launch whatever the sets; and the LDS bytes of one block of
// retile_distortion_kernel, from retile_distortion_lds (pxz_varied_tile.h), for source windows of wdw_src dwords and set windows of
// wdw_set, under the conventions of retile_lds_bytes
hipError_t launch_retile_distortion(const RetileDistortionArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
uint32_t retile_distortion_lds_bytes(uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t wdw_src, uint32_t wdw_set);
// fit to a budget (pxz_fit.hip): one rung per image, and the chosen rungs' tiles as a varied batch; one launch each
hipError_t launch_fit_select(const FitArgs &a, hipStream_t stream);
hipError_t launch_gather_rungs(const GatherArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
// fit to a budget per tile (pxz_tilefit.hip): the record lengths out of the writer's scratch (one launch); the select, a chain
// of 3 + kTileFitSteps + 1 launches whatever the sizes; the gather with a choice per tile (one launch)
hipError_t launch_record_bytes(const RecordBytesArgs &a, hipStream_t stream);
hipError_t launch_tilefit(const TileFitArgs &a, hipStream_t stream);
hipError_t launch_gather_tile_rungs(const GatherArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream);
size_t qoi_scratch_bytes(uint32_t n_tiles, uint32_t slot_px, uint32_t channels);
uint32_t qoi_bins_dwords();
uint32_t waves_per_tile(uint32_t bw, uint32_t bh);

// The grid of a tile-per-block kernel (four waves, grid-stride over n_tiles) whose block takes lds_bytes of a CU's LDS: as many
// blocks as the CUs hold at once, at most eight per CU; the rest of the tiles walk the grid-stride loop.
constexpr uint32_t kLdsPerCu = 160u * 1024u;
inline uint32_t tile_blocks(uint32_t n_tiles, uint32_t lds_bytes, uint32_t n_cus)
{
	uint32_t per_cu = kLdsPerCu / lds_bytes;
	per_cu = per_cu < 1u ? 1u : (per_cu > 8u ? 8u : per_cu);
	const uint64_t cap = (uint64_t)n_cus * per_cu;
	return (uint32_t)(n_tiles < cap ? n_tiles : cap);
}

#ifdef __HIP__
// A launch with dynamic LDS: above 64 KB the kernel's limit is raised first.  Returns what the launch left behind.
template <class Kernel, class Args>
hipError_t launch_with_lds(Kernel kernel, uint32_t blocks, uint32_t threads, uint32_t lds_bytes, hipStream_t stream, const Args &a)
{
	if (lds_bytes > 64u * 1024u) {
		const hipError_t e =
			hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, stream, a);
	return hipGetLastError();
}
#endif
}  // namespace pxz
