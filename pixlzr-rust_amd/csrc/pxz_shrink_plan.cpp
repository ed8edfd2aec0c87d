// pxz_shrink_plan.cpp — the route of a single-geometry shrink call, see pxz_shrink_plan.h.  Pure host code.
#include "pxz_shrink_plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace pxz {

namespace {

uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

int refuse(char *text, size_t text_len, int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(text, text_len, fmt, ap);
	va_end(ap);
	return code;
}

// The part of the plan that stands before the tables in the order of checks: the grid and its refusals, the layout of the frames
// as given, and whether an RGB batch is a candidate for the RGBA kernels.
struct Front {
	TileGrid grid;
	bool conv;             // pixels wanted, a convolution
	bool covers;           // oklab_covers_rgba
	bool shape;            // a tile shape whose kernels want RGBA rows of 16-byte multiples: widen RGB, re-pitch RGBA.  (PXZ_NO_OKLAB_GENERAL
	                       //   does not enter here, as it never did: the batch is widened or re-pitched and then finds no detector)
	ShrinkLayout given;    // the layout for the caller's channel count
	bool rgb_must_widen;   // the RGB layout with its own detector planes does not run; the widened RGBA one without them does
	bool widen;            // RGB rides the RGBA kernels -- if opaque_stays allows (needs_opaque)
	bool needs_opaque;
};

int front(const ShrinkRequest &q, const Knobs &k, Front *o, char *text, size_t text_len)
{
	const pxz_frames &f = *q.frames;
	const pxz_params &p = *q.params;
	const uint32_t bw = p.block_w, bh = p.block_h;
	o->grid = tile_grid(f.width, f.height, bw, bh, f.n_frames);
	const TileGrid &g = o->grid;
	// (the detector's refusal is reported first, also for a batch of too many tiles)
	if (p.mode == PXZ_MODE_SHRINK_DIRECTIONALLY && (g.edge_w < 2 || g.edge_h < 2 || bw < 2 || bh < 2))
		return refuse(text, text_len, PXZ_ERR_TILE_TOO_SMALL,
		              "directional detector needs tiles of at least 2x2 px (edge tile is %ux%u); the reference panics here", g.edge_w, g.edge_h);
	if (g.tiles > kShrinkMaxTiles) return refuse(text, text_len, PXZ_ERR_UNSUPPORTED, "too many tiles");
	if (bw > 0xffffu || bh > 0xffffu) return refuse(text, text_len, PXZ_ERR_UNSUPPORTED, "block side above 65535");
	o->conv = q.want_pixels && p.filter != PXZ_FILTER_NEAREST;
	o->covers = oklab_covers_rgba(f, p, k);
	o->shape = square_fast(bw, bh) || oklab_shape(p.mode, bw, bh);
	const bool by = p.mode == PXZ_MODE_SHRINK_BY;
	o->given = shrink_layout(bw, bh, o->conv, by && !(o->covers && f.channels == 4), q.n_cus, k);
	o->rgb_must_widen = false;
	if (o->given.refused) {
		if (o->covers && f.channels == 3 && !k.no_widen && !shrink_layout(bw, bh, o->conv, false, q.n_cus, k).refused)
			o->rgb_must_widen = true;
		else
			return refuse(text, text_len, PXZ_ERR_UNSUPPORTED,
			              "a %ux%u tile needs %llu B of LDS (limit 163840) and has too many pixels for the HBM-resident form (limit 2^20 - 1)", bw, bh,
			              (unsigned long long)o->given.lds_bytes);
	}
	o->widen = f.channels == 3 && o->shape && !k.no_widen;
	// (16x16, 32x32, 64x64 tiles: the fast kernels and the Oklab detector read RGB themselves, when the rows are 4-byte aligned)
	if (o->widen && square_fast(bw, bh) && !o->rgb_must_widen && !k.no_native_rgb && rows_aligned4(q.src_low_bits, f)) o->widen = false;
	// widened, a constant-255 alpha goes through the filter's windows: the tiles are the RGB ones only if it comes back as 255
	o->needs_opaque = o->widen && o->conv;
	return PXZ_OK;
}

// these frames as tightly packed RGBA with rows of a 16-byte multiple (what the fast kernels and the block-cooperative Oklab
// detector want)
pxz_frames rgba16_frames(const pxz_frames &frames)
{
	pxz_frames f = frames;
	f.channels = 4;
	f.pitch_bytes = (frames.width * 4u + 15u) & ~15u;
	f.frame_stride_bytes = (uint64_t)f.pitch_bytes * frames.height;
	return f;
}

}  // namespace

ShrinkLayout shrink_layout(uint32_t bw, uint32_t bh, bool conv, bool lab, uint32_t n_cus, const Knobs &k)
{
	auto round2 = [](uint32_t v) { return (v + 1u) & ~1u; };
	auto skew = [](uint32_t v) { return (v & 15u) == 0 ? v + 2u : v; };  // keep rows off a common LDS bank
	ShrinkLayout l{};
	l.rs = skew(round2(ceil_div(bw, 2)));
	l.plane_dw = l.rs * bh;
	l.hps = skew(round2(ceil_div(bh, 2)));
	l.tmp_dw = conv ? ceil_div(bw, 2) * l.hps : 0;
	// (without lab every tile's Oklab value comes from oklab_kernel launches -- the generic kernel then needs no f32 planes of its
	// own, which is what limits shrink_by to ~7000-pixel tiles otherwise)
	l.lab_dw = lab ? 3 * bw * bh : 0;
	// planes | max(transposed planes, Oklab scratch) | slack for zero-weight over-reads past the last row
	const uint32_t scratch = 4 * l.tmp_dw > l.lab_dw ? 4 * l.tmp_dw : l.lab_dw;
	l.tile_dw = (4 * l.plane_dw + scratch + 4 * l.rs + 4 * l.hps + 3u) & ~3u;
	const uint32_t nw = layout_waves(bw * bh);
	l.lds_bytes = (uint64_t)l.tile_dw * 4u + (nw > 1 ? 16u * nw : 0u);
	if (!l.in_lds()) {
		// (round 4) a tile image beyond LDS lives in HBM, one per block of the generic kernel: any block size the reference's CLI
		// accepts runs (src/bin/main.rs:19-24), at the speed of L2 round trips.  The kernel's index arithmetic (small_div, RowWalker)
		// holds below 2^20 pixels per tile; the grid is capped so that the images stay under 2 GB.
		if ((uint64_t)bw * bh >= kBigTilePixels || k.no_big_tiles) {
			l.refused = true;
			return l;
		}
		uint64_t blocks = (2ull << 30) / ((uint64_t)l.tile_dw * 4u);
		if (blocks > 2ull * n_cus) blocks = 2ull * n_cus;
		if (blocks < 1) blocks = 1;
		l.big_blocks = (uint32_t)blocks;  // (capped by the tile count in the route)
	}
	return l;
}

bool shrink_ladder_in_lds(const pxz_params &p, bool want_pixels, uint64_t tiles, uint32_t n_cus, const Knobs &k, ShrinkLayout *bare)
{
	// (the sides first: beyond 65535 the layout's 32-bit products wrap)
	if (p.mode != PXZ_MODE_SHRINK_BY || tiles > kShrinkMaxTiles || p.block_w > 0xffffu || p.block_h > 0xffffu) return false;
	const bool conv = want_pixels && p.filter != PXZ_FILTER_NEAREST;
	*bare = shrink_layout(p.block_w, p.block_h, conv, false, n_cus, k);
	return shrink_layout(p.block_w, p.block_h, conv, true, n_cus, k).in_lds() && bare->in_lds();
}

bool shrink_plan_needs_opaque_stays(const ShrinkRequest &q, const Knobs &k)
{
	Front fr;
	char text[8];
	return front(q, k, &fr, text, sizeof text) == PXZ_OK && fr.needs_opaque;
}

int shrink_plan(const ShrinkRequest &q, const Knobs &k, ShrinkRoute *route, char *text, size_t text_len)
{
	Front fr;
	const int rc = front(q, k, &fr, text, text_len);
	if (rc != PXZ_OK) return rc;
	const pxz_frames &f = *q.frames;
	const pxz_params &p = *q.params;
	const uint32_t bw = p.block_w, bh = p.block_h;
	const bool by = p.mode == PXZ_MODE_SHRINK_BY;
	ShrinkRoute &r = *route;
	r = ShrinkRoute{};
	r.grid = fr.grid;
	const uint32_t n_tiles = (uint32_t)fr.grid.tiles;

	// ---- input form ----
	bool widen = fr.widen && (!fr.needs_opaque || q.opaque_stays);
	if (fr.rgb_must_widen && !widen)
		return refuse(text, text_len, PXZ_ERR_UNSUPPORTED, "a %ux%u RGB tile needs more LDS than there is (and this filter cannot run it as RGBA)", bw, bh);
	ShrinkLayout widened{};
	if (widen) {
		widened = shrink_layout(bw, bh, fr.conv, by && !fr.covers, q.n_cus, k);
		if (widened.refused) widen = false;  // e.g. four planes of a large tile exceed LDS
	}
	// RGBA frames whose rows (or first byte, or frame stride) are not 16-byte multiples would miss the fast kernels and the
	// block-cooperative Oklab detector: one device-to-device 2D copy into aligned scratch first (0.4 ms per GB against 5-50x on
	// the kernels)
	const bool repitch = !widen && f.channels == 4 && fr.shape && !k.no_repitch && !rows_aligned16(q.src_low_bits, f);
	r.input = widen ? ShrinkInput::Widened : repitch ? ShrinkInput::Repitched : ShrinkInput::AsGiven;
	r.frames = r.input == ShrinkInput::AsGiven ? f : rgba16_frames(f);
	r.channels = r.frames.channels;
	r.frame_stride = frame_stride_of(r.frames);
	r.rgba_bytes = r.input == ShrinkInput::AsGiven ? 0 : (size_t)r.frames.frame_stride_bytes * f.n_frames;
	r.slots4_bytes = widen && q.want_pixels ? (size_t)n_tiles * bw * bh * 4u : 0;
	r.layout = widen ? widened : fr.given;
	const uint32_t low_bits = r.input == ShrinkInput::AsGiven ? q.src_low_bits : 0u;  // (the handle's scratch is 256-byte aligned)
	r.factor = q.identity ? 1.0f : p.factor;
	r.scale2 = q.identity ? 1.0f : 10.0f;  // BASE_FACTOR, pixlzr.rs:15; (x * 1) * 1 is x exactly: the identity closure

	// ---- scratch ----
	r.sums_bytes = (size_t)n_tiles * 8u;
	r.work_bytes = (2u * (size_t)n_tiles + kWorkList + 4u) * 4u + 64u + 4608u * 8u;  // + diagnostic stamps (8 phase sums + 256 blocks x 17 qwords)
	// + the 2 KB spare bytes of the detector's copies (ahead_spare) + the list of clone_split64_kernel (8 + n_tiles dwords)
	r.work_total_bytes = r.work_bytes + 2048u + 8u + (8u + (size_t)n_tiles) * 4u;
	r.big_blocks = r.layout.big_blocks < n_tiles ? r.layout.big_blocks : n_tiles;
	r.bigscratch_bytes = (size_t)r.big_blocks * r.layout.tile_dw * 4u;

	// ---- transparency ----
	// Without the caller's hint: the last finished launch reported how many full tiles had any (one dword in pinned memory, written
	// by the worklist kernel).  Past ~2000 tiles shrink32a_kernel pays for its launch.  Either way the results are the same; only
	// the kernel that produces them differs.  The counts are only trusted when they come from a launch of THIS configuration: the
	// kernel writes the signature beside them.
	uint32_t factor_bits;
	std::memcpy(&factor_bits, &r.factor, 4);
	r.stats_sig = ((n_tiles * 2654435761u) ^ (bw << 20) ^ (bh << 8) ^ (p.mode << 31) ^ (r.channels << 28) ^ f.width ^ (f.height * 40503u) ^
	               (p.filter * 0x9e3779b1u) ^ (factor_bits * 31u)) | 1u;
	const bool stats_ours = q.have_stats && q.stats[2] == r.stats_sig;
	const uint32_t seen_transparent = stats_ours ? q.stats[0] : 0u;
	r.expect_listed = stats_ours ? q.stats[1] : 0xffffffffu;
	r.alpha_kernel = ((p.reserved & PXZ_HINT_TRANSPARENCY) != 0 || seen_transparent >= kAlphaKernelTiles) && !k.no_alpha_kernel ? 1u : 0u;
	// ... and past half of the tiles the lean kernel would only read, test and list them: the four-plane kernel goes first
	r.alpha_first = r.alpha_kernel && seen_transparent >= n_tiles / 2u && seen_transparent >= kAlphaKernelTiles && !k.no_alpha_first ? 1u : 0u;
	r.write_stats = !q.quiet_stats;

	// ---- the fast kernels' region and the detector's rows ----
	const TileGrid &g = r.grid;
	const bool sq = square_fast(bw, bh);
	const bool aligned16 = r.channels == 4 && rows_aligned16(low_bits, r.frames);
	// RGB frames on the square fast paths (round 2): 12-byte pixel quads, rows 4-byte aligned
	const bool rgb_native = r.channels == 3 && sq && !k.no_native_rgb && rows_aligned4(low_bits, r.frames);
	r.ok_bands = (bw * bh + 255u) / 256u;
	// rows of a ragged last tile row the square detectors can take: whole 256-px bands (oklab_kernel), for 64-px tiles whole
	// 512-px super-bands (oklab2_kernel<64>: four producer waves x two rows)
	const uint32_t ok_row_quantum = bw == 64u ? 8u : (bw <= 256u ? 256u / bw : 1u);
	if (rgb_native || (aligned16 && (sq || general_oklab(p.mode, bw, bh, k)))) {
		r.full_cols = g.edge_w == bw ? g.cols : g.cols - 1;
		r.full_rows = g.edge_h == bh ? g.rows : g.rows - 1;
		// the square detectors also take a ragged last row of whole bands
		r.ok_rows = sq && g.edge_h % ok_row_quantum == 0 ? g.rows : r.full_rows;
	}
	// (a pitch whose lane offsets leave 32 bits: no fast path, as for an unaligned batch)
	if (!fast32_lane_offset_fits(r.frames.pitch_bytes)) r.full_cols = r.full_rows = r.ok_rows = 0;

	// ---- detector ----
	// INVARIANT B: the detector's loads are unconditional, so it only runs on a frame of at least one block each way.
	// full_cols != 0 && full_rows != 0 says so: a frame narrower (lower) than a block has one ragged column (row) and no full one.
	const bool detect = by && r.full_cols != 0 && r.full_rows != 0 && !k.no_oklab32;
	// 64x64 tiles are converted by oklab2_kernel<64> (round 3), which parks nothing in HBM; PXZ_OKLAB_V1 keeps oklab_kernel<64>
	const bool parks64 = !(bw == 64u && bh == 64u) || k.oklab_v1;
	// a tile of more than 1024 pixels does not fit the registers between the detector's two passes: 13 dwords per pixel quad in HBM
	const size_t parked = r.ok_bands > 4u && parks64 ? (size_t)n_tiles * r.ok_bands * 3328u : 0u;
	r.regions[0] = {1u, 1u, false, 0u, 0u};
	r.regions[1] = {2u, 2u, false, 0u, 0u};
	r.regions[2] = {3u, 4u, false, 0u, 0u};
	r.detector = !detect ? ShrinkDetector::None : r.channels == 4 ? ShrinkDetector::Rgba : ShrinkDetector::RgbNative;
	// INVARIANT A: clone_ahead lets the fast kernels skip tiles as "already in their slots".  That is only sound while
	// every tile a fast kernel may skip (tx < full_cols, ty < full_rows) was taken by the detector in this launch (tx < full_cols,
	// ty < ok_rows): clone_ahead is set nowhere but here, beside a detector, and ok_rows >= full_rows by construction above.
	const bool may_clone = q.want_pixels && !k.oklab_v1 && !k.no_clone_ahead;
	const bool right = r.full_cols < g.cols, bottom = r.full_rows < g.rows && r.ok_rows < g.rows, corner = r.full_cols < g.cols && r.full_rows < g.rows;
	if (r.detector == ShrinkDetector::Rgba) {
		// The ragged edge of the grid -- right column (edge_w x bh), bottom row (bw x edge_h), corner tile -- goes through the
		// same detector with run-time geometry, one launch per region (tile rows that are not whole pixel quads are walked
		// padded).  Without it the edge runs its chains in the generic kernel: four lanes per tile, ~0.1-0.5 ms of latency per
		// launch whatever the batch.
		const struct { uint32_t w, hh, per_frame; bool wanted; } edge[3] = {
		    {g.edge_w, bh, r.full_rows, right}, {bw, g.edge_h, r.full_cols, bottom}, {g.edge_w, g.edge_h, 1u, corner}};
		r.okscratch_bytes = parked;
		for (int i = 0; i < 3; ++i) {
			const uint32_t wp = (edge[i].w + 3u) & ~3u;  // rows are walked in whole quads (the padding counts as zeros)
			ShrinkRegion &e = r.regions[i];
			e.wanted = edge[i].wanted && edge[i].per_frame != 0u && bw % 4u == 0u && wp * edge[i].hh <= 16384u && !k.no_oklab_edges;
			e.bands = (wp * edge[i].hh + 255u) / 256u;
			e.count = f.n_frames * edge[i].per_frame;
			if (e.wanted && e.bands > 4u && (size_t)e.count * e.bands * 3328u > r.okscratch_bytes) r.okscratch_bytes = (size_t)e.count * e.bands * 3328u;
		}
		r.clone_ahead = sq && may_clone ? 1u : 0u;
	} else if (r.detector == ShrinkDetector::RgbNative) {
		// RGB, 16x16 / 32x32 / 64x64: oklab2_kernel<16 | 32, 3> / oklab_kernel<64, 0, 3> for the full tiles; a ragged edge keeps its
		// chains in the generic kernel.  An RGB lane's six bytes are two stores, which costs the 16x16 detector more than its
		// shrink kernel gains -- 8 x 8K: 1.151 against 1.141 ms; 32x32 1.052 against 1.072, 64x64 1.20 against 1.37
		r.okscratch_bytes = parked;
		r.clone_ahead = bw != 16u && may_clone ? 1u : 0u;
	}
	if (by && r.layout.lab_dw == 0) {
		// The layout was sized without the generic kernel's detector planes because oklab_covers_rgba said the detector's launches
		// leave it no tile.  The one way past that is a pitch beyond fast32_lane_offset_fits, which takes every launch away: refused
		// here, as it always was.
		const uint32_t edges = r.ok_edges();
		const bool covered = r.detector != ShrinkDetector::None && (!right || (edges & 1u)) && (!bottom || (edges & 2u)) && (!corner || (edges & 4u));
		if (!covered) return refuse(text, text_len, PXZ_ERR_UNSUPPORTED, "internal: Oklab values missing for a layout sized without detector planes");
	}
	return PXZ_OK;
}

}  // namespace pxz
