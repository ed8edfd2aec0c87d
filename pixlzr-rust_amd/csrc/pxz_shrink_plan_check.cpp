// pxz_shrink_plan_check — the route of a single-geometry shrink call (pxz_shrink_plan.h) on the host.
//   pxz_shrink_plan_check.bin            reads one case per line from stdin, "key=value ..." (defaults below), and prints one line of
//                                        route fields per case; tests/test_shrink_plan_host.py holds the lines against expectations
//                                        written out by hand from the rules
//   pxz_shrink_plan_check.bin sweep      every block side of 1..130 and 256, 512, 1024 each way, both channel counts, both modes, with
//                                        and without pixels, aligned and odd addresses, frames of one to three tiles each way (whole
//                                        and ragged): asserts the two invariants the plan states (A: the detector's tiles are a
//                                        superset of what the fast kernels may skip; B: a detector only on a frame of at least one
//                                        block each way) and that a layout without detector planes has every tile's value covered.
//                                        Prints "ok <plans>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pxz_shrink_plan.h"

using namespace pxz;

static bool set_knob(Knobs &k, const std::string &name)
{
	struct { const char *n; bool Knobs::*f; } const table[] = {
	    {"no_alpha_kernel", &Knobs::no_alpha_kernel}, {"no_oklab_general", &Knobs::no_oklab_general}, {"no_oklab32", &Knobs::no_oklab32},
	    {"no_oklab_edges", &Knobs::no_oklab_edges}, {"no_repitch", &Knobs::no_repitch}, {"no_widen", &Knobs::no_widen},
	    {"no_native_rgb", &Knobs::no_native_rgb}, {"no_alpha_first", &Knobs::no_alpha_first}, {"no_big_tiles", &Knobs::no_big_tiles},
	    {"no_clone_ahead", &Knobs::no_clone_ahead}, {"oklab_v1", &Knobs::oklab_v1}};
	for (const auto &t : table)
		if (name == t.n) {
			k.*(t.f) = true;
			return true;
		}
	return false;
}

static const char *input_name(ShrinkInput i) { return i == ShrinkInput::AsGiven ? "given" : i == ShrinkInput::Widened ? "widened" : "repitched"; }
static const char *detector_name(ShrinkDetector d) { return d == ShrinkDetector::None ? "none" : d == ShrinkDetector::Rgba ? "rgba" : "rgb"; }

static int run_cases()
{
	char line[1024];
	while (fgets(line, sizeof line, stdin)) {
		if (line[0] == '#' || line[0] == '\n') continue;
		pxz_frames f{64, 64, 4, 0, 1, 0, 0};
		pxz_params p{32, 32, PXZ_MODE_SHRINK_DIRECTIONALLY, 4, 16.0f, 0};
		ShrinkRequest q{};
		q.want_pixels = true;
		q.n_cus = 256;
		q.opaque_stays = true;
		Knobs k{};
		uint32_t pitch = 0, seen = 0, listed = 0;
		uint64_t stride = 0;
		bool ladder = false;
		std::string sig = "none";
		for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
			char *eq = strchr(tok, '=');
			if (!eq) return 2;
			const std::string key(tok, eq), val(eq + 1);
			const unsigned long long v = strtoull(val.c_str(), nullptr, 0);
			if (key == "w") f.width = (uint32_t)v;
			else if (key == "h") f.height = (uint32_t)v;
			else if (key == "c") f.channels = (uint32_t)v;
			else if (key == "n") f.n_frames = (uint32_t)v;
			else if (key == "pitch") pitch = (uint32_t)v;
			else if (key == "stride") stride = v;
			else if (key == "bw") p.block_w = (uint32_t)v;
			else if (key == "bh") p.block_h = (uint32_t)v;
			else if (key == "mode") p.mode = (uint32_t)v;
			else if (key == "filt") p.filter = (uint32_t)v;
			else if (key == "factor") p.factor = strtof(val.c_str(), nullptr);
			else if (key == "hint") p.reserved = (uint32_t)v;
			else if (key == "px") q.want_pixels = v != 0;
			else if (key == "ident") q.identity = v != 0;
			else if (key == "low") q.src_low_bits = (uint32_t)v;
			else if (key == "cus") q.n_cus = (uint32_t)v;
			else if (key == "seen") seen = (uint32_t)v;
			else if (key == "listed") listed = (uint32_t)v;
			else if (key == "sig") sig = val;
			else if (key == "quiet") q.quiet_stats = v != 0;
			else if (key == "opaque") q.opaque_stays = v != 0;
			else if (key == "ladder") ladder = v != 0;
			else if (key == "knob") { if (!set_knob(k, val)) return 2; }
			else return 2;
		}
		f.pitch_bytes = pitch ? pitch : f.width * f.channels;
		f.frame_stride_bytes = stride ? stride : (uint64_t)f.pitch_bytes * f.height;
		q.frames = &f;
		q.params = &p;
		if (ladder) {
			ShrinkLayout bare{};
			const TileGrid g = tile_grid(f.width, f.height, p.block_w, p.block_h, f.n_frames);
			const bool in = shrink_ladder_in_lds(p, q.want_pixels, g.tiles, q.n_cus, k, &bare);
			printf("ladder=%d tile=%u\n", in ? 1 : 0, in ? bare.tile_dw : 0u);
			continue;
		}
		ShrinkRoute r;
		char why[256];
		int rc = shrink_plan(q, k, &r, why, sizeof why);
		if (rc == PXZ_OK && sig != "none") {  // the handle's statistics: of this configuration, or of another
			q.have_stats = true;
			q.stats[0] = seen;
			q.stats[1] = listed;
			q.stats[2] = sig == "own" ? r.stats_sig : r.stats_sig ^ 2u;
			rc = shrink_plan(q, k, &r, why, sizeof why);
		}
		if (rc != PXZ_OK) {
			printf("rc=%d text=%s\n", rc, why);
			continue;
		}
		printf("rc=0 needs_opaque=%d input=%s ch=%u pitch=%u stride=%llu rgba=%zu slots4=%zu", shrink_plan_needs_opaque_stays(q, k) ? 1 : 0,
		       input_name(r.input), r.channels, r.frames.pitch_bytes, (unsigned long long)r.frame_stride, r.rgba_bytes, r.slots4_bytes);
		printf(" rs=%u plane=%u hps=%u tmp=%u lab=%u tile=%u lds=%llu big=%u blocks=%u bigscratch=%zu", r.layout.rs, r.layout.plane_dw, r.layout.hps,
		       r.layout.tmp_dw, r.layout.lab_dw, r.layout.tile_dw, (unsigned long long)r.layout.lds_bytes, r.layout.big_blocks, r.big_blocks,
		       r.bigscratch_bytes);
		printf(" det=%s bands=%u okrows=%u clone=%u edges=%u", detector_name(r.detector), r.ok_bands, r.ok_rows, r.clone_ahead, r.ok_edges());
		for (const ShrinkRegion &e : r.regions) printf(" r%u=%u:%u", e.id, e.wanted ? e.count : 0u, e.wanted ? e.bands : 0u);
		printf(" okscratch=%zu full=%ux%u alpha=%u first=%u listed=%u stats=%d sums=%zu work=%zu factor=%g scale=%g\n", r.okscratch_bytes, r.full_cols,
		       r.full_rows, r.alpha_kernel, r.alpha_first, r.expect_listed, r.write_stats ? 1 : 0, r.sums_bytes, r.work_total_bytes, r.factor, r.scale2);
	}
	return 0;
}

static int run_sweep()
{
	uint32_t sides[133];
	for (uint32_t i = 0; i < 130; ++i) sides[i] = i + 1;
	sides[130] = 256, sides[131] = 512, sides[132] = 1024;
	const Knobs k{};
	long plans = 0;
	for (uint32_t bw : sides)
		for (uint32_t bh : sides)
			for (uint32_t c = 3; c <= 4; ++c)
				for (uint32_t mode = 0; mode <= 1; ++mode)
					for (int px = 0; px <= 1; ++px)
						for (uint32_t low = 0; low <= 1; ++low)
							for (uint32_t tx = 1; tx <= 3; ++tx)
								for (uint32_t ty = 1; ty <= 3; ++ty)
									for (int ragged = 0; ragged < 4; ++ragged) {
										const uint32_t w = tx * bw - ((ragged & 1) ? bw / 2u : 0u), hh = ty * bh - ((ragged & 2) ? bh / 2u : 0u);
										if (w == 0 || hh == 0) continue;
										pxz_frames f{w, hh, c, w * c, 2, 0, (uint64_t)w * c * hh};
										pxz_params p{bw, bh, mode, 4, 1.0f, 0};
										ShrinkRequest q{};
										q.frames = &f, q.params = &p, q.want_pixels = px != 0, q.src_low_bits = low, q.n_cus = 256;
										for (int opaque = 0; opaque <= 1; ++opaque) {
											q.opaque_stays = opaque != 0;
											if (!opaque && !shrink_plan_needs_opaque_stays(q, k)) continue;
											ShrinkRoute r;
											char why[256];
											const int rc = shrink_plan(q, k, &r, why, sizeof why);
											++plans;
											auto bad = [&](const char *what) {
												printf("FAIL %s: %ux%u frame, %ux%u block, c=%u mode=%u px=%d low=%u opaque=%d rc=%d %s\n", what, w, hh, bw, bh, c, mode, px, low,
												       opaque, rc, rc ? why : "");
												return 1;
											};
											if (rc != PXZ_OK) {
												if (strncmp(why, "internal", 8) == 0) return bad("a layout without detector planes and tiles without a value");
												continue;
											}
											const TileGrid &g = r.grid;
											// A: what a fast kernel may skip as copied (tx < full_cols, ty < full_rows) the detector took (tx < full_cols, ty < ok_rows)
											if (r.clone_ahead && (r.detector == ShrinkDetector::None || r.ok_rows < r.full_rows || r.full_cols == 0 || r.full_rows == 0 || !q.want_pixels))
												return bad("invariant A");
											if (r.full_cols > g.cols || r.full_rows > g.rows || r.ok_rows > g.rows) return bad("a region beyond the grid");
											// B: a detector (interior or edge launch) only on frames of at least one block each way
											if (r.detector != ShrinkDetector::None && (r.frames.width < bw || r.frames.height < bh)) return bad("invariant B");
											if (r.detector == ShrinkDetector::None && (r.ok_edges() != 0 || r.clone_ahead || r.okscratch_bytes != 0)) return bad("edges without a detector");
											// no_lab: every tile is either inside the detector's interior launch or in a wanted edge region
											if (mode == PXZ_MODE_SHRINK_BY && r.layout.lab_dw == 0) {
												const bool right = r.full_cols < g.cols, bottom = r.ok_rows < g.rows, corner = right && r.full_rows < g.rows;
												if (r.detector == ShrinkDetector::None || (right && !r.regions[0].wanted) || (bottom && !r.regions[1].wanted) ||
												    (corner && !r.regions[2].wanted))
													return bad("no_lab without cover");
											}
											if (r.input != ShrinkInput::AsGiven && (r.channels != 4 || (r.frames.pitch_bytes & 15u) != 0)) return bad("scratch frames not RGBA16");
										}
									}
	printf("ok %ld\n", plans);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 1 && strcmp(argv[1], "sweep") == 0) return run_sweep();
	return run_cases();
}
