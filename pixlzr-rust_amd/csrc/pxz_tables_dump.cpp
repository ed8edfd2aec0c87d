// pxz_tables_dump — runs the table builders of libpixlzr_hip.so (pxz_tables.h) over a fixed sweep of geometries and filters
// and prints one line per table set: the geometry, then element count and FNV-1a 64 hash of every array ("-": absent).
// tests/test_tables_host.py pins a digest of these lines per (family, filter).  With the argument `varied` it prints the
// directories of varied batches instead (tests/test_varied_host.py), with `varied_expand` those of their decode side
// (tests/test_varied_decode_host.py), with `thresholds` the level decision's float thresholds as bit patterns.
#include <array>
#include <cstring>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "pxz_tables.h"

namespace {

uint64_t fnv(const void *p, size_t n)
{
	uint64_t h = 14695981039346656037ull;
	for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const uint8_t *>(p)[i]) * 1099511628211ull;
	return h;
}

template <class T>
void arr(const char *name, const std::vector<T> &v)
{
	if (v.empty()) printf(" %s=-", name);
	else printf(" %s=%zu:%016llx", name, v.size(), (unsigned long long)fnv(v.data(), v.size() * sizeof(T)));
}

// every tile of the sweep with a full edge and ragged edges of 1, 3 and side / 2 + 1 (per axis, clamped to the side):
// {bw, bh, edge_w, edge_h}
std::vector<std::array<uint32_t, 4>> grids(bool expand)
{
	std::vector<std::pair<uint32_t, uint32_t>> tiles;
	for (uint32_t s : {1u, 2u, 3u, 4u, 7u, 8u, 12u, 16u, 24u, 31u, 32u, 33u, 48u, 63u, 64u, 96u, 128u}) tiles.emplace_back(s, s);
	tiles.insert(tiles.end(), {{32, 16}, {16, 32}, {64, 32}, {8, 64}});
	// (an expand set of a 4096-px side holds 4095 up-scaling tables of 4096 outputs: about 250 MB and seconds to build)
	if (!expand) tiles.insert(tiles.end(), {{4096, 4}, {4, 4096}});
	std::vector<std::array<uint32_t, 4>> g;
	for (const auto &t : tiles) {
		std::set<std::pair<uint32_t, uint32_t>> seen;
		for (uint32_t e : {0u, 1u, 3u, ~0u}) {
			auto edge = [e](uint32_t s) {
				const uint32_t v = e == 0 ? s : e == ~0u ? s / 2 + 1 : e;
				return v < s ? v : s;
			};
			const uint32_t ew = edge(t.first), eh = edge(t.second);
			if (seen.insert({ew, eh}).second) g.push_back({t.first, t.second, ew, eh});
		}
	}
	return g;
}

}  // namespace

// the (source size, level) directories of varied batches: sets of tile sides a batch can hold (full block sides and the
// distinct edges of its images), every filter
int dump_varied()
{
	const std::vector<std::vector<uint32_t>> side_sets = {
	    {16}, {1, 16}, {32}, {3, 17, 32}, {64}, {1, 2, 5, 33, 64}, {20, 48}, {1, 7, 19, 20, 47, 48}, {37, 61}, {2, 36, 37, 60, 61}, {128}};
	for (uint32_t f = 0; f < 5; ++f)
		for (const auto &sides : side_sets) {
			pxz::VariedTableSet s;
			if (!pxz::build_varied_tables(sides, f, &s)) return 1;
			uint32_t used = 0;
			for (const pxz::TreeAxisEntry &e : s.dir) used += e.out != 0;
			printf("varied filter=%u sides=", f);
			for (size_t i = 0; i < sides.size(); ++i) printf(i ? ",%u" : "%u", sides[i]);
			printf(" n_dir=%zu used=%u", s.dir.size(), used);
			arr("dir", s.dir);
			arr("starts", s.starts);
			arr("sizes", s.sizes);
			arr("coeffs", s.coeffs);
			printf("\n");
		}
	return 0;
}

// One up-scaling table as a line: what a kernel reads of it (window, precision, the outputs' starts and sizes, the weights)
namespace {
void expand_tab_line(const char *who, uint32_t f, uint32_t full, uint32_t stored, const pxz::ExpandTab &t, const std::vector<uint16_t> &starts,
                     const std::vector<uint16_t> &sizes, const std::vector<int16_t> &coeffs)
{
	const size_t nc = f == 0 ? 0 : (size_t)full * t.window;
	printf("%s filter=%u full=%u stored=%u window=%u precision=%u starts=%016llx sizes=%016llx coeffs=%016llx\n", who, f, full, stored, t.window,
	       t.precision, (unsigned long long)fnv(starts.data() + t.start_off, full * sizeof(uint16_t)),
	       (unsigned long long)fnv(sizes.data() + t.start_off, full * sizeof(uint16_t)),
	       (unsigned long long)fnv(coeffs.data() + t.coeff_off, nc * sizeof(int16_t)));
}
}  // namespace

// The (full size, stored size) directories of the varied expand, table by table ("vexpand" lines), and beside each the table
// build_expand_tables makes for a tile geometry whose full size is that side ("expand1" lines: axis 0, full class) -- the one
// expand_kernel reads.  tests/test_varied_decode_host.py compares the two and pins a digest of the first.
int dump_varied_expand()
{
	const std::vector<uint32_t> sides = {64, 32, 20, 17, 5, 1};
	for (uint32_t f = 0; f < 5; ++f) {
		pxz::VariedExpandTableSet v;
		if (!pxz::build_varied_expand_tables(sides, f, &v)) return 1;
		printf("vexpand-set filter=%u stride=%u max_window=%u", f, v.stride, v.max_window);
		arr("slot", v.slot);
		arr("dir", v.dir);
		arr("starts", v.starts);
		arr("sizes", v.sizes);
		arr("coeffs", v.coeffs);
		printf("\n");
		for (uint32_t full : sides) {
			pxz::ExpandTableSet s;
			if (!pxz::build_expand_tables(full, full, full, full, f, &s)) return 1;
			for (uint32_t stored = 1; stored < full; ++stored) {
				expand_tab_line("vexpand", f, full, stored, v.dir[(size_t)v.slot[full] * v.stride + stored], v.starts, v.sizes, v.coeffs);
				expand_tab_line("expand1", f, full, stored, s.dir[stored], s.starts, s.sizes, s.coeffs);
			}
		}
	}
	return 0;
}

// build_level_thresholds: one line per k, the threshold's bit pattern in hex (tests/test_tables_host.py holds them against the
// oracle's reduce_dims)
int dump_thresholds()
{
	float t[pxz::kNumThresholds];
	if (!pxz::build_level_thresholds(t, pxz::kNumThresholds)) return 1;
	for (int k = 0; k < pxz::kNumThresholds; ++k) {
		uint32_t bits;
		std::memcpy(&bits, &t[k], 4);
		printf("threshold k=%d bits=%08x\n", k, bits);
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 1 && std::strcmp(argv[1], "thresholds") == 0) return dump_thresholds();
	if (argc > 1 && std::strcmp(argv[1], "varied") == 0) return dump_varied();
	if (argc > 1 && std::strcmp(argv[1], "varied_expand") == 0) return dump_varied_expand();
	for (uint32_t f = 0; f < 5; ++f)
		for (const auto &g : grids(false)) {
			pxz::ShrinkTableSet s;
			if (!pxz::build_shrink_tables(g[0], g[1], g[2], g[3], f, &s)) return 1;
			uint32_t mf = 0;
			for (const pxz::AxisTab &t : s.tabs) mf += t.mf_off != 0;
			printf("shrink filter=%u tile=%ux%u edge=%ux%u tabs=%016llx", f, g[0], g[1], g[2], g[3],
			       (unsigned long long)fnv(s.tabs.data(), s.tabs.size() * sizeof(pxz::AxisTab)));
			arr("bounds", s.bounds);
			arr("coeffs", s.coeffs);
			arr("ksums", s.ksums);
			arr("rows", s.rows);
			arr("mf64", s.mf64);
			printf(" rows_dw=%zu mf_tabs=%u opaque=%u\n", s.rows.size(), mf, s.opaque_stays ? 1u : 0u);
		}
	for (uint32_t f = 0; f < 5; ++f)
		for (const auto &g : grids(true)) {
			pxz::ExpandTableSet s;
			if (!pxz::build_expand_tables(g[0], g[1], g[2], g[3], f, &s)) return 1;
			printf("expand filter=%u tile=%ux%u edge=%ux%u stride=%u", f, g[0], g[1], g[2], g[3], s.dir_stride);
			arr("dir", s.dir);
			arr("starts", s.starts);
			arr("sizes", s.sizes);
			arr("coeffs", s.coeffs);
			arr("xmf", s.xmf);
			arr("xmf16", s.xmf16);
			arr("xmf64", s.xmf64);
			printf("\n");
		}
	// (frame width, height, block width, height, minimum width, height), each with every pair of filters
	const uint32_t geo[][6] = {{1920, 1080, 128, 128, 4, 4}, {333, 217, 50, 50, 8, 8}, {640, 360, 96, 64, 4, 4}};
	for (uint32_t f = 0; f < 5; ++f)
		for (const auto &g : geo)
			for (uint32_t u = 0; u < 5; ++u) {
				// the levels of the recursion as pxz_tree_process_frames_device walks them
				const uint32_t mbw = g[4] > 4 ? g[4] : 4, mbh = g[5] > 4 ? g[5] : 4;
				std::vector<std::pair<uint32_t, uint32_t>> levels;
				for (uint32_t bw = g[2], bh = g[3]; bw > mbw && bh > mbh; bw >>= 1, bh >>= 1) levels.emplace_back(bw, bh);
				pxz::TreeTableSet s;
				if (!pxz::build_tree_tables(g[0], g[1], levels, f, u, &s)) return 1;
				printf("tree filter=%u up=%u frame=%ux%u block=%ux%u min=%ux%u n_dir=%zu", f, u, g[0], g[1], g[2], g[3], mbw, mbh,
				       s.dir.size());
				arr("dir", s.dir);
				arr("starts", s.starts);
				arr("sizes", s.sizes);
				arr("coeffs", s.coeffs);
				printf("\n");
			}
	return 0;
}
