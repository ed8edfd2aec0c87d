// pxz_tilefit.hip -- fit to a budget per tile (pxz_record_bytes_varied_device, pxz_fit_varied_tiles_device,
// pxz_gather_varied_tile_rungs_device): after a varied ladder every rung of every tile is on the device, with its record's
// length (record_bytes_kernel reads the writer's own) and its squared error (the distortion calls' d_tile_sse).  The kernels
// here pick one rung per tile under a budget per group of images -- the rule is pxz_tilefit.h's, the text pxz_fit_tiles_select
// runs on the host -- and gather_tile_rungs_kernel copies the chosen tiles into the varied layout of the images themselves.
//
// The select is a fixed chain of launches over the flat tile space, one thread per tile, whatever the images, groups and rungs:
//   tilefit_init_kernel     the tile's group (a search in the groups' first tiles, once), its candidates packed into one u64
//                           each (tilefit_pack: the steps below read 8 bytes a candidate, not 4 + 8 channels), and the group's
//                           interval [0, 2^32]
//   tilefit_step_kernel     kTileFitSteps times: step k advances the group's interval by the total step k-1 left (every thread
//                           of the group derives the same interval; the thread of the group's first tile stores it for step
//                           k+1, in the one of two buffers that step k does not read), picks the tile's rung at the interval's
//                           middle and adds its bytes (PXZ_FIT_BYTES) or its error (PXZ_FIT_SSE) to the group's total of step k
//   tilefit_totals_kernel   the last advance gives lambda*; the tile's pick at lambda* is its choice, and its bytes and error go
//                           to the group's totals, with the uniform totals of every rung
//   tilefit_decide_kernel   one thread per group: tilefit_decide -> the group's outputs
//   tilefit_apply_kernel    the tiles of a group that took one rung for all take it
// The kernel boundary is the only synchronisation: nothing is read back, no block waits for another.  Sums: a segmented
// reduction over the wave first (the tiles of a group are neighbours, so a wave holds a few runs of equal groups; seg_sum),
// then one integer atomic add per run -- or, where all 256 tiles of a block belong to one group, one per block (group_add): a
// folder in one group is spread over all its blocks, which then meet at one address a quarter as often.  Integer sums do not
// depend on the order of arrival.
#include "pxz_device.h"
#include "pxz_launch.h"
#include "pxz_tilefit.h"

namespace pxz {

constexpr uint32_t kTileFitThreads = 256;
constexpr uint32_t kTileGatherThreads = 256;
constexpr uint32_t kNoGroup = 0xffffffffu;

// The runs of equal groups in a wave: same[i] -- lane + 2^i holds the same group; head -- the first lane of its run.
// Every lane of the wave calls these (lanes without a tile: kNoGroup, 0).
struct SegRuns {
	bool same[6], head;
};
__device__ __forceinline__ SegRuns seg_runs(uint32_t g, uint32_t lane)
{
	SegRuns s;
#pragma unroll
	for (uint32_t i = 0; i < 6u; ++i) {
		const uint32_t d = 1u << i, other = (uint32_t)__shfl_down((int)g, d, 64);
		s.same[i] = lane + d < 64u && other == g;
	}
	const uint32_t before = (uint32_t)__shfl_up((int)g, 1u, 64);
	s.head = lane == 0u || before != g;
	return s;
}
// the sum over the run's lanes from this one on: the run's total on its head
__device__ __forceinline__ unsigned long long seg_sum(unsigned long long v, const SegRuns &s)
{
#pragma unroll
	for (uint32_t i = 0; i < 6u; ++i) {
		const unsigned long long other = __shfl_down(v, 1u << i, 64);
		if (s.same[i]) v += other;
	}
	return v;
}

// Is the whole block one group?  Every thread of the block calls this once (lanes without a tile: kNoGroup, so the last block of
// the grid is not).
__device__ __forceinline__ bool block_is_one_group(uint32_t g)
{
	__shared__ uint32_t s_g;
	if (threadIdx.x == 0u) s_g = g;
	__syncthreads();
	return __syncthreads_and(g == s_g && g != kNoGroup) != 0;
}

// N sums at once to dst[k][g]: v[k] of every tile of the block added to its group's entry.  Every thread of the block calls this
// (one_group: block_is_one_group's answer; lanes without a tile pass zeros).  Zeros are not added: most totals of most steps
// are touched by few blocks.
template <int N>
__device__ __forceinline__ void group_add(unsigned long long (&v)[N], uint32_t g, const SegRuns &runs, bool one_group, unsigned long long *const (&dst)[N])
{
	__shared__ unsigned long long s_part[N][kTileFitThreads / 64u];
#pragma unroll
	for (int k = 0; k < N; ++k) v[k] = seg_sum(v[k], runs);
	if (!one_group) {
		if (runs.head && g != kNoGroup)
#pragma unroll
			for (int k = 0; k < N; ++k)
				if (v[k] != 0ull) atomicAdd(dst[k], v[k]);
		return;
	}
	if ((threadIdx.x & 63u) == 0u)  // (the wave is one run: its total is on lane 0)
#pragma unroll
		for (int k = 0; k < N; ++k) s_part[k][threadIdx.x >> 6] = v[k];
	__syncthreads();
	if (threadIdx.x < (uint32_t)N) {
		unsigned long long sum = 0;
		for (uint32_t w = 0; w < kTileFitThreads / 64u; ++w) sum += s_part[threadIdx.x][w];
		if (sum != 0ull) atomicAdd(dst[threadIdx.x], sum);
	}
	__syncthreads();  // (the next call writes s_part again)
}

__global__ void __launch_bounds__(kTileFitThreads) tilefit_init_kernel(const TileFitArgs a)
{
	const uint64_t t = (uint64_t)blockIdx.x * kTileFitThreads + threadIdx.x;
	if (t >= a.n_tiles) return;
	uint32_t lo = 0, hi = a.n_groups - 1u;  // the last group whose first tile is <= t
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (a.group_tile0[mid] <= (uint32_t)t) lo = mid;
		else hi = mid - 1u;
	}
	a.tile_group[t] = lo;
	if (a.group_tile0[lo] == (uint32_t)t) {
		a.interval[2u * lo] = 0ull;
		a.interval[2u * lo + 1u] = kTileFitLambdaMax;
	}
	for (uint32_t r = 0; r < a.n_factors; ++r) {
		const uint64_t k = (uint64_t)r * a.n_tiles + t;
		uint64_t sse[4];
		for (uint32_t c = 0; c < a.channels; ++c) sse[c] = a.tile_sse[k * a.channels + c];
		a.cand[k] = tilefit_pack(a.record_bytes[k], sse, a.channels);
	}
}

// the group's interval at step `step`: what step - 1 used, advanced by the total it left (step 0: as tilefit_init_kernel set it)
__device__ __forceinline__ void tilefit_interval(const TileFitArgs &a, uint32_t step, uint32_t g, uint64_t *lo, uint64_t *hi)
{
	const unsigned long long *in = a.interval + (size_t)((step + 1u) & 1u) * 2u * a.n_groups;
	if (step == 0u) in = a.interval;
	*lo = in[2u * g];
	*hi = in[2u * g + 1u];
	if (step == 0u) return;
	uint64_t total = a.acc[(size_t)(step - 1u) * a.n_groups + g];
	if (a.criterion == kFitBytes) total += a.fixed[g];
	tilefit_advance(a.criterion, a.targets[g], total, lo, hi);
}

__global__ void __launch_bounds__(kTileFitThreads) tilefit_step_kernel(const TileFitArgs a)
{
	const uint64_t t = (uint64_t)blockIdx.x * kTileFitThreads + threadIdx.x;
	const bool live = t < a.n_tiles;
	const uint32_t g = live ? a.tile_group[t] : kNoGroup;
	unsigned long long v = 0;
	if (live) {
		uint64_t lo, hi;
		tilefit_interval(a, a.step, g, &lo, &hi);
		if (a.step != 0u && a.group_tile0[g] == (uint32_t)t) {
			unsigned long long *out = a.interval + (size_t)(a.step & 1u) * 2u * a.n_groups;
			out[2u * g] = lo;
			out[2u * g + 1u] = hi;
		}
		const TilePick p = tilefit_pick(a.n_factors, tilefit_mid(a.criterion, lo, hi), [&](uint32_t r) { return a.cand[(uint64_t)r * a.n_tiles + t]; });
		v = a.criterion == kFitBytes ? p.b : p.s;
	}
	const SegRuns runs = seg_runs(g, threadIdx.x & 63u);
	const bool one_group = block_is_one_group(g);
	unsigned long long sums[1] = {v};
	unsigned long long *const dst[1] = {a.acc + (size_t)a.step * a.n_groups + (live ? g : 0u)};
	group_add(sums, g, runs, one_group, dst);
}

__global__ void __launch_bounds__(kTileFitThreads) tilefit_totals_kernel(const TileFitArgs a)
{
	const uint64_t t = (uint64_t)blockIdx.x * kTileFitThreads + threadIdx.x;
	const bool live = t < a.n_tiles;
	const uint32_t g = live ? a.tile_group[t] : kNoGroup;
	unsigned long long b = 0, s = 0;
	if (live) {
		uint64_t lo, hi;
		tilefit_interval(a, kTileFitSteps, g, &lo, &hi);  // (33 halvings: lo == hi)
		if (a.group_tile0[g] == (uint32_t)t) a.group_lambda[g] = lo;
		const TilePick p = tilefit_pick(a.n_factors, lo, [&](uint32_t r) { return a.cand[(uint64_t)r * a.n_tiles + t]; });
		a.tile_choice[t] = p.r;
		b = p.b;
		s = p.s;
		if (!p.any) atomicOr(a.group_bits + g, kTileFitNoCandidate);
	}
	const SegRuns runs = seg_runs(g, threadIdx.x & 63u);
	const bool one_group = block_is_one_group(g);
	const size_t gi = live ? g : 0u;
	{
		unsigned long long sums[2] = {b, s};
		unsigned long long *const dst[2] = {a.tot + 2u * gi, a.tot + 2u * gi + 1u};
		group_add(sums, g, runs, one_group, dst);
	}
	// the uniform totals: per rung the bytes and the error of the tiles that have it, and how many have not
	for (uint32_t r = 0; r < a.n_factors; ++r) {
		const unsigned long long cand = live ? a.cand[(uint64_t)r * a.n_tiles + t] : 0ull;
		const bool bad = cand == kTileFitUnusable;
		unsigned long long *u = a.uni + (gi * a.n_factors + r) * 3u;
		unsigned long long sums[3] = {bad ? 0ull : tilefit_b(cand), bad ? 0ull : tilefit_s(cand), bad ? 1ull : 0ull};
		unsigned long long *const dst[3] = {u, u + 1, u + 2};
		group_add(sums, g, runs, one_group, dst);
	}
}

__global__ void __launch_bounds__(kTileFitThreads) tilefit_decide_kernel(const TileFitArgs a)
{
	const uint32_t g = blockIdx.x * kTileFitThreads + threadIdx.x;
	if (g >= a.n_groups) return;
	const uint64_t fixed = a.fixed[g];
	const unsigned long long *u = a.uni + (size_t)g * a.n_factors * 3u;
	const TileFitDecision d = tilefit_decide(
		a.n_factors, a.criterion, a.targets[g], fixed + a.tot[2u * (size_t)g], a.tot[2u * (size_t)g + 1u],
		(a.group_bits[g] & kTileFitNoCandidate) != 0u, [&](uint32_t r) -> uint64_t { return fixed + u[3u * r]; },
		[&](uint32_t r) -> uint64_t { return u[3u * r + 1u]; }, [&](uint32_t r) -> bool { return u[3u * r + 2u] != 0ull; });
	a.group_bytes[g] = d.bytes;
	a.group_sse[g] = d.sse;
	a.group_flags[g] = d.flags;
	a.uni_rung[g] = (d.flags & kTileFitUniform) ? d.uniform : 0xffffffffu;
}

__global__ void __launch_bounds__(kTileFitThreads) tilefit_apply_kernel(const TileFitArgs a)
{
	const uint64_t t = (uint64_t)blockIdx.x * kTileFitThreads + threadIdx.x;
	if (t >= a.n_tiles) return;
	const uint32_t rung = a.uni_rung[a.tile_group[t]];
	if (rung != 0xffffffffu) a.tile_choice[t] = rung;
}

// The writer's record lengths as the caller's: one thread per tile.  varied_reclen_kernel (pxz_varied.hip) has added the next
// image's header onto the last record of every image but the last, for the writer's scan: that comes off again.
__global__ void __launch_bounds__(256) record_bytes_kernel(const RecordBytesArgs a)
{
	const uint64_t t64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (t64 >= a.n_tiles) return;
	const uint32_t t = (uint32_t)t64;
	uint32_t len = a.rec_len[t];
	const uint32_t owner = owner_of(a.images, a.n_images, t, &VariedImage::tile0);
	const VariedImage im = a.images[owner];
	if (owner + 1u < a.n_images && t == im.tile0 + im.cols * im.rows - 1u) len -= a.images[owner + 1u].hdr_bytes;
	a.record_bytes[t] = len;
}

// gather_rungs_kernel (pxz_fit.hip) with a choice per tile: one wave per output tile, four waves per block, grid-stride, no LDS.
// The tile's image is looked for only where its flag has to be set -- a choice beyond the ladder -- never on the copy path.
template <int C>
__global__ void __launch_bounds__(kTileGatherThreads) gather_tile_rungs_kernel(const GatherArgs a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (kTileGatherThreads / 64u);
	const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kTileGatherThreads / 64u) + (threadIdx.x >> 6)));
	for (uint64_t t64 = first; t64 < a.n_tiles; t64 += waves) {
		const uint32_t t = (uint32_t)t64;
		uint32_t rung = a.choice[t];
		const bool beyond = rung >= a.n_factors;
		if (beyond) rung = a.n_factors - 1u;  // nothing is read out of bounds, whatever the choice says
		const uint64_t from = (uint64_t)rung * a.n_tiles + t;
		const uint32_t w = a.w[from], h = a.h[from];
		if (lane == 0u) {
			a.out_value[t] = a.value[from];
			a.out_w[t] = w;
			a.out_h[t] = h;
			if (beyond && a.image_flags != nullptr) atomicOr(a.image_flags + owner_of(a.images, a.n_images, t, &VariedImage::tile0), 2u);
		}
		if (a.out_slots == nullptr) continue;
		// the valid bytes; sizes that no tile of this block can have copy no more than the slot
		const uint64_t valid = (uint64_t)w * h * (uint32_t)C;
		const uint32_t bytes = valid < a.slot_bytes ? (uint32_t)valid : a.slot_bytes;
		gather_copy(a.out_slots + t64 * a.slot_bytes, a.slots + from * a.slot_bytes, bytes, lane);
	}
}

// the chain of the select: 3 + kTileFitSteps + 1 launches, whatever the sizes
hipError_t launch_tilefit(const TileFitArgs &args, hipStream_t stream)
{
	if (args.n_tiles == 0u || args.n_groups == 0u || args.n_factors == 0u) return hipSuccess;
	TileFitArgs a = args;
	const uint32_t tile_blocks_n = (uint32_t)(((uint64_t)a.n_tiles + kTileFitThreads - 1u) / kTileFitThreads);
	const uint32_t group_blocks = (uint32_t)(((uint64_t)a.n_groups + kTileFitThreads - 1u) / kTileFitThreads);
	hipLaunchKernelGGL(tilefit_init_kernel, dim3(tile_blocks_n), dim3(kTileFitThreads), 0, stream, a);
	for (a.step = 0; a.step < kTileFitSteps; ++a.step) hipLaunchKernelGGL(tilefit_step_kernel, dim3(tile_blocks_n), dim3(kTileFitThreads), 0, stream, a);
	hipLaunchKernelGGL(tilefit_totals_kernel, dim3(tile_blocks_n), dim3(kTileFitThreads), 0, stream, a);
	hipLaunchKernelGGL(tilefit_decide_kernel, dim3(group_blocks), dim3(kTileFitThreads), 0, stream, a);
	hipLaunchKernelGGL(tilefit_apply_kernel, dim3(tile_blocks_n), dim3(kTileFitThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_record_bytes(const RecordBytesArgs &a, hipStream_t stream)
{
	if (a.n_tiles == 0u) return hipSuccess;
	hipLaunchKernelGGL(record_bytes_kernel, dim3((uint32_t)(((uint64_t)a.n_tiles + 255u) / 256u)), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_gather_tile_rungs(const GatherArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.n_tiles == 0u || a.n_factors == 0u) return hipSuccess;
	// as launch_gather_rungs: four tiles at a time per block, no LDS, eight blocks per CU
	const uint32_t per_block = kTileGatherThreads / 64u;
	const uint32_t blocks = tile_blocks((uint32_t)(((uint64_t)a.n_tiles + per_block - 1u) / per_block), kLdsPerCu / 8u, n_cus);
	auto go = [&](auto kernel) {
		hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kTileGatherThreads), 0, stream, a);
		return hipGetLastError();
	};
	return channels == 4u ? go(gather_tile_rungs_kernel<4>) : go(gather_tile_rungs_kernel<3>);
}

}  // namespace pxz
