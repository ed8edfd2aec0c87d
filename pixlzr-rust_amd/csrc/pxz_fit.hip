// pxz_fit.hip -- fit to a budget (pxz_fit_varied_ladder_device, pxz_gather_varied_rungs_device): after a varied ladder, the
// writer's offsets and the distortion call's sums are on the device for every rung of every image.  fit_select_kernel picks one
// rung per image from them (the rule is fit_pick's, pxz_fit.h, the text pxz_fit_select runs on the host), and
// gather_rungs_kernel copies the chosen rungs' tiles into the varied layout of the images themselves, where the unchanged writer
// makes files of them.
//
// gather_rungs_kernel: one wave per output tile of the flat tile space (four waves per block, grid-stride).  A wave
//   1. finds the tile's image by owner_of (pxz_device.h) and reads that image's choice, once, wave-uniform;
//   2. lane 0 copies the value's bits and both sizes (and, for the image's first tile, writes the image's flag);
//   3. the wave copies the tile's valid bytes, tw * th * C of them (never more than a slot), from input slot
//      choice * n_tiles + t to output slot t, both addressed with 64-bit offsets.  Nothing is staged: there is no LDS.
// Slots are not multiples of 16 bytes in general (5x3 RGB: 45; 37x61 RGB: 6771), so how a tile moves is decided per tile from
// the two addresses, and every access is naturally aligned:
//   source and destination congruent mod 16: bytes up to a dword, dwords up to a 16-byte line, 16-byte loads and stores for
//                                            the body, then dwords and bytes;
//   congruent mod 4 only:                    bytes, dwords, bytes;
//   otherwise:                               bytes.
// No byte behind the valid ones is written.  (gather_copy, pxz_fit.h.)
#include "pxz_device.h"
#include "pxz_fit.h"
#include "pxz_launch.h"

namespace pxz {

constexpr uint32_t kFitThreads = 256;
constexpr uint32_t kGatherThreads = 256;

__global__ void __launch_bounds__(kFitThreads) fit_select_kernel(const FitArgs a)
{
	const uint32_t i = blockIdx.x * kFitThreads + threadIdx.x;
	if (i >= a.n_images) return;
	const uint64_t n = a.n_images;
	const FitPick p = fit_pick(
		a.n_factors, a.criterion, a.targets[i],
		[&](uint32_t r) -> uint64_t { return a.file_offsets[r * n + i + 1u] - a.file_offsets[r * n + i]; },
		[&](uint32_t r) -> uint64_t {
			const unsigned long long *s = a.image_sse + (r * n + i) * a.channels;
			uint64_t sum = 0;
			for (uint32_t c = 0; c < a.channels; ++c) sum += s[c];
			return sum;
		});
	a.choice[i] = p.choice;
	a.flags[i] = p.flags;
}

// (the copy itself is gather_copy of pxz_fit.h: host code too, so that pxz_fit_check.cpp can run it for every alignment)

template <int C>
__global__ void __launch_bounds__(kGatherThreads) gather_rungs_kernel(const GatherArgs a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (kGatherThreads / 64u);
	const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kGatherThreads / 64u) + (threadIdx.x >> 6)));
	for (uint64_t t64 = first; t64 < a.n_tiles; t64 += waves) {
		const uint32_t t = (uint32_t)t64;
		const uint32_t owner = owner_of(a.images, a.n_images, t, &VariedImage::tile0);
		uint32_t rung = a.choice[owner];
		const bool beyond = rung >= a.n_factors;
		if (beyond) rung = a.n_factors - 1u;  // nothing is read out of bounds, whatever the choice says
		const uint64_t from = (uint64_t)rung * a.n_tiles + t;
		const uint32_t w = a.w[from], h = a.h[from];
		if (lane == 0u) {
			a.out_value[t] = a.value[from];
			a.out_w[t] = w;
			a.out_h[t] = h;
			if (a.image_flags != nullptr && t == a.images[owner].tile0) a.image_flags[owner] = beyond ? 2u : 0u;
		}
		if (a.out_slots == nullptr) continue;
		// the valid bytes; sizes that no tile of this block can have copy no more than the slot
		const uint64_t valid = (uint64_t)w * h * (uint32_t)C;
		const uint32_t bytes = valid < a.slot_bytes ? (uint32_t)valid : a.slot_bytes;
		gather_copy(a.out_slots + t64 * a.slot_bytes, a.slots + from * a.slot_bytes, bytes, lane);
	}
}

hipError_t launch_fit_select(const FitArgs &a, hipStream_t stream)
{
	if (a.n_images == 0u || a.n_factors == 0u) return hipSuccess;
	const uint32_t blocks = (uint32_t)(((uint64_t)a.n_images + kFitThreads - 1u) / kFitThreads);
	hipLaunchKernelGGL(fit_select_kernel, dim3(blocks), dim3(kFitThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_gather_rungs(const GatherArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.n_tiles == 0u || a.n_factors == 0u) return hipSuccess;
	// a block of four waves takes four tiles at a time and no LDS: eight blocks per CU, as tile_blocks gives for an eighth of it
	const uint32_t per_block = kGatherThreads / 64u;
	const uint32_t blocks = tile_blocks((uint32_t)(((uint64_t)a.n_tiles + per_block - 1u) / per_block), kLdsPerCu / 8u, n_cus);
	auto go = [&](auto kernel) {
		hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kGatherThreads), 0, stream, a);
		return hipGetLastError();
	};
	return channels == 4u ? go(gather_rungs_kernel<4>) : go(gather_rungs_kernel<3>);
}

}  // namespace pxz
