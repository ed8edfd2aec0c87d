// pxz_retile_distortion.hip -- what a re-tiled tile lost against the archive it came from
// (pxz_retile_distortion_varied_device): per tile of the DESTINATION layout, set and channel the sum over the tile's w x h pixels of
//   (decoded(archive)[pixel] - expand(set's stored tile, filter_up)[pixel])^2,
// decoded(archive) being what varied_expand_kernel writes from the archive's tiles -- tiles of ANOTHER layout of the same images,
// expanded with expand_filter.  A destination tile of that image is put together from the parts of the source tiles that cover it,
// as the re-tile does it, so the error of rung r of a re-tile ladder against "what the files decode to now" needs
// two tile-sized images in LDS and nothing of image size anywhere.  The reference has no such function.
//
// retile_distortion_kernel: one DESTINATION tile per block of 256 threads, grid-stride over the flat tile space of the destination
// layout, owners by owner_of (pxz_device.h), the grid of tile_blocks (pxz_launch.h) -- the tile loop of retile_ladder_kernel.  Image
// i is entry i of both per-image tables, the destination layout's (a.images) and the source layout's (a.src_images).  A tile
//   1. finds      its rectangle and checks the stored sizes of the source tiles that cover it, before anything is staged: one that
//                 cannot be (zero, or beyond its place in the SOURCE grid) sets status bit 0 and the image's flag, every set's entry
//                 becomes all-ones, no total has the tile and nothing of it is read;
//   2. per set    a stored size that cannot be: that entry all-ones, status bit 0, the flag, not in the totals;
//                 stored at full size: zeros, the slot is not read (block.rs:279-281: it IS the reference);
//   3. otherwise  the reference R, once per tile and only when a set needs it: retile_assemble (pxz_varied_tile.h) over the source
//                 layout with expand_filter's tables;
//   4.            the set's tile E at its full size: retile_assemble again, with the source block equal to the destination block --
//                 exactly one covering tile, the whole of it wanted -- filter_up's tables, and the destination layout's entry with
//                 tile0 shifted to the set.  Both are CALLS of the one text; nothing of the expand arithmetic is written here;
//   5.            the squared byte differences of the two packed planes, in u32 (below), a wave reduction, and one lane per channel
//                 that stores the tile's sums and adds them to the image's with a 64-bit integer atomic.
// Everything is integer, so the result does not depend on the order in which blocks arrive.
//
// LDS of one block: retile_distortion_lds (pxz_varied_tile.h), where the layout and its limit are described; the kernel, this launch
// and the host take it from there.  [R] [E] [S]: S is retile_assemble's staging, for the source side while R is assembled and for
// the set side while E is, each at its own offsets and window stride.
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(kVariedThreads) retile_distortion_kernel(const RetileDistortionArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ uint32_t s_red[4u * (kVariedThreads / 64u)];  // per wave: the channels' sums
	const uint32_t tid = threadIdx.x;
	const RetileDistortionLds L = retile_distortion_lds(a.r.bw, a.r.bh, a.u.bw, a.u.bh, a.r.wdw, a.u.wdw);
	uint8_t *const s_base = reinterpret_cast<uint8_t *>(lds);
	uint32_t *s_ref = reinterpret_cast<uint32_t *>(s_base + L.r), *s_exp = reinterpret_cast<uint32_t *>(s_base + L.e);
	uint32_t *s_stage = reinterpret_cast<uint32_t *>(s_base + L.s);
	uint32_t *s_rtmp = reinterpret_cast<uint32_t *>(s_base + L.src_inter), *s_utmp = reinterpret_cast<uint32_t *>(s_base + L.set_inter);
	uint32_t *s_rwx = reinterpret_cast<uint32_t *>(s_base + L.src_wx), *s_rwy = s_rwx + a.r.wdw * a.r.bw;
	uint32_t *s_uwx = reinterpret_cast<uint32_t *>(s_base + L.set_wx), *s_uwy = s_uwx + a.u.wdw * a.u.bw;

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		// ---- 1. the tile's owner, its rectangle, and the stored sizes of the source tiles that cover it
		const uint32_t owner = owner_of(a.images, a.n_images, tile_g, &VariedImage::tile0);
		const VariedImage im = a.images[owner];
		const VariedImage sm = a.src_images[owner];
		const uint32_t t = tile_g - im.tile0;
		const uint32_t ty = t / im.cols, tx = t - ty * im.cols;
		const uint32_t w = tx + 1u == im.cols ? im.edge_w : a.u.bw;  // split.rs:18
		const uint32_t h = ty + 1u == im.rows ? im.edge_h : a.u.bh;  // split.rs:19
		const uint32_t n = w * h;
		const uint32_t X0 = tx * a.u.bw, Y0 = ty * a.u.bh;
		const uint32_t sc0 = X0 / a.r.bw, sr0 = Y0 / a.r.bh, sc1 = (X0 + w - 1u) / a.r.bw, sr1 = (Y0 + h - 1u) / a.r.bh;
		bool bad = false;
		for (uint32_t sty = sr0; sty <= sr1; ++sty)
			for (uint32_t stx = sc0; stx <= sc1; ++stx) {
				const uint32_t fw = stx + 1u == sm.cols ? sm.edge_w : a.r.bw, fh = sty + 1u == sm.rows ? sm.edge_h : a.r.bh;
				const uint32_t st = sm.tile0 + sty * sm.cols + stx;
				const uint32_t rw = a.r.tile_w[st], rh = a.r.tile_h[st];
				bad = bad || rw == 0u || rh == 0u || rw > fw || rh > fh;  // (bad_stored_size, pxz_device.h)
			}
		if (bad) {
			// a reference that cannot be: every set's entry is all-ones, no total has the tile
			if (tid == 0u) {
				atomicOr(a.r.status, 1u);
				if (a.image_flags) a.image_flags[owner] = 1u;
			}
			if (a.tile_sse)
				for (uint32_t e = tid; e < a.n_sets * (uint32_t)C; e += kVariedThreads)
					a.tile_sse[((size_t)(e / (uint32_t)C) * a.n_tiles + tile_g) * (uint32_t)C + e % (uint32_t)C] = ~0ull;
			continue;
		}
		bool have_ref = false;  // R holds the reference, once a set has needed it

		for (uint32_t s = 0; s < a.n_sets; ++s) {
			// ---- 2. the set's stored size (the same in every thread)
			const size_t idx = (size_t)s * a.n_tiles + tile_g;
			const uint32_t tw = a.u.tile_w[idx], th = a.u.tile_h[idx];
			if (tw == 0u || th == 0u || tw > w || th > h) {
				if (tid == 0u) {
					atomicOr(a.r.status, 1u);
					if (a.image_flags) a.image_flags[owner] = 1u;
				}
				if (a.tile_sse && tid < (uint32_t)C) a.tile_sse[idx * (uint32_t)C + tid] = ~0ull;
				continue;
			}
			if (tw == w && th == h) {  // block.rs:279-281: the stored tile is the reference
				if (a.tile_sse && tid < (uint32_t)C) a.tile_sse[idx * (uint32_t)C + tid] = 0ull;
				continue;
			}

			// ---- 3. the reference, once: the tile of what the archive decodes to, from the source tiles that cover it
			if (!have_ref) {
				retile_assemble<C>(a.r, sm, X0, Y0, w, h, s_ref, s_stage, s_rtmp, s_rwx, s_rwy, tid);  // (no bad size: step 1)
				have_ref = true;
			}

			// ---- 4. the set's stored tile at its full size: one covering tile of the destination layout's own grid, set s of it
			VariedImage um = im;
			um.tile0 = s * a.n_tiles + im.tile0;  // (n_sets * n_tiles fits 32 bits: the host's check)
			retile_assemble<C>(a.u, um, X0, Y0, w, h, s_exp, s_stage, s_utmp, s_uwx, s_uwy, tid);

			// ---- 5. the squared error over both packed planes.  u32 holds: a plane has at most 65536 bytes, so a tile has at most
			// 16384 pixels (21845 of RGB never fit: the plane is laid out a dword per pixel), a thread sees at most 64 of them, and
			// the whole tile 16384 * 255^2 < 1.07e9 < 2^32, so neither the wave's nor the block's sum wraps.
			uint32_t acc[4] = {0u, 0u, 0u, 0u};
			if constexpr (C == 4) {
				for (uint32_t i = tid; i < n; i += kVariedThreads) {
					const uint32_t px = s_ref[i], ex = s_exp[i];
#pragma unroll
					for (uint32_t c = 0; c < 4u; ++c) {
						const int32_t d = (int32_t)((px >> (8u * c)) & 255u) - (int32_t)((ex >> (8u * c)) & 255u);
						acc[c] += (uint32_t)(d * d);
					}
				}
			} else {
				// RGB: four pixels are three dwords; byte k of dword j of a group is channel (4 j + k) mod 3.  The tail by bytes
				const uint32_t n4 = n >> 2;
				for (uint32_t q = tid; q < n4; q += kVariedThreads) {
#pragma unroll
					for (uint32_t j = 0; j < 3u; ++j) {
						const uint32_t px = s_ref[3u * q + j], ex = s_exp[3u * q + j];
#pragma unroll
						for (uint32_t k = 0; k < 4u; ++k) {
							const int32_t d = (int32_t)((px >> (8u * k)) & 255u) - (int32_t)((ex >> (8u * k)) & 255u);
							acc[(4u * j + k) % 3u] += (uint32_t)(d * d);
						}
					}
				}
				const uint8_t *rb = reinterpret_cast<const uint8_t *>(s_ref), *eb = reinterpret_cast<const uint8_t *>(s_exp);
				for (uint32_t i = 4u * n4 + tid; i < n; i += kVariedThreads) {
#pragma unroll
					for (uint32_t c = 0; c < 3u; ++c) {
						const int32_t d = (int32_t)rb[3u * i + c] - (int32_t)eb[3u * i + c];
						acc[c] += (uint32_t)(d * d);
					}
				}
			}
#pragma unroll
			for (uint32_t c = 0; c < (uint32_t)C; ++c) {
				for (int d = 32; d >= 1; d >>= 1) acc[c] += (uint32_t)__shfl_xor((int)acc[c], d, 64);
				if ((tid & 63u) == 0u) s_red[4u * (tid >> 6) + c] = acc[c];
			}
			__syncthreads();  // the waves' sums; and every thread has read R and E
			if (tid < (uint32_t)C) {
				uint32_t sum = 0;
#pragma unroll
				for (uint32_t q = 0; q < kVariedThreads / 64u; ++q) sum += s_red[4u * q + tid];
				if (a.tile_sse) a.tile_sse[idx * (uint32_t)C + tid] = sum;
				if (sum) atomicAdd(a.image_sse + ((size_t)s * a.n_images + owner) * (uint32_t)C + tid, (unsigned long long)sum);
			}
			// (s_red is written again only behind the barriers of the next retile_assemble)
		}
	}
}

hipError_t launch_retile_distortion(const RetileDistortionArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.n_tiles == 0u || a.n_sets == 0u) return hipSuccess;
	const uint32_t lds = retile_distortion_lds(a.r.bw, a.r.bh, a.u.bw, a.u.bh, a.r.wdw, a.u.wdw).total;
	if (lds > kLdsPerCu) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(retile_distortion_kernel<4>) : go(retile_distortion_kernel<3>);
}

uint32_t retile_distortion_lds_bytes(uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t wdw_src, uint32_t wdw_set)
{
	return retile_distortion_lds(sbw, sbh, dbw, dbh, wdw_src, wdw_set).total;
}

}  // namespace pxz
