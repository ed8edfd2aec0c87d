// pxz_retile_ladder.hip -- stored tiles of a varied batch brought to another block size at several factors in one launch
// (pxz_retile_varied_ladder_frames_device): retile_kernel (pxz_retile.hip) up to the packed tile image, the two ladders'
// detectors up to their raw results, then varied_ladder_kernel (pxz_varied_ladder.hip) from the rungs' decisions on.  Neither
// the assembly of a destination tile nor the detector's raw result depends on the factor, so a destination tile is assembled
// once and measured once; each rung only decides its levels, and the tile is resampled once per distinct pair of levels among
// its rungs.  K calls of the one-factor re-tile assemble and measure every tile K times.
//
// retile_ladder_kernel: one DESTINATION tile per block of 256 threads, grid-stride over the flat tile space of the destination
// layout (pxz_varied_layout at the new block), owners by owner_of (pxz_device.h), the grid of tile_blocks (pxz_launch.h).  Image
// i is entry i of both per-image tables, the destination layout's (v.images) and the source layout's (src_images).  A tile
//   1. finds      its rectangle and the source tiles that cover it;
//   2. is assembled in X, one dword per pixel: a covering tile stored at full size is cloned in, any other is expanded over only
//                 the stored pixels the part's windows read.  A covering tile whose stored size cannot be (zero, or beyond its
//                 place in the SOURCE grid) sets status bit 0 and the image's flag; EVERY rung of the destination tile then gets
//                 0 x 0 and value bits 0, and every rung's slot is left as it was;
//   3. is packed to C bytes per pixel in place.
//                 Steps 1 to 3 are retile_assemble (pxz_varied_tile.h): the text of retile_kernel's steps 1 to 3, which that
//                 kernel keeps inline.  A fix to either belongs in the other;
//   4. is measured once: x = total / count, or the two integer sums (varied_oklab_raw, varied_sobel_sums);
//   5. is decided per rung, by thread r for rung r, cloned, premultiplied once and resampled once per distinct pair of levels:
//                 varied_ladder_tail (pxz_varied_tile.h), CALLED, not copied.  reshrink_ladder_kernel keeps a copy because the
//                 call measured 2-3.5 % slower there; here a build with the copy ran beside this one over the 48 rows
//                 of the bench: copy / call time 0.98-1.02, median 1.00, ahead on some rows and behind on others (DESIGN.md
//                 8p), so the one text is used.
// Source and destination layouts differ, so there is no in-place form.
//
// LDS of one block: retile_ladder_lds (pxz_varied_tile.h), where the layout and its limit are described; the kernel, this
// launch and the host take it from there.  [oklab tables] [X] [U]: U is retile_kernel's staging while the tile is assembled and
// the ladder's A afterwards -- the detector's planes, then I at its start and F behind I.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(kVariedThreads) retile_ladder_kernel(const RetileLadderArgs la)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	__shared__ uint32_t s_key[kVariedLadderMaxRungs];  // per rung: mx | my << 8 of the axes that shrink (0: a clone)
	const VariedArgs &a = la.r.v;
	const TileResizeArgs &x = la.r.x;
	const uint32_t tid = threadIdx.x, n_rungs = la.n_factors;
	const bool oklab = a.mode == 0u;
	const RetileLadderLds L = retile_ladder_lds(a.mode, x.bw, x.bh, a.bw, a.bh, (uint32_t)C, x.wdw);
	uint8_t *const s_base = reinterpret_cast<uint8_t *>(lds);
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint32_t *s_img = reinterpret_cast<uint32_t *>(s_base + L.x);
	uint32_t *s_src = reinterpret_cast<uint32_t *>(s_base + L.u), *s_tmp = reinterpret_cast<uint32_t *>(s_base + L.inter);
	uint32_t *s_wx = reinterpret_cast<uint32_t *>(s_base + L.wx), *s_wy = s_wx + x.wdw * x.bw;
	uint8_t *s_x = s_base + L.x;                      // the packed tile image
	uint8_t *s_a = s_base + L.u;                      // A: I, or a vertical-only result
	uint8_t *s_f = s_a + L.f;                         // F
	float *s_plane = reinterpret_cast<float *>(s_a);  // [4][kVariedChunk] (the detector, before A holds a pass)
	if (oklab) {
		oklab_fill_tables(s_lms, s_alpha, s_scale, tid);
		__syncthreads();
	}

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		// the tile's owner and its rectangle
		const uint32_t owner = owner_of(a.images, a.n_images, tile_g, &VariedImage::tile0);
		const VariedImage im = a.images[owner];
		const VariedImage sm = la.r.src_images[owner];
		const uint32_t t = tile_g - im.tile0;
		const uint32_t ty = t / im.cols, tx = t - ty * im.cols;
		const uint32_t w = tx + 1u == im.cols ? im.edge_w : a.bw;  // split.rs:18
		const uint32_t h = ty + 1u == im.rows ? im.edge_h : a.bh;  // split.rs:19

		// ---- 1. to 3. the tile image X, tightly packed (ends in a barrier)
		if (retile_assemble<C>(x, sm, tx * a.bw, ty * a.bh, w, h, s_img, s_src, s_tmp, s_wx, s_wy, tid)) {
			// a stored size that cannot be: flagged, empty at every rung, every slot left alone
			if (tid == 0u) {
				atomicOr(x.status, 1u);
				if (la.r.image_flags) la.r.image_flags[owner] = 1u;
			}
			if (tid < n_rungs) {
				const size_t at = (size_t)tid * a.n_tiles + tile_g;
				a.value[at] = 0.0f;
				a.out_w[at] = 0u;
				a.out_h[at] = 0u;
			}
			continue;
		}

		// ---- 4. the detector up to what the factor has not entered, once
		float xr = 0.0f;
		uint32_t shz = 0, svr = 0;
		if (oklab) xr = varied_oklab_raw<C>(s_x, w * h, s_lms, s_alpha, s_scale, s_plane, s_acc, tid);
		else varied_sobel_sums<C>(s_x, w, h, s_red, tid, shz, svr);

		// ---- 5. the rungs: decisions, clones, one premultiply, one resample per distinct pair of levels, stores
		varied_ladder_tail<C>(a, la.factors, n_rungs, tile_g, w, h, xr, shz, svr, s_key, s_x, s_a, s_f, tid);
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_retile_ladder(const RetileLadderArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.r.v.n_tiles == 0u || a.n_factors == 0u) return hipSuccess;
	const uint32_t lds = retile_ladder_lds(a.r.v.mode, a.r.x.bw, a.r.x.bh, a.r.v.bw, a.r.v.bh, channels, a.r.x.wdw).total;
	if (lds > kLdsPerCu) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.r.v.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(retile_ladder_kernel<4>) : go(retile_ladder_kernel<3>);
}

uint32_t retile_ladder_lds_bytes(uint32_t mode, uint32_t sbw, uint32_t sbh, uint32_t dbw, uint32_t dbh, uint32_t channels, uint32_t wdw)
{
	return retile_ladder_lds(mode, sbw, sbh, dbw, dbh, channels, wdw).total;
}

}  // namespace pxz
