// pxz_patch.hip -- pixel windows written INTO .pixlzr files: patch_kernel, tiles to tiles (pxz_patch_windows_device), and behind it
// the splice, old files and new tiles to new files (pxz_splice_windows_device; described where it stands).  The reference
// operation: open a file (decode_block gives every stored block block_value: Some(..), src/encoding/mod.rs:236-241), replace the
// blocks a window covers by fresh full-size blocks -- the stored block resized to its place (PixlzrBlock::resize, as expand does)
// with the new pixels written over it -- and shrink: Pixlzr::shrink_by returns blocks that carry a value as they are and shrinks
// only the fresh ones (src/data_types/pixlzr.rs:166-170).  So exactly the covered tiles are measured and resampled again, and this
// kernel sees no other tile.  The tile space is pxz_window_layout's: window k owns tiles [tile0, tile0 + ccols * crows), the tiles
// of its covered grid in row-major order -- which is pxz_varied_layout of one image of the size of the window's hull (the covered
// tiles' rectangle, clipped to the image), so every call that takes a varied batch takes the outputs with one hull per window.
//
// patch_kernel: one tile per block of 256 threads, grid-stride over the flat tile space, owners by owner_of over the windows'
// table (pxz_device.h), the grid of tile_blocks (pxz_launch.h).  A tile
//   1. finds     its window, its place in the image's grid, its full size (w, h) and the part [cx0, cx1) x [cy0, cy1) of it that
//                lies inside the window's rectangle (window_expand_kernel step 1, pxz_window.hip);
//   2. is flagged and emptied when its stored size cannot be (zero, or beyond its place), as reshrink_kernel does it: status bit 0,
//                the WINDOW's flag, outputs 0 x 0 with value bits 0, its slot left as it was -- also when the window covers the
//                tile wholly and the stored pixels would not be read: one rule for whoever puts the tiles back into their file;
//   3. is rebuilt at full size: reshrink_tile_image (pxz_varied_tile.h; clone-in, or varied_resize_tile by the whole block and the
//                RGB pack), called, not copied.  Skipped when the window covers the tile wholly;
//   4. is overlaid: the part's new pixels from patch_base into the tile image X, a wave per row: dwords where source and destination
//                agree modulo 4, bytes at the ends and otherwise.
//                THE ORDER: the overlay writes plain bytes over the FINISHED tile image -- C bytes per pixel, tightly packed, RGB
//                already packed to 3 bytes, RGBA already un-premultiplied by the expand -- and the shrink's own premultiply (step 5
//                of varied_ladder_tail) comes after it, over old and new pixels alike: what expanding the hull into an image,
//                writing the rectangle over it and shrinking that image does;
//   5. is measured, decided, resampled and stored: varied_oklab_raw / varied_sobel_sums and varied_ladder_tail (pxz_varied_tile.h)
//                with one rung, the text the ladders share.  The tail's F is X itself: with one rung X serves no second pair, so
//                the passes alternate between the two planes as reshrink_kernel's do and the block needs nothing beyond that
//                kernel's LDS.  No arithmetic is written here.
// In place: tile t's stored size and slot are read only by the block that writes tile t's outputs, into registers and LDS and
// before its first store (barriers lie between), so out_w / out_h / out_px may be the input arrays.
//
// LDS of one block: reshrink_lds with no rung channels (pxz_varied_tile.h), reshrink_kernel's layout and the call's limit
// (pxz_reshrink_lds_bytes):
//   [oklab tables, shrink_by only: 14 336 B] [P0: plane] [P1: plane] [windows of both axes: (bw + bh) * wdw dwords]
//   [the detector's planes, shrink_by with planes below 16 KB only: 16 KB]
// A plane is bw * bh dwords.  A is the plane the tile image leaves free, or the detector's own region where that exists; a
// horizontal result has at most w * h * C bytes and fits either.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

template <int C>
__global__ void __launch_bounds__(kVariedThreads) patch_kernel(const PatchArgs p)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	__shared__ uint32_t s_key[1];
	const VariedArgs &a = p.r.v;
	const TileResizeArgs &x = p.r.x;
	const uint32_t tid = threadIdx.x;
	const bool oklab = a.mode == 0u;
	const ReshrinkLds l = reshrink_lds(a.mode, a.bw, a.bh, 0u, x.wdw);
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint8_t *s_p0 = reinterpret_cast<uint8_t *>(lds) + l.p0;
	uint8_t *s_p1 = reinterpret_cast<uint8_t *>(lds) + l.p1;
	uint32_t *s_wx = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(lds) + l.wx), *s_wy = s_wx + x.wdw * a.bw;
	if (oklab) {
		oklab_fill_tables(s_lms, s_alpha, s_scale, tid);
		__syncthreads();
	}

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		// ---- 1. the window, the tile's place in the image and the part of it the window covers
		const uint32_t owner = owner_of(p.windows, p.n_windows, tile_g, &WindowEntry::tile0);
		const WindowEntry wn = p.windows[owner];
		const uint32_t tl = tile_g - wn.tile0;
		const uint32_t cty = tl / wn.ccols, ctx = tl - cty * wn.ccols;
		const uint32_t tx = wn.c0 + ctx, ty = wn.r0 + cty;
		const uint32_t w = tx + 1u == wn.cols ? wn.edge_w : a.bw;  // split.rs:18
		const uint32_t h = ty + 1u == wn.rows ? wn.edge_h : a.bh;  // split.rs:19
		const uint32_t n = w * h;
		const uint32_t tw = x.tile_w[tile_g], th = x.tile_h[tile_g];
		const uint8_t *src = x.slots + (size_t)tile_g * x.slot_bytes;
		// the tile is [px0, px0 + w) x [py0, py0 + h) of the image; a covered tile shares at least one pixel with the rectangle
		const uint32_t px0 = tx * a.bw, py0 = ty * a.bh;
		const uint32_t cx0 = wn.x > px0 ? wn.x - px0 : 0u, cy0 = wn.y > py0 ? wn.y - py0 : 0u;
		const uint32_t cx1 = wn.x + wn.w < px0 + w ? wn.x + wn.w - px0 : w, cy1 = wn.y + wn.h < py0 + h ? wn.y + wn.h - py0 : h;

		// ---- 2. a stored size that cannot be (bad_stored_size, pxz_device.h): flagged, its outputs empty, its slot left alone
		if (tw == 0u || th == 0u || tw > w || th > h) {
			if (tid == 0u) {
				atomicOr(x.status, 1u);
				if (p.window_flags) p.window_flags[owner] = 1u;
				a.value[tile_g] = 0.0f;
				a.out_w[tile_g] = 0u;
				a.out_h[tile_g] = 0u;
			}
			continue;
		}

		// ---- 3. the tile image X, tightly packed, and the plane it leaves free: cloned in or expanded, unless every pixel is new
		ReshrinkTileImage ti{s_p0, s_p1};
		const bool whole = cx0 == 0u && cy0 == 0u && cx1 == w && cy1 == h;
		if (!whole) ti = reshrink_tile_image<C>(x, src, tw, th, w, h, s_p0, s_p1, s_wx, s_wy, tid);
		uint8_t *s_x = ti.x;
		uint8_t *s_a = l.own != 0u ? reinterpret_cast<uint8_t *>(lds) + l.own : ti.free;  // I, or a vertical-only result
		float *s_plane = reinterpret_cast<float *>(s_a);                                  // [4][kVariedChunk] (the detector, before A holds a pass)

		// ---- 4. the new pixels over their part of X: a wave per row (X starts on 16 bytes, so a row's place in it gives its alignment)
		{
			const uint32_t row_bytes = (cx1 - cx0) * (uint32_t)C;
			const uint8_t *from = p.patch_base + wn.offset + (size_t)(py0 + cy0 - wn.y) * wn.pitch + (size_t)(px0 + cx0 - wn.x) * (uint32_t)C;
			const uint32_t wave = tid >> 6, lane = tid & 63u;
			for (uint32_t row = cy0 + wave; row < cy1; row += kVariedThreads / 64u) {
				const uint8_t *s = from + (size_t)(row - cy0) * wn.pitch;
				const uint32_t at = (row * w + cx0) * (uint32_t)C;
				uint8_t *d = s_x + at;
				uint32_t head = 0, body = 0;
				if (((uint32_t)reinterpret_cast<uintptr_t>(s) & 3u) == (at & 3u)) {
					head = (4u - (at & 3u)) & 3u;
					head = head < row_bytes ? head : row_bytes;
					body = (row_bytes - head) >> 2;
				}
				if (lane < head) d[lane] = s[lane];
				const uint32_t *s32 = reinterpret_cast<const uint32_t *>(s + head);
				uint32_t *d32 = reinterpret_cast<uint32_t *>(d + head);
				for (uint32_t i = lane; i < body; i += 64u) d32[i] = s32[i];
				for (uint32_t i = head + 4u * body + lane; i < row_bytes; i += 64u) d[i] = s[i];
			}
			__syncthreads();
		}

		// ---- 5. the detector up to what the factor has not entered, then the ladder's tail with one rung; F is X (see above)
		float xr = 0.0f;
		uint32_t shz = 0, svr = 0;
		if (oklab) xr = varied_oklab_raw<C>(s_x, n, s_lms, s_alpha, s_scale, s_plane, s_acc, tid);
		else varied_sobel_sums<C>(s_x, w, h, s_red, tid, shz, svr);
		varied_ladder_tail<C>(a, p.factor, 1u, tile_g, w, h, xr, shz, svr, s_key, s_x, s_a, s_x, tid);
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_patch(const PatchArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.r.v.n_tiles == 0u || a.n_windows == 0u) return hipSuccess;
	const uint32_t lds = reshrink_lds(a.r.v.mode, a.r.v.bw, a.r.v.bh, 0u, a.r.x.wdw).total;
	if (lds > kLdsPerCu) return hipErrorInvalidValue;
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.r.v.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(patch_kernel<4>) : go(patch_kernel<3>);
}

// ---------------------------------------------------------------------------
// The splice (pxz_splice_windows_device): the old files and the new records of the covered tiles -> the new files.  What the
// pieces and their bounds are is said at SpliceArgs (pxz_internal.h).  Five launches whatever the images and windows:
//   splice_flags_kernel   one thread per covered tile: an image is unusable when a window of it is flagged, when the reader left
//                         a covered tile without a record (rec_len 0) or when a new tile is empty -- so the kernels below never
//                         follow an offset the reader did not write, whether or not the caller passed the flags on;
//   splice_pieces_kernel  one wave per piece: its two bounds as byte offsets (the line tables are summed lane-parallel), its
//                         length; zero for an unusable image and for bounds that do not lie inside their file;
//   splice_scan_kernel    one block: the pieces' places, the files' offsets;
//   splice_copy_kernel    the bytes, balanced over the OUTPUT: a block takes 16 KB of it at a time, finds the pieces that end up
//                         there by a binary search over their places, and moves each span with 16-byte stores (byte head and tail;
//                         the source is read at whatever address it has), nothing at or beyond the capacity;
//   splice_rows_kernel    one thread per touched tile row: its new length into the copied line table.
// Every value is written with ordinary vector stores.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long splice_be32(const uint8_t *p)
{
	return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// the sum of the first n entries of a line table, by one wave; the same in every lane
__device__ __forceinline__ unsigned long long splice_line_sum(const uint8_t *table, uint32_t n, uint32_t lane)
{
	unsigned long long sum = 0;
	for (uint32_t q = lane; q < n; q += 64u) sum += splice_be32(table + 4ull * q);
	for (int sh = 32; sh >= 1; sh >>= 1) sum += __shfl_xor(sum, sh, 64);
	return sum;
}

// A bound as a byte offset into the old files' buffer (or the staging buffer), by one wave; b is the same in every lane, and so
// is the result.  false: the bound cannot be (its file is shorter than its tables, the reader left no record).
__device__ __forceinline__ bool splice_bound(const SpliceArgs &s, const SpliceBound &b, uint32_t lane, unsigned long long *at)
{
	switch (b.kind) {
	case SpliceBound::kFileStart: *at = s.file_offsets[b.a]; return true;
	case SpliceBound::kFileEnd: *at = s.file_offsets[b.a + 1u]; return true;
	case SpliceBound::kRow: {
		const WindowEntry wn = s.windows[b.a];
		const unsigned long long f0 = s.file_offsets[wn.image], f1 = s.file_offsets[wn.image + 1u], hdr = 26ull + 4ull * wn.rows;
		if (f1 < f0 || f1 - f0 < hdr || b.b > wn.rows) return false;
		*at = f0 + hdr + splice_line_sum(s.files + f0 + 26u, b.b, lane);
		return *at <= f1;
	}
	case SpliceBound::kRecStart:
	case SpliceBound::kRecEnd: {
		const uint32_t len = s.rec_len[b.a];
		if (len == 0u) return false;
		const unsigned long long off = s.rec_off[b.a];
		if (off < 23ull) return false;
		*at = b.kind == SpliceBound::kRecStart ? off - 23ull : off + len + 8ull;
		return true;
	}
	case SpliceBound::kStageRow: {
		const uint32_t crows = s.windows[b.a].crows;
		const unsigned long long f0 = s.stage_offsets[b.a], f1 = s.stage_offsets[b.a + 1u], hdr = 26ull + 4ull * crows;
		if (f1 < f0 || f1 - f0 < hdr || f1 > s.stage_capacity || b.b > crows) return false;
		*at = f0 + hdr + splice_line_sum(s.stage + f0 + 26u, b.b, lane);
		return *at <= f1;
	}
	default: return false;
	}
}

__global__ void __launch_bounds__(256) splice_flags_kernel(const SpliceArgs s)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= s.n_tiles) return;
	const uint32_t k = owner_of(s.windows, s.n_windows, t, &WindowEntry::tile0);
	const WindowEntry wn = s.windows[k];
	uint32_t bits = (s.rec_len[t] == 0u ? 2u : 0u) | ((s.new_w[t] == 0u || s.new_h[t] == 0u) ? 1u : 0u);
	if (t == wn.tile0) {
		if (s.reader_flags) bits |= s.reader_flags[k] & 3u;
		if (s.patch_flags) bits |= s.patch_flags[k] & 3u;
	}
	if (bits) atomicOr(s.image_flags + wn.image, bits);
}

__global__ void __launch_bounds__(256) splice_pieces_kernel(const SpliceArgs s)
{
	const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (p >= s.n_pieces) return;
	const SplicePiece pc = s.pieces[p];
	const bool staged = pc.lo.kind == SpliceBound::kStageRow;
	unsigned long long lo = 0, hi = 0;
	bool ok = s.image_flags[pc.image] == 0u;
	if (ok) ok = splice_bound(s, pc.lo, lane, &lo);
	if (ok) ok = splice_bound(s, pc.hi, lane, &hi);
	if (ok) ok = lo <= hi;
	if (ok && !staged) ok = lo >= s.file_offsets[pc.image] && hi <= s.file_offsets[pc.image + 1u];
	if (lane == 0u) {
		s.piece_src[p] = ok ? lo | (staged ? 1ull << 63 : 0ull) : 0ull;
		s.piece_len[p] = ok ? hi - lo : 0ull;
	}
}

__global__ void __launch_bounds__(1024) splice_scan_kernel(const SpliceArgs s)
{
	__shared__ unsigned long long s_wave[16];
	const uint32_t tid = threadIdx.x;
	const unsigned long long n = s.n_pieces, per = (n + 1023ull) / 1024ull;
	const unsigned long long b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
	unsigned long long sum = 0;
	for (unsigned long long p = b; p < e; ++p) sum += s.piece_len[p];
	unsigned long long incl = sum;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const unsigned long long u = __shfl_up(incl, off, 64);
		if ((tid & 63u) >= (uint32_t)off) incl += u;
	}
	if ((tid & 63u) == 63u) s_wave[tid >> 6] = incl;
	__syncthreads();
	unsigned long long run = incl - sum;
	for (uint32_t q = 0; q < (tid >> 6); ++q) run += s_wave[q];
	for (unsigned long long p = b; p < e; ++p) {
		s.piece_dst[p] = run;
		const SplicePiece pc = s.pieces[p];
		if (pc.first) s.out_file_offsets[pc.image] = run;
		run += s.piece_len[p];
	}
	if (tid == 1023u) {
		s.piece_dst[n] = run;
		s.out_file_offsets[s.n_images] = run;
	}
}

constexpr uint32_t kSpliceChunk = 16384;  // bytes of the output a block moves at a time

__global__ void __launch_bounds__(256) splice_copy_kernel(const SpliceArgs s)
{
	const uint32_t tid = threadIdx.x, n = s.n_pieces;
	const unsigned long long total = s.piece_dst[n], lim = total < s.capacity ? total : s.capacity;
	for (unsigned long long c0 = (unsigned long long)blockIdx.x * kSpliceChunk; c0 < lim; c0 += (unsigned long long)gridDim.x * kSpliceChunk) {
		const unsigned long long c1 = c0 + kSpliceChunk < lim ? c0 + kSpliceChunk : lim;
		// the last piece that starts at or before c0: it holds byte c0 (the pieces lie back to back, and c0 < total)
		uint32_t lo = 0, hi = n - 1u;
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo + 1u) / 2u;
			if (s.piece_dst[mid] <= c0) lo = mid;
			else hi = mid - 1u;
		}
		for (uint32_t p = lo; p < n; ++p) {
			const unsigned long long d0 = s.piece_dst[p];
			if (d0 >= c1) break;
			const unsigned long long len = s.piece_len[p];
			const unsigned long long a = d0 > c0 ? d0 : c0, b = d0 + len < c1 ? d0 + len : c1;
			if (a >= b) continue;
			const unsigned long long sw = s.piece_src[p];
			const uint8_t *S = ((sw >> 63) ? s.stage : s.files) + (sw & ~(1ull << 63)) + (a - d0);
			uint8_t *D = s.out + a;
			const uint32_t bytes = (uint32_t)(b - a);  // <= kSpliceChunk
			uint32_t head = (16u - ((uint32_t)reinterpret_cast<uintptr_t>(D) & 15u)) & 15u;
			head = head < bytes ? head : bytes;
			if (tid < head) D[tid] = S[tid];
			const uint32_t body = (bytes - head) >> 4;
			typedef uint32_t u32q_a1 __attribute__((ext_vector_type(4), aligned(1)));
			const u32q_a1 *s16 = reinterpret_cast<const u32q_a1 *>(S + head);
			uint4 *d16 = reinterpret_cast<uint4 *>(D + head);
			for (uint32_t i = tid; i < body; i += 256u) {
				const u32q_a1 v = s16[i];
				d16[i] = make_uint4(v.x, v.y, v.z, v.w);
			}
			for (uint32_t i = head + 16u * body + tid; i < bytes; i += 256u) D[i] = S[i];
		}
	}
}

__global__ void __launch_bounds__(256) splice_rows_kernel(const SpliceArgs s)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= s.n_rows) return;
	const SpliceRow r = s.rows[i];
	if (s.image_flags[r.image] != 0u) return;
	const unsigned long long f0 = s.file_offsets[r.image];
	unsigned long long len = splice_be32(s.files + f0 + 26ull + 4ull * r.row);
	for (uint32_t q = 0; q < r.n_parts; ++q) {
		const SpliceRowPart pt = s.parts[r.part0 + q];
		const WindowEntry wn = s.windows[pt.window];
		const uint32_t t0 = wn.tile0 + pt.crow * wn.ccols, t1 = t0 + wn.ccols - 1u;
		const unsigned long long old_bytes = (s.rec_off[t1] + s.rec_len[t1] + 8ull) - (s.rec_off[t0] - 23ull);
		len = len - old_bytes + splice_be32(s.stage + s.stage_offsets[pt.window] + 26ull + 4ull * pt.crow);
	}
	const unsigned long long at = s.out_file_offsets[r.image] + 26ull + 4ull * r.row;
	for (uint32_t b = 0; b < 4u; ++b)
		if (at + b < s.capacity) s.out[at + b] = (uint8_t)(len >> (8u * (3u - b)));
}

hipError_t launch_splice(const SpliceArgs &s, uint32_t n_cus, hipStream_t stream)
{
	if (s.n_pieces == 0u) return hipErrorInvalidValue;
	if (s.n_tiles) hipLaunchKernelGGL(splice_flags_kernel, dim3((s.n_tiles + 255u) / 256u), dim3(256), 0, stream, s);
	hipLaunchKernelGGL(splice_pieces_kernel, dim3((s.n_pieces + 3u) / 4u), dim3(256), 0, stream, s);
	hipLaunchKernelGGL(splice_scan_kernel, dim3(1), dim3(1024), 0, stream, s);
	hipLaunchKernelGGL(splice_copy_kernel, dim3(n_cus * 8u), dim3(256), 0, stream, s);
	if (s.n_rows) hipLaunchKernelGGL(splice_rows_kernel, dim3((s.n_rows + 255u) / 256u), dim3(256), 0, stream, s);
	return hipGetLastError();
}

}  // namespace pxz
