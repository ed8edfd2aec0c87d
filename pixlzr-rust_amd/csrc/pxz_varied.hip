// pxz_varied.hip -- batches of differently sized images (pxz_shrink_varied_frames_device, pxz_encode_varied_frames_device).
// The tiles of every image of the batch form one flat tile space: image i owns tiles [tile0, tile0 + cols * rows), in the
// reference's row-major order (src/data_types/iter.rs:64-76), and each tile finds its image by a binary search over the
// per-image table (owner_of, pxz_device.h).  One launch covers the batch, whatever the number of images.
//
// varied_kernel: one tile per block of 256 threads (grid-stride over the batch).  A tile is
//   1. staged      into LDS as tightly packed bytes (16-byte loads where its rows are aligned, dwords or bytes otherwise);
//   2. measured    shrink_by: get_block_variance with |x - avg| and x * factor * BASE_FACTOR (operations.rs:26-126,
//                  pixlzr.rs:160-162): the detector kernels' own colour conversion (pxz_oklab_math.h), 1024 pixels at a
//                  time, and four lanes that add them up in pixel order, twice -- the two sequential f32 sums of the
//                  reference; shrink_directionally: the integer gradient sums of operations.rs:192-259, then its f64
//                  normalisation by (w - 2)(h - 2) * 4096 -- the arithmetic finish_tile uses, per tile, so that any tile
//                  size decides its level exactly as the single-geometry call does with its integer breakpoints;
//   3. resampled   reduce_image_section (operations.rs:140-156) -> PixlzrBlock::resize (block.rs:273-334): a clone when
//                  nothing shrinks, else fir's premultiply (RGBA under a convolution) -> horizontal pass -> vertical pass
//                  -> un-premultiply, or the nearest pick, with the axis tables of the (source size, level) directory.
// The arithmetic of every step is the one the generic kernel and the tree rectangle kernel use (fir's i16 windows with
// i32 accumulators, clip, mul_div_255 and the reciprocal table's division), so a tile's value bits, sizes and pixels
// equal the single-geometry call's.
//
// Compiled with -ffp-contract=off (the detector's f32 arithmetic follows the reference's unfused operations).
#include "pxz_varied_tile.h"
#include "pxz_launch.h"

namespace pxz {

constexpr uint32_t kVariedPackChunk = 4096;                   // tiles per chunk of the writer's record scan (pxz_stream.hip)

// LDS of one block: [oklab tables, shrink_by only] [X: the tile, tile_bytes] [A: max(tile_bytes, the detector's planes)]
__host__ __device__ inline uint32_t varied_lds_bytes(uint32_t mode, uint32_t tile_bytes)
{
	const uint32_t tables = mode == 0u ? kVariedTables * 4u : 0u;
	const uint32_t a = mode == 0u && tile_bytes < kVariedPlaneBytes ? kVariedPlaneBytes : tile_bytes;
	return tables + tile_bytes + a;
}

template <int C>
__global__ void __launch_bounds__(kVariedThreads) varied_kernel(const VariedArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	__shared__ float s_acc[4];
	__shared__ uint32_t s_red[2 * (kVariedThreads / 64u)];
	const uint32_t tid = threadIdx.x;
	const bool oklab = a.mode == 0u;
	float4 *s_lms = reinterpret_cast<float4 *>(lds);
	float *s_alpha = reinterpret_cast<float *>(s_lms + 768);
	double *s_scale = reinterpret_cast<double *>(s_alpha + 256);
	uint8_t *s_x = reinterpret_cast<uint8_t *>(lds) + (oklab ? kVariedTables * 4u : 0u);
	uint8_t *s_a = s_x + a.tile_bytes;
	float *s_plane = reinterpret_cast<float *>(s_a);  // [4][kVariedChunk] (the detector, before A holds a pass)
	if (oklab) {
		oklab_fill_tables(s_lms, s_alpha, s_scale, tid);
		__syncthreads();
	}

	for (uint32_t tile_g = blockIdx.x; tile_g < a.n_tiles; tile_g += gridDim.x) {
		const VariedImage im = a.images[owner_of(a.images, a.n_images, tile_g, &VariedImage::tile0)];
		const uint32_t t = tile_g - im.tile0;
		const uint32_t ty = t / im.cols, tx = t - ty * im.cols;
		const uint32_t w = tx + 1u == im.cols ? im.edge_w : a.bw;  // split.rs:18
		const uint32_t h = ty + 1u == im.rows ? im.edge_h : a.bh;  // split.rs:19
		const uint32_t n = w * h;
		const uint8_t *src = a.base + im.offset + (size_t)(ty * a.bh) * im.pitch + (size_t)(tx * a.bw) * (uint32_t)C;

		// ---- 1. the tile into LDS, tightly packed
		if (C == 4 && (w & 3u) == 0u && ((reinterpret_cast<uintptr_t>(src) | im.pitch) & 15u) == 0u) {
			const uint32_t qpr = w >> 2;
			uint4 *d = reinterpret_cast<uint4 *>(s_x);
			for (uint32_t i = tid; i < qpr * h; i += kVariedThreads) {
				const uint32_t row = i / qpr, col = i - row * qpr;
				d[i] = *reinterpret_cast<const uint4 *>(src + (size_t)row * im.pitch + col * 16u);
			}
		} else if (C == 4 && ((reinterpret_cast<uintptr_t>(src) | im.pitch) & 3u) == 0u) {
			uint32_t *d = reinterpret_cast<uint32_t *>(s_x);
			for (uint32_t i = tid; i < n; i += kVariedThreads) {
				const uint32_t row = i / w, col = i - row * w;
				d[i] = *reinterpret_cast<const uint32_t *>(src + (size_t)row * im.pitch + col * 4u);
			}
		} else {
			const uint32_t rb = w * (uint32_t)C;
			for (uint32_t i = tid; i < n * (uint32_t)C; i += kVariedThreads) {
				const uint32_t row = i / rb, col = i - row * rb;
				s_x[i] = src[(size_t)row * im.pitch + col];
			}
		}
		__syncthreads();

		// ---- 2. the detector
		float v0, v1;
		if (oklab) {
			const float count = (float)n;  // operations.rs:51
			float mean = 0.0f;
			for (int pass = 0; pass < 2; ++pass) {
				float acc = 0.0f;
				for (uint32_t base = 0; base < n; base += kVariedChunk) {
					const uint32_t first = base + tid * 4u;
					uint32_t px[4];
#pragma unroll
					for (int j = 0; j < 4; ++j) px[j] = first + (uint32_t)j < n ? varied_pixel(s_x, first + (uint32_t)j, C) : 0u;
#pragma unroll
					for (int j = 0; j < 4; j += 2) {
						float o0[3], o1[3];
						oklab_pair(px[j], px[j + 1], s_lms, s_scale, o0, o1);
						const uint32_t k = tid * 4u + (uint32_t)j;
#pragma unroll
						for (int c = 0; c < 3; ++c) {
							s_plane[c * kVariedChunk + k] = o0[c];
							s_plane[c * kVariedChunk + k + 1u] = o1[c];
						}
						s_plane[3 * kVariedChunk + k] = s_alpha[px[j] >> 24];
						s_plane[3 * kVariedChunk + k + 1u] = s_alpha[px[j + 1] >> 24];
					}
					__syncthreads();
					if (tid < 4u) {
						// chains a, b, l, alpha: one lane each, in pixel order (operations.rs:60-63, :80-83)
						const uint32_t m = n - base < kVariedChunk ? n - base : kVariedChunk;
						const float *v = s_plane + tid * kVariedChunk;
						const uint32_t m4 = m & ~3u;
						if (pass == 0) {
							for (uint32_t i = 0; i < m4; i += 4u) {
								const float4 q = *reinterpret_cast<const float4 *>(v + i);
								acc += q.x; acc += q.y; acc += q.z; acc += q.w;
							}
							for (uint32_t i = m4; i < m; ++i) acc += v[i];
						} else {
							for (uint32_t i = 0; i < m4; i += 4u) {
								const float4 q = *reinterpret_cast<const float4 *>(v + i);
								acc += fabsf(q.x - mean); acc += fabsf(q.y - mean); acc += fabsf(q.z - mean); acc += fabsf(q.w - mean);
							}
							for (uint32_t i = m4; i < m; ++i) acc += fabsf(v[i] - mean);
						}
					}
					__syncthreads();
				}
				if (tid < 4u) {
					if (pass == 0) mean = __fdiv_rn(acc, count);  // :65-68
					else s_acc[tid] = acc;
				}
			}
			__syncthreads();
			const float total = C == 4 ? ((s_acc[0] + s_acc[1]) + s_acc[2]) + s_acc[3] : (s_acc[0] + s_acc[1]) + s_acc[2];  // :89 / :124
			const float x = __fdiv_rn(total, count);
			v0 = v1 = parse_value((x * a.factor) * 10.0f);  // pixlzr.rs:162 (BASE_FACTOR, :15), :177-178
		} else {
			// get_block_variance_directionally (operations.rs:192-259): Sobel-like sums over the (w - 2) x (h - 2) interior
			uint32_t shz = 0, svr = 0;
			if (w > 2u && h > 2u) {
				const uint32_t iw = w - 2u, rb = w * (uint32_t)C;
				for (uint32_t i = tid; i < iw * (h - 2u); i += kVariedThreads) {
					const uint32_t y = i / iw, x = i - y * iw;
					const uint8_t *p0 = s_x + y * rb + x * (uint32_t)C, *p1 = p0 + rb, *p2 = p1 + rb;
#pragma unroll
					for (int c = 0; c < 3; ++c) {
						const int32_t hz = -(int32_t)p0[c] - 2 * (int32_t)p0[C + c] - (int32_t)p0[2 * C + c] + (int32_t)p2[c] +
						                   2 * (int32_t)p2[C + c] + (int32_t)p2[2 * C + c];
						const int32_t vr = -(int32_t)p0[c] - 2 * (int32_t)p1[c] - (int32_t)p2[c] + (int32_t)p0[2 * C + c] +
						                   2 * (int32_t)p1[2 * C + c] + (int32_t)p2[2 * C + c];
						shz += (uint32_t)(hz < 0 ? -hz : hz);
						svr += (uint32_t)(vr < 0 ? -vr : vr);
					}
				}
			}
			for (int d = 32; d >= 1; d >>= 1) {
				shz += (uint32_t)__shfl_xor((int)shz, d, 64);
				svr += (uint32_t)__shfl_xor((int)svr, d, 64);
			}
			if ((tid & 63u) == 0u) {
				s_red[2u * (tid >> 6)] = shz;
				s_red[2u * (tid >> 6) + 1u] = svr;
			}
			__syncthreads();
			shz = svr = 0;
#pragma unroll
			for (uint32_t q = 0; q < kVariedThreads / 64u; ++q) {
				shz += s_red[2u * q];
				svr += s_red[2u * q + 1u];
			}
			const uint64_t fac = (uint64_t)(w - 2u) * (uint64_t)(h - 2u) * 4096ull;  // operations.rs:253-254
			if (fac == 0ull || w < 2u || h < 2u) {
				v0 = v1 = 0.0f;  // 0/0: the negative default NaN, which parse_value turns into 0 (finish_tile)
			} else {
				const double dfac = (double)fac;
				v0 = parse_value((float)((double)shz / dfac) * a.factor);  // :256-257, pixlzr.rs:199
				v1 = parse_value((float)((double)svr / dfac) * a.factor);
			}
		}
		// level_count against the thresholds (round(log2f(v)) >= -k), as the single-geometry call decides it
		uint32_t mx = 0, my = 0;
#pragma unroll
		for (int j = 0; j < kMaxLevel; ++j) {
			mx += v0 < a.thresholds[j] ? 1u : 0u;
			my += v1 < a.thresholds[j] ? 1u : 0u;
		}
		const uint32_t nw = reduced_size(w, mx), nh = reduced_size(h, my);  // operations.rs:150-151
		if (tid == 0u) {
			a.value[tile_g] = hypot_f32(v0, v1);  // operations.rs:154
			a.out_w[tile_g] = nw;
			a.out_h[tile_g] = nh;
		}

		// ---- 3. the resample into the tile's slot
		if (a.out_px != nullptr) {
			uint8_t *slot = a.out_px + (uint64_t)tile_g * a.slot_bytes;
			if (nw == w && nh == h) {
				varied_store(slot, s_x, n * (uint32_t)C, tid);  // block.rs:279-281: a clone
			} else {
				const bool nearest = a.filter == 0u;
				const bool need_h = nw != w, need_v = nh != h;
				const uint32_t lx = mx < (uint32_t)kMaxLevel ? mx : (uint32_t)kMaxLevel - 1u;
				const uint32_t ly = my < (uint32_t)kMaxLevel ? my : (uint32_t)kMaxLevel - 1u;
				if (C == 4 && !nearest) {
					// ResizeAlg::Convolution, default options: U8x4 is alpha-premultiplied first
					uint32_t *p32 = reinterpret_cast<uint32_t *>(s_x);
					for (uint32_t i = tid; i < n; i += kVariedThreads) p32[i] = premultiply(p32[i]);
					__syncthreads();
				}
				uint8_t *cur = s_x;
				if (need_h) {
					const TreeAxisEntry ex = a.dir[w * (uint32_t)kMaxLevel + lx];
					varied_pass<C>(a, ex, nearest, s_x, (uint32_t)C, w * (uint32_t)C, s_a, (uint32_t)C, nw * (uint32_t)C, h, tid);
					__syncthreads();
					cur = s_a;
				}
				if (need_v) {
					const TreeAxisEntry ey = a.dir[h * (uint32_t)kMaxLevel + ly];
					uint8_t *o = cur == s_x ? s_a : s_x;
					// one "line" per column of the nw-wide image, samples a row apart
					varied_pass<C>(a, ey, nearest, cur, nw * (uint32_t)C, (uint32_t)C, o, nw * (uint32_t)C, (uint32_t)C, nw, tid);
					__syncthreads();
					cur = o;
				}
				if (C == 4 && !nearest) {
					uint32_t *p32 = reinterpret_cast<uint32_t *>(cur);
					for (uint32_t i = tid; i < nw * nh; i += kVariedThreads) {
						const uint32_t px = p32[i], al = px >> 24;
						const uint32_t rc = kRecipAlpha.v[al];
						uint32_t r = ((px & 255u) * rc + 128u) >> 8, g = (((px >> 8) & 255u) * rc + 128u) >> 8, b = (((px >> 16) & 255u) * rc + 128u) >> 8;
						r = r > 255u ? 255u : r;
						g = g > 255u ? 255u : g;
						b = b > 255u ? 255u : b;
						p32[i] = r | (g << 8) | (b << 16) | (al << 24);
					}
					__syncthreads();
				}
				varied_store(slot, cur, nw * nh * (uint32_t)C, tid);
			}
		}
		__syncthreads();  // the next tile reuses LDS
	}
}

hipError_t launch_varied(const VariedArgs &a, uint32_t channels, uint32_t n_cus, hipStream_t stream)
{
	if (a.n_tiles == 0u) return hipSuccess;
	const uint32_t lds = varied_lds_bytes(a.mode, a.tile_bytes);
	auto go = [&](auto kernel) { return launch_with_lds(kernel, tile_blocks(a.n_tiles, lds, n_cus), kVariedThreads, lds, stream, a); };
	return channels == 4u ? go(varied_kernel<4>) : go(varied_kernel<3>);
}

uint32_t varied_lds_limit_bytes(uint32_t mode, uint32_t tile_bytes) { return varied_lds_bytes(mode, tile_bytes); }

// ---- writer ----------------------------------------------------------------------------------------------------------
// The records of the flat tile list are placed by the writer's own scan of their lengths.  Adding the header of image i + 1
// to the length of image i's last record makes that scan leave room for every header but the first (whose size is the
// writer's constant hdr_bytes): record t of image i then lands at hdr_0 + scan(t) = its place in file i.
__global__ void __launch_bounds__(256) varied_reclen_kernel(const VariedWriterArgs a)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i + 1u >= a.n_images) return;
	const VariedImage im = a.images[i];
	a.rec_len[im.tile0 + im.cols * im.rows - 1u] += a.images[i + 1u].hdr_bytes;
}

// file header + line-length table of every image (mod.rs:50-57,77-82): one thread per tile row of the batch
__global__ void __launch_bounds__(64) varied_headers_kernel(const VariedWriterArgs a)
{
	const uint32_t rg = blockIdx.x * 64u + threadIdx.x;
	if (rg >= a.n_rows) return;
	const uint32_t i = owner_of(a.images, a.n_images, rg, &VariedImage::row0);
	const VariedImage im = a.images[i];
	const uint32_t r = rg - im.row0;
	auto record_offset = [&](uint32_t t) -> unsigned long long {
		return t == a.n_tiles ? a.offsets[a.n_tiles] : a.chunk_totals[t / kVariedPackChunk] + a.offsets[t];
	};
	const unsigned long long hdr0 = a.images[0].hdr_bytes;
	const uint32_t next_hdr = i + 1u < a.n_images ? a.images[i + 1u].hdr_bytes : 0u;
	const uint32_t t0 = im.tile0 + r * im.cols;
	const unsigned long long row_lo = record_offset(t0), row_hi = record_offset(t0 + im.cols);
	const uint32_t len = (uint32_t)(row_hi - row_lo - (r + 1u == im.rows ? next_hdr : 0u));
	const unsigned long long file0 = hdr0 + record_offset(im.tile0) - im.hdr_bytes;
	if (r == 0u) {
		// exact whatever the room (a caller sizes its next buffer from file_offsets[n_images])
		a.file_offsets[i] = file0;
		if (i + 1u == a.n_images) a.file_offsets[a.n_images] = hdr0 + a.offsets[a.n_tiles];
	}
	if (file0 + im.hdr_bytes > a.capacity) return;
	uint8_t *hd = a.out + file0;
	uint8_t *lt = hd + 26 + 4 * r;
	lt[0] = (uint8_t)(len >> 24); lt[1] = (uint8_t)(len >> 16); lt[2] = (uint8_t)(len >> 8); lt[3] = (uint8_t)len;
	if (r == 0u) {
		const uint8_t magic[10] = {'P', 'I', 'X', 'L', 'Z', 'R', 0, 0, 2, (uint8_t)a.filter_byte};
		for (int k = 0; k < 10; ++k) hd[k] = magic[k];
		const uint32_t v[4] = {im.width, im.height, a.bw, a.bh};
		for (int k = 0; k < 4; ++k) {
			hd[10 + 4 * k] = (uint8_t)(v[k] >> 24);
			hd[11 + 4 * k] = (uint8_t)(v[k] >> 16);
			hd[12 + 4 * k] = (uint8_t)(v[k] >> 8);
			hd[13 + 4 * k] = (uint8_t)v[k];
		}
	}
}

hipError_t launch_varied_reclen(const VariedWriterArgs &a, hipStream_t stream)
{
	if (a.n_images < 2u) return hipSuccess;
	hipLaunchKernelGGL(varied_reclen_kernel, dim3((a.n_images + 255u) / 256u), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_varied_headers(const VariedWriterArgs &a, hipStream_t stream)
{
	hipLaunchKernelGGL(varied_headers_kernel, dim3((a.n_rows + 63u) / 64u), dim3(64), 0, stream, a);
	return hipGetLastError();
}

}  // namespace pxz
