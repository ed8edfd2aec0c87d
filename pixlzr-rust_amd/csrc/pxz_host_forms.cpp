// pxz_host_forms.cpp — the host forms: entry points of include/pixlzr_hip.h that take host pointers and compose the device
// entry points of pxz_api.cpp through the public C ABI -- reader, ladder, writer, distortion, fit and gather -- around
// handle scratch.  What the forms share stands once, up front: the header scan, the files' way up, the layout of a tile set
// and of the packed images, the flags check, the rung table, the writer's two passes and the fit tail.  From the runtime they
// take what pxz_runtime.h declares; of the handle they touch the scratch buffers, `stream` and `device`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/pixlzr_hip.h"
#include "pxz_launch.h"
#include "pxz_runtime.h"

namespace {

using namespace pxz_runtime;
using pxz::kLdsPerCu;

// A set of stored tiles in device memory: values, widths and heights (twelve bytes a tile, rounded up to 256), with the slots
// behind them.
struct TileSet {
	float *value;
	uint32_t *w, *h;
	uint8_t *slots;
	static uint64_t meta_bytes(uint64_t n_tiles) { return up256(n_tiles * 12u); }
	static uint64_t bytes(uint64_t n_tiles, uint64_t slot_bytes) { return meta_bytes(n_tiles) + n_tiles * slot_bytes; }
	TileSet(uint8_t *d = nullptr, uint64_t n_tiles = 0)
	    : value((float *)d), w((uint32_t *)(d + n_tiles * 4u)), h((uint32_t *)(d + n_tiles * 8u)), slots(d + meta_bytes(n_tiles)) {}
};

// The packed layout of n owners (pxz_image_desc or pxz_window) in device memory: tight pitch, starts aligned to 256 bytes.
// Returns the bytes of all.
template <class Owner>
uint64_t pack_owners(std::vector<Owner> *dev, uint32_t channels)
{
	uint64_t bytes = 0;
	for (Owner &o : *dev) {
		o.offset_bytes = bytes;
		o.pitch_bytes = o.width * channels;
		bytes += up256((uint64_t)o.pitch_bytes * o.height);
	}
	return bytes;
}

// The way back of n owners (pxz_image_desc or pxz_window): owner k's rows, tightly packed at packed[k].offset_bytes of stage,
// go to the caller's place and pitch (host[k]); flags holds the decode stage's n flags, then the expand stage's, merged into
// out_flags (or null).  Returns the first owner with a flag (n: none) and, in *first_flags, what it has.
template <class Owner>
uint32_t copy_out_owners(const Owner *host, const Owner *packed, uint32_t n, uint32_t channels, const uint8_t *stage, uint8_t *out_base,
                         const uint32_t *flags, uint32_t *out_flags, uint32_t *first_flags)
{
	uint32_t first_bad = n;
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t fl = flags[k] | flags[n + k];
		if (out_flags) out_flags[k] = fl;
		if (fl && first_bad == n) {
			first_bad = k;
			*first_flags = fl;
		}
		const size_t row = (size_t)host[k].width * channels;
		for (uint32_t y = 0; y < host[k].height; ++y)
			std::memcpy(out_base + host[k].offset_bytes + (size_t)y * host[k].pitch_bytes, stage + packed[k].offset_bytes + (size_t)y * row, row);
	}
	return first_bad;
}

// The host forms' images (checked, none null) into handle scratch, back to back with 256-byte aligned starts: *dev are their
// descriptors there, *raw the bytes of their pixels.
int send_images(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                std::vector<pxz_image_desc> *dev, uint64_t *raw)
{
	dev->assign(descs, descs + n_images);
	auto bytes_of = [&](uint32_t i) { return (uint64_t)descs[i].pitch_bytes * (descs[i].height - 1) + (uint64_t)descs[i].width * channels; };
	uint64_t in_bytes = 0;
	*raw = 0;
	for (uint32_t i = 0; i < n_images; ++i) {
		(*dev)[i].offset_bytes = in_bytes;
		in_bytes += up256(bytes_of(i));
		*raw += (uint64_t)descs[i].width * descs[i].height * channels;
	}
	const int rc = ensure(h, h->varied_in, in_bytes);
	if (rc != PXZ_OK) return rc;
	uint8_t *d_in = (uint8_t *)h->varied_in.ptr;
	for (uint32_t i = 0; i < n_images; ++i)
		PXZ_HIP(h, hipMemcpyAsync(d_in + (*dev)[i].offset_bytes, pixels[i], bytes_of(i), hipMemcpyHostToDevice, h->stream));
	return PXZ_OK;
}

// Every header first: a file that is not the image its descriptor announces is refused before anything is written.
// what: who expects the image ("batch", "call").  *file_bytes: the files' lengths added up.
int check_file_headers(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs, uint32_t n_images,
                       uint32_t channels, const pxz_params &p, const char *what, uint64_t *file_bytes)
{
	*file_bytes = 0;
	for (uint32_t i = 0; i < n_images; ++i) {
		if (!files[i]) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: null file", i);
		uint32_t w, hh, bw, bh, ch, fb;
		const char *why;
		const int rc = file_header(files[i], lens[i], &w, &hh, &bw, &bh, &ch, &fb, &why);
		if (rc != PXZ_OK) return fail(h, rc, "image %u: %s", i, why);
		if (w != descs[i].width || hh != descs[i].height || bw != p.block_w || bh != p.block_h || ch != channels)
			return fail(h, PXZ_ERR_INVALID_ARG, "image %u: the file holds %ux%u px in %ux%u blocks of %u channels, the %s expects %ux%u in %ux%u of %u",
			            i, w, hh, bw, bh, ch, what, descs[i].width, descs[i].height, p.block_w, p.block_h, channels);
		*file_bytes += lens[i];
	}
	return PXZ_OK;
}

// Every header first, for the forms that take their geometry from the files: they must share channels and block size.
// descs: the files' images, tightly pitched; raw: the bytes of their pixels.
struct FileScan {
	std::vector<pxz_image_desc> descs;
	uint32_t block_w = 0, block_h = 0, channels = 0;
	uint64_t file_bytes = 0, raw = 0;
};
int scan_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, FileScan *s)
{
	s->descs.resize(n_images);
	for (uint32_t i = 0; i < n_images; ++i) {
		if (!files[i]) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: null file", i);
		uint32_t w, hh, bw, bh, c, fb;
		const char *why;
		const int hrc = file_header(files[i], lens[i], &w, &hh, &bw, &bh, &c, &fb, &why);
		if (hrc != PXZ_OK) return fail(h, hrc, "image %u: %s", i, why);
		if (i == 0) {
			s->block_w = bw;
			s->block_h = bh;
			s->channels = c;
		} else if (bw != s->block_w || bh != s->block_h || c != s->channels) {
			return fail(h, PXZ_ERR_INVALID_ARG, "image %u: the file holds %ux%u blocks of %u channels, image 0 holds %ux%u of %u", i, bw, bh, c,
			            s->block_w, s->block_h, s->channels);
		}
		s->descs[i] = pxz_image_desc{w, hh, w * c, 0, 0};
		s->file_bytes += lens[i];
		s->raw += (uint64_t)w * hh * c;
	}
	return PXZ_OK;
}

// The files as the reader takes them, back to back behind their table of n_images + 1 offsets: the first sent_bytes() of
// `buffer`, which is grown to `room` bytes (the windows form keeps more in it).  stage: the host side of the one copy up, of
// max(what goes up, down_bytes) bytes -- one staging buffer for both directions, the results come back after the files have gone.
struct SentFiles {
	const uint64_t *d_offsets = nullptr;
	const uint8_t *d_files = nullptr;
	std::vector<uint8_t> stage;
};
uint64_t sent_bytes(uint32_t n_images, uint64_t file_bytes) { return 8ull * ((uint64_t)n_images + 1u) + file_bytes + 16u; }
int send_files(pxz_handle *h, DeviceBuffer &buffer, uint64_t room, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
               uint64_t file_bytes, uint64_t down_bytes, SentFiles *s)
{
	const uint64_t offs_bytes = 8ull * ((uint64_t)n_images + 1u);
	s->stage.resize((size_t)std::max(offs_bytes + file_bytes, down_bytes));
	uint64_t *offs = reinterpret_cast<uint64_t *>(s->stage.data());
	offs[0] = 0;
	for (uint32_t i = 0; i < n_images; ++i) {
		std::memcpy(s->stage.data() + offs_bytes + offs[i], files[i], lens[i]);
		offs[i + 1] = offs[i] + lens[i];
	}
	const int rc = ensure(h, buffer, room);
	if (rc != PXZ_OK) return rc;
	PXZ_HIP(h, hipMemcpyAsync(buffer.ptr, s->stage.data(), offs_bytes + file_bytes, hipMemcpyHostToDevice, h->stream));
	s->d_offsets = (const uint64_t *)buffer.ptr;
	s->d_files = (const uint8_t *)buffer.ptr + offs_bytes;
	return PXZ_OK;
}

// All or nothing: the flags of the reader (n_images) and of the stage behind it (n_images more) are fetched, and a malformed
// file or a tile that cannot be stops the call before the writer runs.
int check_stage_flags(pxz_handle *h, const uint32_t *d_flags, uint32_t n_images)
{
	std::vector<uint32_t> flags(2u * (size_t)n_images);
	PXZ_HIP(h, hipMemcpyAsync(flags.data(), d_flags, flags.size() * 4u, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	for (uint32_t i = 0; i < n_images; ++i)
		if (flags[i] | flags[n_images + i])
			return fail(h, PXZ_ERR_INVALID_ARG, "image %u: malformed .pixlzr file or record (flags %u); nothing was written", i,
			            flags[i] | flags[n_images + i]);
	return PXZ_OK;
}

// the descriptors once per rung: the rung sets as one varied batch of n_factors * n images
std::vector<pxz_image_desc> repeat_descs(const std::vector<pxz_image_desc> &descs, uint32_t n_factors)
{
	std::vector<pxz_image_desc> rungs;
	rungs.reserve((size_t)n_factors * descs.size());
	for (uint32_t r = 0; r < n_factors; ++r) rungs.insert(rungs.end(), descs.begin(), descs.end());
	return rungs;
}

// One block of handle scratch (rd) that one copy brings back (n_down u64s): the rung files' offsets (n_sets + 1), the sums (n_sets *
// ch) and, for a fit form of n_fit images (0: no fit), the chosen files' offsets (n_fit + 1), the choices and the flags (a choice and
// a flag: one u64 together) -- and behind it the room the offsets-only writer is given (none).
struct RungTable {
	size_t n_sets = 0, n_table = 0, n_down = 0;
	uint64_t *d_offs = nullptr, *d_sse = nullptr, *d_fit_offs = nullptr;
	uint8_t *d_room = nullptr;
};
int carve_rung_table(pxz_handle *h, size_t n_sets, uint32_t ch, size_t n_fit, RungTable *t)
{
	t->n_sets = n_sets;
	t->n_table = n_sets + 1u + n_sets * ch;
	t->n_down = t->n_table + (n_fit ? 2u * n_fit + 1u : 0u);
	const int rc = ensure(h, h->rd, t->n_down * 8u + 256u);
	if (rc != PXZ_OK) return rc;
	t->d_offs = (uint64_t *)h->rd.ptr;
	t->d_sse = t->d_offs + n_sets + 1u;
	t->d_fit_offs = t->d_offs + t->n_table;
	t->d_room = (uint8_t *)(t->d_offs + t->n_down);
	return PXZ_OK;
}

// the table as the callers want it: the files' lengths and the sums (either may be null)
void unpack_rung_table(const uint64_t *got, size_t n_sets, uint32_t ch, uint64_t *file_bytes, uint64_t *sse)
{
	if (file_bytes)
		for (size_t k = 0; k < n_sets; ++k) file_bytes[k] = got[k + 1u] - got[k];
	if (sse) std::memcpy(sse, got + n_sets + 1u, n_sets * ch * 8u);
}

// where the rate-distortion forms end: the table comes down, the stream drains, and the caller gets it unpacked
int download_rung_table(pxz_handle *h, const RungTable &t, uint32_t ch, uint64_t *file_bytes, uint64_t *sse)
{
	std::vector<uint64_t> got(t.n_table);
	PXZ_HIP(h, hipMemcpyAsync(got.data(), t.d_offs, t.n_table * 8u, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	unpack_rung_table(got.data(), t.n_sets, ch, file_bytes, sse);
	return PXZ_OK;
}

// Fills the table of the rungs `all` (rung-major, n_factors sets of the images descs): the writer over the descriptors once per
// rung, for its offsets alone, then the rungs' distortion -- against the images at d_images (ref null: descs say where), or
// against the archive's own tiles *ref, which expand_filter expands and which lie in the layout of src_bw x src_bh blocks: the
// block of p (the re-shrink's distortion) or another (the re-tile's).  The tile-fit forms want the same per tile: with
// d_record_bytes the writer's pass is pxz_record_bytes_varied_device (the offsets come with it), and d_tile_sse takes the
// distortion call's per-tile sums (both null: the per-image forms, as before).
int rung_table(pxz_handle *h, const std::vector<pxz_image_desc> &descs, uint32_t n_factors, uint32_t ch, const pxz_params &p, const pxz_params &up,
               const TileSet &all, const RungTable &t, const uint8_t *d_images, const TileSet *ref, uint32_t src_bw, uint32_t src_bh,
               uint32_t expand_filter, uint32_t *d_record_bytes = nullptr, uint64_t *d_tile_sse = nullptr)
{
	const std::vector<pxz_image_desc> rungs = repeat_descs(descs, n_factors);
	const int rc = d_record_bytes ? pxz_record_bytes_varied_device(h, rungs.data(), (uint32_t)rungs.size(), ch, &p, all.value, all.w, all.h, all.slots,
	                                                               d_record_bytes, t.d_offs)
	                              : pxz_encode_varied_frames_device(h, rungs.data(), (uint32_t)rungs.size(), ch, &p, 0, all.value, all.w, all.h, all.slots,
	                                                                t.d_room, 0, t.d_offs);
	if (rc != PXZ_OK) return rc;
	if (!ref)
		return pxz_distortion_varied_frames_device(h, rungs.data(), (uint32_t)rungs.size(), ch, &up, d_images, all.w, all.h, all.slots, d_tile_sse, t.d_sse,
		                                           nullptr);
	if (src_bw != p.block_w || src_bh != p.block_h)
		return pxz_retile_distortion_varied_device(h, descs.data(), (uint32_t)descs.size(), ch, src_bw, src_bh, &up, expand_filter, n_factors, ref->w, ref->h,
		                                           ref->slots, all.w, all.h, all.slots, d_tile_sse, t.d_sse, nullptr);
	return pxz_reshrink_distortion_varied_device(h, descs.data(), (uint32_t)descs.size(), ch, &up, expand_filter, n_factors, ref->w, ref->h, ref->slots,
	                                             all.w, all.h, all.slots, d_tile_sse, t.d_sse, nullptr);
}

// The files of `tiles` (n_factors sets of the images descs, rung-major) into varied_files and out to the caller: a first guess
// at their room (raw: the bytes of the images' pixels; n_tiles: the tiles of one set), and one more writer pass when it was
// short -- the offsets are exact whichever pass wrote them, so they come down once, behind the first: the n_block u64s at
// d_block into *got, the offsets among them at offs_at.  file_offsets is filled also when out is too small; nothing goes out then.
int write_files(pxz_handle *h, const std::vector<pxz_image_desc> &descs, uint32_t n_factors, uint32_t ch, const pxz_params &p, uint32_t filter_byte,
                const TileSet &tiles, uint64_t raw, uint32_t n_tiles, uint64_t *d_block, size_t n_block, size_t offs_at, std::vector<uint64_t> *got,
                uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets)
{
	const std::vector<pxz_image_desc> rungs = repeat_descs(descs, n_factors);
	const uint32_t n_files = (uint32_t)rungs.size();
	got->resize(n_block);
	uint64_t cap = (raw + raw / 4u + 64ull * n_tiles + 4096ull * descs.size()) * n_factors;
	if (cap < h->varied_files.cap) cap = h->varied_files.cap;
	for (int pass = 0; pass < 2; ++pass) {
		int rc = ensure(h, h->varied_files, cap);
		if (rc != PXZ_OK) return rc;
		if ((rc = pxz_encode_varied_frames_device(h, rungs.data(), n_files, ch, &p, filter_byte, tiles.value, tiles.w, tiles.h, tiles.slots,
		                                          (uint8_t *)h->varied_files.ptr, cap, d_block + offs_at)) != PXZ_OK)
			return rc;
		if (pass == 0) PXZ_HIP(h, hipMemcpyAsync(got->data(), d_block, n_block * 8u, hipMemcpyDeviceToHost, h->stream));
		PXZ_HIP(h, hipStreamSynchronize(h->stream));
		if ((*got)[offs_at + n_files] <= cap) break;
		cap = (*got)[offs_at + n_files];
	}
	std::memcpy(file_offsets, got->data() + offs_at, ((size_t)n_files + 1u) * 8u);
	const uint64_t total = file_offsets[n_files];
	if (!out || out_capacity < total)
		return fail(h, PXZ_ERR_BUFFER_TOO_SMALL, "the files need %llu bytes, out holds %llu", (unsigned long long)total,
		            (unsigned long long)out_capacity);
	PXZ_HIP(h, hipMemcpy(out, h->varied_files.ptr, total, hipMemcpyDeviceToHost));
	return PXZ_OK;
}

// The images as the device calls take them (of the image forms: where send_images put them), every rung's tiles in varied_out
// and their table in rd.
struct Rungs {
	std::vector<pxz_image_desc> descs;
	pxz_params p;   // the ladder's and the writer's: factor 1 (ignored by the ladder calls)
	uint32_t ch = 0, n_tiles = 0;  // (the tiles of one rung)
	uint64_t raw = 0;
	TileSet all;
	RungTable t;
	bool per_tile = false;             // the tile-fit forms (set by the caller): the two tables below are wanted
	uint32_t *d_record_bytes = nullptr;  // every rung's record bytes (n_factors * n_tiles) ...
	uint64_t *d_tile_sse = nullptr;      // ... and squared errors per channel, in tilefit_tables
};

// the per-tile tables of the tile-fit forms, over `tiles` = n_factors * n_tiles rung tiles (nothing unless s->per_tile)
int carve_tile_tables(pxz_handle *h, uint64_t tiles, uint32_t ch, Rungs *s)
{
	if (!s->per_tile) return PXZ_OK;
	const uint64_t sse_at = up256(tiles * 4u);
	const int rc = ensure(h, h->tilefit_tables, sse_at + tiles * ch * 8u);
	if (rc != PXZ_OK) return rc;
	s->d_record_bytes = (uint32_t *)h->tilefit_tables.ptr;
	s->d_tile_sse = (uint64_t *)((uint8_t *)h->tilefit_tables.ptr + sse_at);
	return PXZ_OK;
}

// The image forms from their parameter checks to the filled table: the ladder over the images, then rung_table against the
// images themselves.  criterion: the fit form's, checked in its place among the others (null: no fit).
int image_rungs(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels, uint32_t block_w,
                uint32_t block_h, uint32_t mode, uint32_t filter_down, uint32_t filter_up, const float *factors, uint32_t n_factors,
                const uint32_t *criterion, Rungs *s)
{
	s->p = pxz_params{block_w, block_h, mode, filter_down, 1.0f, 0};
	const pxz_params up{block_w, block_h, 0, filter_up, 0.0f, 0};
	int rc = check_params(h, &up);
	if (rc != PXZ_OK) return rc;
	if ((rc = varied_check_params(h, channels, &s->p)) != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	if ((rc = varied_plan(h, descs, n_images, block_w, block_h, channels, mode, &images, nullptr, nullptr)) != PXZ_OK) return rc;
	if (criterion && (rc = fit_check(h, n_images, n_factors, channels, *criterion)) != PXZ_OK) return rc;
	for (uint32_t i = 0; i < n_images; ++i)
		if (!pixels[i]) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: null pixels", i);
	s->ch = channels;
	s->n_tiles = varied_n_tiles(images);
	const uint64_t n_sets = (uint64_t)n_factors * n_images, tiles = (uint64_t)n_factors * s->n_tiles;
	if (tiles > 0xffffffffull || n_sets > 0xffffffffull)
		return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	PXZ_HIP(h, hipSetDevice(h->device));
	if ((rc = send_images(h, pixels, descs, n_images, channels, &s->descs, &s->raw)) != PXZ_OK) return rc;
	const uint64_t slot = (uint64_t)block_w * block_h * channels;
	if ((rc = ensure(h, h->varied_out, TileSet::bytes(tiles, slot))) != PXZ_OK) return rc;
	if ((rc = carve_rung_table(h, (size_t)n_sets, channels, criterion ? n_images : 0u, &s->t)) != PXZ_OK) return rc;
	if ((rc = carve_tile_tables(h, tiles, channels, s)) != PXZ_OK) return rc;
	const uint8_t *d_in = (const uint8_t *)h->varied_in.ptr;
	s->all = TileSet((uint8_t *)h->varied_out.ptr, tiles);
	if ((rc = pxz_shrink_varied_ladder_frames_device(h, s->descs.data(), n_images, channels, &s->p, factors, n_factors, d_in, s->all.value, s->all.w,
	                                                 s->all.h, s->all.slots)) != PXZ_OK)
		return rc;
	return rung_table(h, s->descs, n_factors, channels, s->p, up, s->all, s->t, d_in, nullptr, 0, 0, 0, s->d_record_bytes, s->d_tile_sse);
}

// The archive forms from their parameter checks to the filled table: the files parsed and uploaded, the reader at the files'
// geometry into a buffer of its own (NOT rung 0: the reference is kept), the rungs into varied_out, the flags of both stages
// checked, then rung_table.  params' block is the rungs'; the files' comes from their headers.
//   equal blocks:   the re-shrink ladder out of place; rung_table against the reference (the re-shrink's distortion).
//   another block (new_block: the forms that take one; the others refuse it): the images in handle scratch (varied_in) -> the
//     varied ladder; rung_table against those images.  The rule of transcode_varied would send a pair whose new block divides the
//     files' on both axes through the re-tile ladder and rung_table against the reference in the files' layout (the re-tile's
//     distortion), with nothing of image size anywhere.  That route measured SLOWER files to files than the images, by 7-9 % on
//     strongly shrunk files in two runs whose samples spread by 1 %, and level elsewhere, so by 8o's precedent
//     every other block takes the images; the route is kept for the measurement build alone.  The device calls take every pair.
// The tables are the same on every path.
int archive_rungs(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *params,
                  uint32_t expand_filter, uint32_t filter_up, const float *factors, uint32_t n_factors, bool fit, bool new_block, Rungs *s)
{
	if (n_images == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	if (expand_filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "expand_filter must be 0..4, got %u", expand_filter);
	if (filter_up > 4) return fail(h, PXZ_ERR_INVALID_ARG, "filter_up must be 0..4, got %u", filter_up);
	s->p = *params;
	s->p.factor = 1.0f;
	int rc = check_params(h, &s->p);
	if (rc != PXZ_OK) return rc;
	FileScan scan;
	if ((rc = scan_files(h, files, lens, n_images, &scan)) != PXZ_OK) return rc;
	const uint32_t fbw = scan.block_w, fbh = scan.block_h, ch = scan.channels;
	const bool same_block = fbw == s->p.block_w && fbh == s->p.block_h;
	if (!same_block && !new_block)
		return fail(h, PXZ_ERR_UNSUPPORTED,
		            "the files hold %ux%u blocks, params ask for %ux%u: this call needs an unchanged block size (pxz_rate_distortion_retile_files, "
		            "pxz_retile_varied_files_fit and pxz_retile_varied_files_fit_tiles take another)", fbw, fbh, s->p.block_w, s->p.block_h);
	pxz_params pin = s->p;  // the files' own geometry
	pin.block_w = fbw;
	pin.block_h = fbh;
	pin.filter = expand_filter;
	if (same_block) {
		if ((rc = reshrink_check_block(h, s->p.mode, fbw, fbh, ch, 1u)) != PXZ_OK) return rc;
		if (reshrink_distortion_bytes(fbw, fbh, 1u) > kLdsPerCu)
			return fail(h, PXZ_ERR_UNSUPPORTED, "the distortion of re-shrunk tiles keeps three planes of block_w*block_h dwords in LDS (%ux%u)", fbw, fbh);
	} else {
		const pxz_params px = decode_side_params(&pin, true);
		if ((rc = varied_check_params(h, ch, &px)) != PXZ_OK) return rc;
		if ((rc = varied_check_params(h, ch, &s->p)) != PXZ_OK) return rc;
	}
	std::vector<pxz::VariedImage> images_in, images;
	if (!same_block && (rc = varied_plan(h, scan.descs.data(), n_images, fbw, fbh, 0, 0, &images_in, nullptr, nullptr)) != PXZ_OK) return rc;
	if ((rc = varied_plan(h, scan.descs.data(), n_images, s->p.block_w, s->p.block_h, ch, s->p.mode, &images, nullptr, nullptr)) != PXZ_OK) return rc;
	s->descs = std::move(scan.descs);
	s->raw = scan.raw;
	s->ch = ch;
	s->n_tiles = varied_n_tiles(images);
	const uint32_t n_in = same_block ? s->n_tiles : varied_n_tiles(images_in);
	const uint64_t n_sets = (uint64_t)n_factors * n_images, tiles = (uint64_t)n_factors * s->n_tiles;
	if (tiles > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	// another block: the images (the rule above).  The re-tile route stays behind a measurement build (make exp EXP=41):
	// there a pair whose new tiles split tiles of the files, and that both kernels take, goes through the re-tile ladder
#if defined(PXZ_EXP) && PXZ_EXP == 41
	uint32_t ladder_bytes = 0, distortion_bytes = 0;
	const bool retile = !same_block && fbw % s->p.block_w == 0 && fbh % s->p.block_h == 0 &&
	                    pxz_retile_ladder_lds_bytes(fbw, fbh, s->p.block_w, s->p.block_h, ch, s->p.mode, expand_filter, &ladder_bytes) == PXZ_OK &&
	                    ladder_bytes <= kLdsPerCu &&
	                    pxz_retile_distortion_lds_bytes(fbw, fbh, s->p.block_w, s->p.block_h, ch, expand_filter, filter_up, &distortion_bytes) == PXZ_OK &&
	                    distortion_bytes <= kLdsPerCu;
#else
	const bool retile = false;
#endif
	const bool by_images = !same_block && !retile;
	PXZ_HIP(h, hipSetDevice(h->device));
	SentFiles sent;
	if ((rc = send_files(h, h->transcode_files, sent_bytes(n_images, scan.file_bytes), files, lens, n_images, scan.file_bytes, 0, &sent)) != PXZ_OK)
		return rc;

	// the archive's tiles and the flags of the reader and the stage behind it (archive_tiles); every rung's tiles (varied_out)
	const uint64_t slot_in = (uint64_t)fbw * fbh * ch, slot = (uint64_t)s->p.block_w * s->p.block_h * ch;
	const uint64_t flags_at = up256(TileSet::bytes(n_in, slot_in));
	if ((rc = ensure(h, h->archive_tiles, flags_at + 8ull * n_images)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->varied_out, TileSet::bytes(tiles, slot))) != PXZ_OK) return rc;
	if ((rc = carve_rung_table(h, (size_t)n_sets, ch, fit ? n_images : 0u, &s->t)) != PXZ_OK) return rc;
	if ((rc = carve_tile_tables(h, tiles, ch, s)) != PXZ_OK) return rc;
	uint8_t *d_img = nullptr;
	if (by_images) {
		const uint64_t img_bytes = pack_owners(&s->descs, ch);
		if ((rc = ensure(h, h->varied_in, img_bytes)) != PXZ_OK) return rc;
		d_img = (uint8_t *)h->varied_in.ptr;
	}
	uint8_t *d_ref = (uint8_t *)h->archive_tiles.ptr;
	const TileSet ref(d_ref, n_in);
	uint32_t *d_flags = (uint32_t *)(d_ref + flags_at);
	s->all = TileSet((uint8_t *)h->varied_out.ptr, tiles);

	// reader -> the reference; ladder out of place -> the rungs
	PXZ_HIP(h, hipMemsetAsync(d_ref, 0, TileSet::meta_bytes(n_in), h->stream));  // (a tile the reader cannot reach keeps size 0 and is flagged)
	if ((rc = pxz_decode_varied_frames_device(h, s->descs.data(), n_images, ch, &pin, sent.d_files, sent.d_offsets, ref.value, ref.w, ref.h, ref.slots,
	                                          d_flags)) != PXZ_OK)
		return rc;
	if (same_block) {
		rc = pxz_reshrink_varied_ladder_frames_device(h, s->descs.data(), n_images, ch, &s->p, expand_filter, factors, n_factors, ref.w, ref.h, ref.slots,
		                                              s->all.value, s->all.w, s->all.h, s->all.slots, d_flags + n_images);
	} else if (retile) {
		rc = pxz_retile_varied_ladder_frames_device(h, s->descs.data(), n_images, ch, fbw, fbh, &s->p, expand_filter, factors, n_factors, ref.w, ref.h,
		                                            ref.slots, s->all.value, s->all.w, s->all.h, s->all.slots, d_flags + n_images);
	} else {
		if ((rc = pxz_expand_varied_frames_device(h, s->descs.data(), n_images, ch, &pin, ref.w, ref.h, ref.slots, d_img, d_flags + n_images)) != PXZ_OK)
			return rc;
		rc = pxz_shrink_varied_ladder_frames_device(h, s->descs.data(), n_images, ch, &s->p, factors, n_factors, d_img, s->all.value, s->all.w, s->all.h,
		                                            s->all.slots);
	}
	if (rc != PXZ_OK) return rc;
	if ((rc = check_stage_flags(h, d_flags, n_images)) != PXZ_OK) return rc;
	pxz_params up = s->p;
	up.filter = filter_up;
	return rung_table(h, s->descs, n_factors, ch, s->p, up, s->all, s->t, d_img, by_images ? nullptr : &ref, fbw, fbh, expand_filter, s->d_record_bytes,
	                  s->d_tile_sse);
}

// Where both fit forms end, behind the filled table: one rung per image chosen on the device, its tiles gathered as a varied
// batch of the images themselves (fit_tiles), the files written, and the one download unpacked -- the table (optional), the
// files' offsets, the choices and the flags.
int fit_and_write(pxz_handle *h, const Rungs &s, uint32_t n_factors, uint32_t criterion, const uint64_t *targets, uint32_t filter_byte, uint8_t *out,
                  uint64_t out_capacity, uint64_t *file_offsets, uint32_t *choice, uint32_t *fit_flags, uint64_t *table_bytes, uint64_t *table_sse)
{
	const uint32_t n_images = (uint32_t)s.descs.size();
	const uint64_t slot = (uint64_t)s.p.block_w * s.p.block_h * s.ch;
	int rc = ensure(h, h->fit_tiles, TileSet::bytes(s.n_tiles, slot));
	if (rc != PXZ_OK) return rc;
	const TileSet fit((uint8_t *)h->fit_tiles.ptr, s.n_tiles);
	uint64_t *d_offs = s.t.d_fit_offs;
	uint32_t *d_choice = (uint32_t *)(d_offs + n_images + 1u), *d_flags = d_choice + n_images;
	if ((rc = pxz_fit_varied_ladder_device(h, n_images, n_factors, s.ch, criterion, targets, s.t.d_offs, s.t.d_sse, d_choice, d_flags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_gather_varied_rungs_device(h, s.descs.data(), n_images, s.ch, &s.p, n_factors, d_choice, s.all.value, s.all.w, s.all.h, s.all.slots,
	                                         fit.value, fit.w, fit.h, fit.slots, nullptr)) != PXZ_OK)
		return rc;
	std::vector<uint64_t> got;
	rc = write_files(h, s.descs, 1u, s.ch, s.p, filter_byte, fit, s.raw, s.n_tiles, s.t.d_offs, s.t.n_down, s.t.n_table, &got, out, out_capacity,
	                 file_offsets);
	if (rc != PXZ_OK && rc != PXZ_ERR_BUFFER_TOO_SMALL) return rc;
	unpack_rung_table(got.data(), s.t.n_sets, s.ch, table_bytes, table_sse);
	const uint32_t *picked = reinterpret_cast<const uint32_t *>(got.data() + s.t.n_table + n_images + 1u);
	std::memcpy(choice, picked, (size_t)n_images * 4u);
	std::memcpy(fit_flags, picked + n_images, (size_t)n_images * 4u);
	return rc;
}

// Where both tile-fit forms end, behind the filled tables: one rung per tile chosen on the device under the groups' targets,
// the chosen tiles gathered as a varied batch of the images themselves (fit_tiles), the files written, and the one download
// unpacked -- the files' offsets, the groups' results and the tiles' choices (optional).
int fit_tiles_and_write(pxz_handle *h, const Rungs &s, uint32_t n_factors, uint32_t criterion, const uint32_t *group_first, uint32_t n_groups,
                        const uint64_t *targets, uint32_t filter_byte, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets, uint32_t *tile_choice,
                        uint64_t *group_lambda, uint64_t *group_bytes, uint64_t *group_sse, uint32_t *group_flags)
{
	const uint32_t n_images = (uint32_t)s.descs.size();
	const uint64_t slot = (uint64_t)s.p.block_w * s.p.block_h * s.ch;
	int rc = ensure(h, h->fit_tiles, TileSet::bytes(s.n_tiles, slot));
	if (rc != PXZ_OK) return rc;
	const TileSet fit((uint8_t *)h->fit_tiles.ptr, s.n_tiles);
	// what comes down in one copy: the files' offsets (n_images + 1) | lambda | bytes | sse (n_groups u64 each) | as dwords the
	// groups' flags, the gather's image flags and the tiles' choices
	const size_t G = n_groups, n_dwords = G + n_images + (size_t)s.n_tiles;
	const size_t n_block = (size_t)n_images + 1u + 3u * G + (n_dwords + 1u) / 2u;
	if ((rc = ensure(h, h->tilefit_down, n_block * 8u)) != PXZ_OK) return rc;
	uint64_t *d_block = (uint64_t *)h->tilefit_down.ptr;
	uint64_t *d_lambda = d_block + n_images + 1u, *d_bytes = d_lambda + G, *d_sse = d_bytes + G;
	uint32_t *d_gflags = (uint32_t *)(d_sse + G), *d_iflags = d_gflags + G, *d_choice = d_iflags + n_images;
	if ((rc = pxz_fit_varied_tiles_device(h, s.descs.data(), n_images, s.ch, &s.p, group_first, n_groups, n_factors, criterion, targets, s.d_record_bytes,
	                                      s.d_tile_sse, d_choice, d_lambda, d_bytes, d_sse, d_gflags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_gather_varied_tile_rungs_device(h, s.descs.data(), n_images, s.ch, &s.p, n_factors, d_choice, s.all.value, s.all.w, s.all.h,
	                                              s.all.slots, fit.value, fit.w, fit.h, fit.slots, d_iflags)) != PXZ_OK)
		return rc;
	std::vector<uint64_t> got;
	rc = write_files(h, s.descs, 1u, s.ch, s.p, filter_byte, fit, s.raw, s.n_tiles, d_block, n_block, 0, &got, out, out_capacity, file_offsets);
	if (rc != PXZ_OK && rc != PXZ_ERR_BUFFER_TOO_SMALL) return rc;
	const uint64_t *g64 = got.data() + n_images + 1u;
	std::memcpy(group_lambda, g64, G * 8u);
	std::memcpy(group_bytes, g64 + G, G * 8u);
	std::memcpy(group_sse, g64 + 2u * G, G * 8u);
	const uint32_t *g32 = reinterpret_cast<const uint32_t *>(g64 + 3u * G);
	std::memcpy(group_flags, g32, G * 4u);
	if (tile_choice) std::memcpy(tile_choice, g32 + G + n_images, (size_t)s.n_tiles * 4u);
	// the library's own ladder gives every tile a usable candidate at every rung, and the select no rung beyond the ladder
	for (uint32_t g = 0; g < n_groups; ++g)
		if (g32[g] & 2u) return fail(h, PXZ_ERR_INTERNAL, "group %u: a tile of the library's own ladder has no usable candidate", g);
	for (uint32_t i = 0; i < n_images; ++i)
		if (g32[G + i]) return fail(h, PXZ_ERR_INTERNAL, "image %u: the select chose a rung beyond the ladder (flags %u)", i, g32[G + i]);
	return rc;
}

// what the tile-fit forms check of their own arguments before anything is uploaded
int fit_tiles_check(pxz_handle *h, uint32_t n_images, uint32_t criterion, const uint32_t *group_first, uint32_t n_groups, const uint64_t *targets,
                    const void *file_offsets, const void *group_lambda, const void *group_bytes, const void *group_sse, const void *group_flags)
{
	if (!targets) return fail(h, PXZ_ERR_INVALID_ARG, "null targets");
	if (!file_offsets || !group_lambda || !group_bytes || !group_sse || !group_flags) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if (criterion != PXZ_FIT_BYTES && criterion != PXZ_FIT_SSE)
		return fail(h, PXZ_ERR_INVALID_ARG, "criterion must be PXZ_FIT_BYTES (0) or PXZ_FIT_SSE (1), got %u", criterion);
	return tile_groups_check(h, group_first, n_groups, n_images);
}

// The three archive forms behind their entry points, each twice: new_block false are the forms that need the files' block to be
// params' (pxz_rate_distortion_varied_files, pxz_transcode_varied_files_fit, pxz_transcode_varied_files_fit_tiles), true the
// forms that take another (pxz_rate_distortion_retile_files, pxz_retile_varied_files_fit, pxz_retile_varied_files_fit_tiles).
int archive_table(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *params, uint32_t expand_filter,
                  uint32_t filter_up, const float *factors, uint32_t n_factors, bool new_block, uint64_t *file_bytes, uint64_t *sse)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!files || !lens || !params || !file_bytes || !sse) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	Rungs s;
	if ((rc = archive_rungs(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, false, new_block, &s)) != PXZ_OK) return rc;
	return download_rung_table(h, s.t, s.ch, file_bytes, sse);
}

int archive_fit(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *params, uint32_t expand_filter,
                uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion, const uint64_t *targets, uint32_t filter_byte,
                bool new_block, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets, uint32_t *choice, uint32_t *fit_flags, uint64_t *table_bytes,
                uint64_t *table_sse)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!targets) return fail(h, PXZ_ERR_INVALID_ARG, "null targets");
	if (!files || !lens || !params || !file_offsets || !choice || !fit_flags) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if (criterion != PXZ_FIT_BYTES && criterion != PXZ_FIT_SSE)
		return fail(h, PXZ_ERR_INVALID_ARG, "criterion must be PXZ_FIT_BYTES (0) or PXZ_FIT_SSE (1), got %u", criterion);
	Rungs s;
	if ((rc = archive_rungs(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, true, new_block, &s)) != PXZ_OK) return rc;
	return fit_and_write(h, s, n_factors, criterion, targets, filter_byte, out, out_capacity, file_offsets, choice, fit_flags, table_bytes, table_sse);
}

int archive_fit_tiles(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *params,
                      uint32_t expand_filter, uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                      const uint32_t *group_first, uint32_t n_groups, const uint64_t *targets, uint32_t filter_byte, bool new_block, uint8_t *out,
                      uint64_t out_capacity, uint64_t *file_offsets, uint32_t *tile_choice, uint64_t *group_lambda, uint64_t *group_bytes,
                      uint64_t *group_sse, uint32_t *group_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!files || !lens || !params) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if (n_images == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	if ((rc = fit_tiles_check(h, n_images, criterion, group_first, n_groups, targets, file_offsets, group_lambda, group_bytes, group_sse, group_flags)) !=
	    PXZ_OK)
		return rc;
	Rungs s;
	s.per_tile = true;
	if ((rc = archive_rungs(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, true, new_block, &s)) != PXZ_OK) return rc;
	return fit_tiles_and_write(h, s, n_factors, criterion, group_first, n_groups, targets, filter_byte, out, out_capacity, file_offsets, tile_choice,
	                           group_lambda, group_bytes, group_sse, group_flags);
}

// Both host forms of pix_to_pix behind one body: factors == nullptr is pxz_transcode_varied_files (one rung, the caller's
// params->factor, the one-factor calls); otherwise pxz_transcode_varied_ladder_files (n_factors rungs, the ladder calls, the
// outputs rung-major and the writer over the descriptors repeated n_factors times).
int transcode_varied(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *user_params,
                     uint32_t expand_filter, const float *factors, uint32_t n_factors, uint32_t filter_byte, uint8_t *out,
                     uint64_t out_capacity, uint64_t *file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!files || !lens || !user_params || !file_offsets) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const bool ladder = factors != nullptr;
	pxz_params ladder_params = *user_params;
	ladder_params.factor = 1.0f;  // (ignored by the ladder calls)
	const pxz_params *params = ladder ? &ladder_params : user_params;
	if (n_images == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	if (expand_filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "expand_filter must be 0..4, got %u", expand_filter);
	FileScan scan;
	int rc = scan_files(h, files, lens, n_images, &scan);
	if (rc != PXZ_OK) return rc;
	const std::vector<pxz_image_desc> &descs = scan.descs;
	const uint32_t fbw = scan.block_w, fbh = scan.block_h, ch = scan.channels;
	const bool same_block = fbw == params->block_w && fbh == params->block_h;
	pxz_params pin = *params;  // the files' own geometry
	pin.block_w = fbw;
	pin.block_h = fbh;
	pin.filter = expand_filter;
	if (same_block) {
		if ((rc = check_params(h, params)) != PXZ_OK) return rc;
		if ((rc = reshrink_check_block(h, params->mode, fbw, fbh, ladder ? ch : 0u, 1u)) != PXZ_OK) return rc;
	} else {
		const pxz_params px = decode_side_params(&pin, true);
		if ((rc = varied_check_params(h, ch, &px)) != PXZ_OK) return rc;
		if ((rc = varied_check_params(h, ch, params)) != PXZ_OK) return rc;
	}
	std::vector<pxz::VariedImage> images_in, images_out;
	if ((rc = varied_plan(h, descs.data(), n_images, fbw, fbh, 0, 0, &images_in, nullptr, nullptr)) != PXZ_OK) return rc;
	if ((rc = varied_plan(h, descs.data(), n_images, params->block_w, params->block_h, ch, params->mode, &images_out, nullptr, nullptr)) != PXZ_OK)
		return rc;
	const uint32_t n_out = varied_n_tiles(images_out), n_in = varied_n_tiles(images_in);
	if ((uint64_t)n_factors * n_out > 0xffffffffull) return fail(h, PXZ_ERR_UNSUPPORTED, "more than 2^32-1 tiles over the %u rungs", n_factors);
	const uint32_t n_all = n_factors * n_out, n_files = n_factors * n_images;  // (n_files: 2^32-1 at most, a file has a tile)
	PXZ_HIP(h, hipSetDevice(h->device));
	SentFiles sent;
	if ((rc = send_files(h, h->transcode_files, sent_bytes(n_images, scan.file_bytes), files, lens, n_images, scan.file_bytes, 0, &sent)) != PXZ_OK)
		return rc;

	// the tiles that go to the writer, rung-major: values, sizes, slots, then the new files' offsets and the flags of both stages
	const uint64_t slot_out = (uint64_t)params->block_w * params->block_h * ch;
	const uint64_t offs_at = (TileSet::bytes(n_all, slot_out) + 7u) & ~(uint64_t)7u;
	const uint64_t flags_at = offs_at + 8ull * ((uint64_t)n_files + 1u);
	if ((rc = ensure(h, h->varied_out, flags_at + 8ull * n_images)) != PXZ_OK) return rc;
	uint8_t *d_out = (uint8_t *)h->varied_out.ptr;
	const TileSet m(d_out, n_all);  // (the reader fills rung 0 of each array)
	uint64_t *d_offs = (uint64_t *)(d_out + offs_at);
	uint32_t *d_flags = (uint32_t *)(d_out + flags_at);

	if (same_block) {
		// reader -> re-shrink in place (the ladder: in place on rung 0) -> writer: nothing of image size anywhere
		PXZ_HIP(h, hipMemsetAsync(d_out, 0, TileSet::meta_bytes(n_all), h->stream));  // (a tile the reader cannot reach keeps size 0 and is flagged)
		if ((rc = pxz_decode_varied_frames_device(h, descs.data(), n_images, ch, &pin, sent.d_files, sent.d_offsets, m.value, m.w, m.h, m.slots,
		                                          d_flags)) != PXZ_OK)
			return rc;
		rc = ladder ? pxz_reshrink_varied_ladder_frames_device(h, descs.data(), n_images, ch, params, expand_filter, factors, n_factors, m.w, m.h,
		                                                       m.slots, m.value, m.w, m.h, m.slots, d_flags + n_images)
		            : pxz_reshrink_varied_frames_device(h, descs.data(), n_images, ch, params, expand_filter, m.w, m.h, m.slots, m.value, m.w, m.h,
		                                                m.slots, d_flags + n_images);
		if (rc != PXZ_OK) return rc;
	} else {
		// another block size: reader at the files' geometry, then
		//   a pair of blocks that retile_kernel (one factor) or retile_ladder_kernel (the ladder) takes and whose new tiles each lie
		//   inside one tile of the files -- the new block divides the files' on both axes: the re-tile, or the re-tile ladder, at the
		//   new geometry, nothing of image size anywhere;
		//   any other pair: the images in handle scratch -> the varied shrink, or the varied ladder, at the new geometry.  (New tiles
		//   that merge or straddle tiles of the files measured slower through the re-tile than through these four calls, files to
		//   files, by more than the spread of two runs: 0.76-0.93x on strongly shrunk files; for the ladder see 8p.  The
		//   device calls take every pair.)
		const uint64_t slot_in = (uint64_t)fbw * fbh * ch;
		if ((rc = ensure(h, h->transcode_tiles, TileSet::bytes(n_in, slot_in))) != PXZ_OK) return rc;
		const TileSet mi((uint8_t *)h->transcode_tiles.ptr, n_in);
		uint32_t retile_bytes = 0;
		const bool retile = fbw % params->block_w == 0 && fbh % params->block_h == 0 &&
		                    (ladder ? pxz_retile_ladder_lds_bytes(fbw, fbh, params->block_w, params->block_h, ch, params->mode, expand_filter, &retile_bytes)
		                            : pxz_retile_lds_bytes(fbw, fbh, params->block_w, params->block_h, params->mode, expand_filter, &retile_bytes)) == PXZ_OK &&
		                    retile_bytes <= kLdsPerCu;
		std::vector<pxz_image_desc> dev = descs;
		uint8_t *d_img = nullptr;
		if (!retile) {
			const uint64_t img_bytes = pack_owners(&dev, ch);
			if ((rc = ensure(h, h->varied_in, img_bytes)) != PXZ_OK) return rc;
			d_img = (uint8_t *)h->varied_in.ptr;
		}
		PXZ_HIP(h, hipMemsetAsync(mi.value, 0, TileSet::meta_bytes(n_in), h->stream));
		if ((rc = pxz_decode_varied_frames_device(h, descs.data(), n_images, ch, &pin, sent.d_files, sent.d_offsets, mi.value, mi.w, mi.h, mi.slots,
		                                          d_flags)) != PXZ_OK)
			return rc;
		if (retile) {
			rc = ladder ? pxz_retile_varied_ladder_frames_device(h, descs.data(), n_images, ch, fbw, fbh, params, expand_filter, factors, n_factors, mi.w,
			                                                     mi.h, mi.slots, m.value, m.w, m.h, m.slots, d_flags + n_images)
			            : pxz_retile_varied_frames_device(h, descs.data(), n_images, ch, fbw, fbh, params, expand_filter, mi.w, mi.h, mi.slots, m.value,
			                                              m.w, m.h, m.slots, d_flags + n_images);
		} else {
			if ((rc = pxz_expand_varied_frames_device(h, dev.data(), n_images, ch, &pin, mi.w, mi.h, mi.slots, d_img, d_flags + n_images)) != PXZ_OK)
				return rc;
			rc = ladder ? pxz_shrink_varied_ladder_frames_device(h, dev.data(), n_images, ch, params, factors, n_factors, d_img, m.value, m.w, m.h, m.slots)
			            : pxz_shrink_varied_frames_device(h, dev.data(), n_images, ch, params, d_img, m.value, m.w, m.h, m.slots);
		}
		if (rc != PXZ_OK) return rc;
	}
	if ((rc = check_stage_flags(h, d_flags, n_images)) != PXZ_OK) return rc;
	std::vector<uint64_t> got;
	return write_files(h, descs, n_factors, ch, *params, filter_byte, m, scan.raw, n_out, d_offs, (size_t)n_files + 1u, 0, &got, out, out_capacity,
	                   file_offsets);
}

}  // namespace

extern "C" {

int pxz_encode_varied_images(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                             uint32_t channels, const pxz_params *params, uint32_t filter_byte, uint8_t *out,
                             uint64_t out_capacity, uint64_t *file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!pixels || !params || !file_offsets) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	int rc = varied_check_params(h, channels, params);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	if ((rc = varied_plan(h, descs, n_images, params->block_w, params->block_h, channels, params->mode, &images, nullptr, nullptr)) != PXZ_OK)
		return rc;
	for (uint32_t i = 0; i < n_images; ++i)
		if (!pixels[i]) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: null pixels", i);
	PXZ_HIP(h, hipSetDevice(h->device));
	// the images, back to back, and the tiles' outputs with the files' offsets behind them
	std::vector<pxz_image_desc> dev;
	uint64_t raw = 0;
	if ((rc = send_images(h, pixels, descs, n_images, channels, &dev, &raw)) != PXZ_OK) return rc;
	const uint32_t n_tiles = varied_n_tiles(images);
	const uint64_t offs_at = TileSet::bytes(n_tiles, (uint64_t)params->block_w * params->block_h * channels);
	if ((rc = ensure(h, h->varied_out, offs_at + 8u * ((uint64_t)n_images + 1u))) != PXZ_OK) return rc;
	uint8_t *d_out = (uint8_t *)h->varied_out.ptr;
	const TileSet m(d_out, n_tiles);
	if ((rc = pxz_shrink_varied_frames_device(h, dev.data(), n_images, channels, params, (const uint8_t *)h->varied_in.ptr, m.value, m.w, m.h,
	                                          m.slots)) != PXZ_OK)
		return rc;
	std::vector<uint64_t> got;
	return write_files(h, dev, 1u, channels, *params, filter_byte, m, raw, n_tiles, (uint64_t *)(d_out + offs_at), (size_t)n_images + 1u, 0, &got, out,
	                   out_capacity, file_offsets);
}

int pxz_decode_varied_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs,
                            uint32_t n_images, uint32_t channels, const pxz_params *params, uint8_t *out_base, uint32_t *image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!files || !lens || !params || !out_base) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	if ((rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, channels, 0, &images, nullptr, nullptr)) != PXZ_OK) return rc;
	uint64_t file_bytes = 0;
	if ((rc = check_file_headers(h, files, lens, descs, n_images, channels, p, "batch", &file_bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	// device side: the files back to back behind their offsets; the images tightly packed
	std::vector<pxz_image_desc> dev(descs, descs + n_images);
	const uint64_t img_bytes = pack_owners(&dev, channels);
	const uint32_t n_tiles = varied_n_tiles(images);
	const uint64_t slot = (uint64_t)p.block_w * p.block_h * channels;
	const uint64_t flags_at = TileSet::bytes(n_tiles, slot);
	SentFiles sent;
	if ((rc = send_files(h, h->varied_files, sent_bytes(n_images, file_bytes), files, lens, n_images, file_bytes, img_bytes, &sent)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->varied_out, flags_at + 8ull * n_images)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->varied_in, img_bytes)) != PXZ_OK) return rc;
	uint8_t *d_out = (uint8_t *)h->varied_out.ptr, *d_img = (uint8_t *)h->varied_in.ptr;
	const TileSet m(d_out, n_tiles);
	PXZ_HIP(h, hipMemsetAsync(m.slots, 0, (size_t)n_tiles * slot, h->stream));
	PXZ_HIP(h, hipMemsetAsync(d_img, 0, img_bytes, h->stream));  // (the place of a tile that cannot be expanded stays zero)
	uint32_t *d_flags = (uint32_t *)(d_out + flags_at);
	if ((rc = pxz_decode_varied_frames_device(h, dev.data(), n_images, channels, &p, sent.d_files, sent.d_offsets, m.value, m.w, m.h, m.slots,
	                                          d_flags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_expand_varied_frames_device(h, dev.data(), n_images, channels, &p, m.w, m.h, m.slots, d_img, d_flags + n_images)) != PXZ_OK)
		return rc;
	std::vector<uint32_t> flags(2u * (size_t)n_images);
	PXZ_HIP(h, hipStreamSynchronize(h->stream));  // the files have left the staging buffer
	PXZ_HIP(h, hipMemcpyAsync(sent.stage.data(), d_img, img_bytes, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(flags.data(), d_flags, flags.size() * 4u, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	uint32_t first_flags = 0;
	const uint32_t first_bad = copy_out_owners(descs, dev.data(), n_images, channels, sent.stage.data(), out_base, flags.data(), image_flags, &first_flags);
	if (first_bad != n_images)
		return fail(h, PXZ_ERR_INVALID_ARG, "image %u: malformed .pixlzr file or record (flags %u); the other images are complete", first_bad,
		            first_flags);
	return PXZ_OK;
}

int pxz_transcode_varied_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                               const pxz_params *params, uint32_t expand_filter, uint32_t filter_byte, uint8_t *out,
                               uint64_t out_capacity, uint64_t *file_offsets)
{
	return transcode_varied(h, files, lens, n_images, params, expand_filter, nullptr, 1u, filter_byte, out, out_capacity, file_offsets);
}

int pxz_transcode_varied_ladder_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                      const pxz_params *params, uint32_t expand_filter, const float *factors, uint32_t n_factors,
                                      uint32_t filter_byte, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	const int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	return transcode_varied(h, files, lens, n_images, params, expand_filter, factors, n_factors, filter_byte, out, out_capacity, file_offsets);
}

int pxz_rate_distortion_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                              uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                              uint32_t filter_up, const float *factors, uint32_t n_factors, uint64_t *file_bytes, uint64_t *sse)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!factors) return fail(h, PXZ_ERR_INVALID_ARG, "null factors");
	if (n_factors == 0 || n_factors > PXZ_LADDER_MAX_RUNGS)
		return fail(h, PXZ_ERR_INVALID_ARG, "n_factors must be 1..%u, got %u", PXZ_LADDER_MAX_RUNGS, n_factors);
	if (!pixels || !file_bytes || !sse) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	pxz_params p{block_w, block_h, mode, filter_down, 1.0f, 0};
	pxz_params up{block_w, block_h, 0, filter_up, 0.0f, 0};
	int rc = check_params(h, &up);
	if (rc != PXZ_OK) return rc;
	pxz_frames f;
	size_t tiles = 0, slot = 0;
	if ((rc = stage_host_image(h, pixels, width, height, channels, pitch_bytes, &p, n_factors, true, &f, &tiles, &slot)) != PXZ_OK) return rc;
	RungTable t;
	if ((rc = carve_rung_table(h, n_factors, channels, 0, &t)) != PXZ_OK) return rc;
	const uint8_t *d_in = (const uint8_t *)h->in.ptr;
	float *d_val = (float *)h->val.ptr;
	uint32_t *d_w = (uint32_t *)h->ow.ptr, *d_h = (uint32_t *)h->oh.ptr;
	uint8_t *d_slots = (uint8_t *)h->out.ptr;
	if ((rc = pxz_shrink_ladder_frames_device(h, &f, &p, factors, n_factors, d_in, d_val, d_w, d_h, d_slots)) != PXZ_OK) return rc;
	pxz_frames rungs = f;  // the rung sets as a batch of n_factors frames
	rungs.n_frames = n_factors;
	rungs.frame_stride_bytes = (uint64_t)f.pitch_bytes * height;
	if ((rc = pxz_encode_frames_device(h, &rungs, &p, 0, d_val, d_w, d_h, d_slots, t.d_room, 0, t.d_offs)) != PXZ_OK) return rc;
	if ((rc = pxz_distortion_frames_device(h, &f, &up, n_factors, d_in, d_w, d_h, d_slots, nullptr, t.d_sse)) != PXZ_OK) return rc;
	return download_rung_table(h, t, channels, file_bytes, sse);
}

int pxz_rate_distortion_varied_images(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                                      uint32_t channels, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                                      uint32_t filter_up, const float *factors, uint32_t n_factors, uint64_t *file_bytes, uint64_t *sse)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!pixels || !file_bytes || !sse) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	Rungs s;
	if ((rc = image_rungs(h, pixels, descs, n_images, channels, block_w, block_h, mode, filter_down, filter_up, factors, n_factors, nullptr, &s)) != PXZ_OK)
		return rc;
	return download_rung_table(h, s.t, channels, file_bytes, sse);
}

int pxz_encode_varied_images_fit(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                                 uint32_t channels, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                                 uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                                 const uint64_t *targets, uint32_t filter_byte, uint8_t *out, uint64_t out_capacity,
                                 uint64_t *file_offsets, uint32_t *choice, uint32_t *fit_flags, uint64_t *table_bytes, uint64_t *table_sse)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!targets) return fail(h, PXZ_ERR_INVALID_ARG, "null targets");
	if (!pixels || !file_offsets || !choice || !fit_flags) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	Rungs s;
	if ((rc = image_rungs(h, pixels, descs, n_images, channels, block_w, block_h, mode, filter_down, filter_up, factors, n_factors, &criterion, &s)) !=
	    PXZ_OK)
		return rc;
	return fit_and_write(h, s, n_factors, criterion, targets, filter_byte, out, out_capacity, file_offsets, choice, fit_flags, table_bytes, table_sse);
}

int pxz_rate_distortion_varied_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                     const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                     uint32_t n_factors, uint64_t *file_bytes, uint64_t *sse)
{
	return archive_table(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, false, file_bytes, sse);
}

int pxz_rate_distortion_retile_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                     const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                     uint32_t n_factors, uint64_t *file_bytes, uint64_t *sse)
{
	return archive_table(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, true, file_bytes, sse);
}

int pxz_transcode_varied_files_fit(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                   const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                   uint32_t n_factors, uint32_t criterion, const uint64_t *targets, uint32_t filter_byte, uint8_t *out,
                                   uint64_t out_capacity, uint64_t *file_offsets, uint32_t *choice, uint32_t *fit_flags, uint64_t *table_bytes,
                                   uint64_t *table_sse)
{
	return archive_fit(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, criterion, targets, filter_byte, false, out,
	                   out_capacity, file_offsets, choice, fit_flags, table_bytes, table_sse);
}

int pxz_retile_varied_files_fit(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *params,
                                uint32_t expand_filter, uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                                const uint64_t *targets, uint32_t filter_byte, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets,
                                uint32_t *choice, uint32_t *fit_flags, uint64_t *table_bytes, uint64_t *table_sse)
{
	return archive_fit(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, criterion, targets, filter_byte, true, out,
	                   out_capacity, file_offsets, choice, fit_flags, table_bytes, table_sse);
}

int pxz_encode_varied_images_fit_tiles(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                                       uint32_t channels, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                                       uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                                       const uint32_t *group_first, uint32_t n_groups, const uint64_t *targets, uint32_t filter_byte, uint8_t *out,
                                       uint64_t out_capacity, uint64_t *file_offsets, uint32_t *tile_choice, uint64_t *group_lambda,
                                       uint64_t *group_bytes, uint64_t *group_sse, uint32_t *group_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	int rc = check_factors(h, factors, n_factors, PXZ_VARIED_LADDER_MAX_RUNGS);
	if (rc != PXZ_OK) return rc;
	if (!pixels) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if ((rc = fit_tiles_check(h, n_images, criterion, group_first, n_groups, targets, file_offsets, group_lambda, group_bytes, group_sse, group_flags)) !=
	    PXZ_OK)
		return rc;
	Rungs s;
	s.per_tile = true;
	if ((rc = image_rungs(h, pixels, descs, n_images, channels, block_w, block_h, mode, filter_down, filter_up, factors, n_factors, &criterion, &s)) !=
	    PXZ_OK)
		return rc;
	return fit_tiles_and_write(h, s, n_factors, criterion, group_first, n_groups, targets, filter_byte, out, out_capacity, file_offsets, tile_choice,
	                           group_lambda, group_bytes, group_sse, group_flags);
}

int pxz_transcode_varied_files_fit_tiles(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                         const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                         uint32_t n_factors, uint32_t criterion, const uint32_t *group_first, uint32_t n_groups,
                                         const uint64_t *targets, uint32_t filter_byte, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets,
                                         uint32_t *tile_choice, uint64_t *group_lambda, uint64_t *group_bytes, uint64_t *group_sse,
                                         uint32_t *group_flags)
{
	return archive_fit_tiles(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, criterion, group_first, n_groups, targets,
	                         filter_byte, false, out, out_capacity, file_offsets, tile_choice, group_lambda, group_bytes, group_sse, group_flags);
}

int pxz_retile_varied_files_fit_tiles(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_params *params,
                                      uint32_t expand_filter, uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                                      const uint32_t *group_first, uint32_t n_groups, const uint64_t *targets, uint32_t filter_byte, uint8_t *out,
                                      uint64_t out_capacity, uint64_t *file_offsets, uint32_t *tile_choice, uint64_t *group_lambda,
                                      uint64_t *group_bytes, uint64_t *group_sse, uint32_t *group_flags)
{
	return archive_fit_tiles(h, files, lens, n_images, params, expand_filter, filter_up, factors, n_factors, criterion, group_first, n_groups, targets,
	                         filter_byte, true, out, out_capacity, file_offsets, tile_choice, group_lambda, group_bytes, group_sse, group_flags);
}

int pxz_decode_windows_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs, uint32_t n_images,
                             const pxz_window *windows, uint32_t n_windows, uint32_t channels, const pxz_params *params, uint8_t *out_base,
                             uint64_t out_bytes, uint32_t *window_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!files || !lens || !params || !out_base) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::WindowEntry> entries;
	if ((rc = window_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, channels, &entries, nullptr, nullptr)) != PXZ_OK) return rc;
	for (uint32_t k = 0; k < n_windows; ++k) {
		const pxz_window &g = windows[k];
		if (g.offset_bytes > out_bytes || (uint64_t)(g.height - 1u) * g.pitch_bytes + (uint64_t)g.width * channels > out_bytes - g.offset_bytes)
			return fail(h, PXZ_ERR_BUFFER_TOO_SMALL, "window %u: its output ends behind the %llu bytes of the buffer", k, (unsigned long long)out_bytes);
	}
	uint64_t file_bytes = 0;
	if ((rc = check_file_headers(h, files, lens, descs, n_images, channels, p, "call", &file_bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	// device side, one buffer: the files back to back behind their offsets | the covered tiles | the crops tightly packed with
	// the two flag arrays behind them
	std::vector<pxz_window> dev(windows, windows + n_windows);
	const uint64_t crop_bytes = pack_owners(&dev, channels);
	const uint32_t n_tiles = window_n_tiles(entries);
	const uint64_t slot = (uint64_t)p.block_w * p.block_h * channels;
	const uint64_t tiles_at = up256(sent_bytes(n_images, file_bytes)), crops_at = tiles_at + up256(TileSet::bytes(n_tiles, slot));
	const uint64_t flags_at = crops_at + crop_bytes, down_bytes = crop_bytes + 8ull * n_windows;
	SentFiles sent;
	if ((rc = send_files(h, h->window_host, flags_at + 8ull * n_windows, files, lens, n_images, file_bytes, down_bytes, &sent)) != PXZ_OK) return rc;
	uint8_t *d = (uint8_t *)h->window_host.ptr;
	PXZ_HIP(h, hipMemsetAsync(d + crops_at, 0, down_bytes, h->stream));  // (the place of a tile that cannot be expanded stays zero)
	const TileSet m(d + tiles_at, n_tiles);
	uint32_t *d_flags = (uint32_t *)(d + flags_at);
	if ((rc = pxz_decode_windows_device(h, descs, n_images, dev.data(), n_windows, channels, &p, sent.d_files, sent.d_offsets, m.value, m.w, m.h, m.slots,
	                                    d_flags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_expand_windows_device(h, descs, n_images, dev.data(), n_windows, channels, &p, m.w, m.h, m.slots, d + crops_at, d_flags + n_windows)) !=
	    PXZ_OK)
		return rc;
	PXZ_HIP(h, hipStreamSynchronize(h->stream));  // the files have left the staging buffer
	PXZ_HIP(h, hipMemcpyAsync(sent.stage.data(), d + crops_at, down_bytes, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	const uint32_t *flags = reinterpret_cast<const uint32_t *>(sent.stage.data() + crop_bytes);
	uint32_t first_flags = 0;
	const uint32_t first_bad = copy_out_owners(windows, dev.data(), n_windows, channels, sent.stage.data(), out_base, flags, window_flags, &first_flags);
	if (first_bad != n_windows)
		return fail(h, PXZ_ERR_INVALID_ARG, "window %u: malformed .pixlzr file or record in what it reads of image %u (flags %u); the other windows are complete",
		            first_bad, windows[first_bad].image, first_flags);
	return PXZ_OK;
}

// ---- decode at reduced scale: the two forms above with a scale per owner.  The descriptors (windows) the caller passed keep
// the FILE's geometry; `out` are the same owners with their SCALED width and height at the caller's pitch and offset, which is
// what pack_owners and copy_out_owners lay out and copy.

int pxz_decode_varied_files_scaled(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs, uint32_t n_images,
                                   uint32_t channels, const pxz_params *params, const uint32_t *scale_log2, uint8_t *out_base, uint32_t *image_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!files || !lens || !params || !out_base || !scale_log2) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::VariedImage> images;
	if ((rc = varied_plan(h, descs, n_images, p.block_w, p.block_h, 0, 0, &images, nullptr, nullptr)) != PXZ_OK) return rc;
	std::vector<pxz_image_desc> out(descs, descs + n_images);
	for (uint32_t i = 0; i < n_images; ++i) {
		if ((rc = scaled_check_shift(h, "image", i, scale_log2[i], p.block_w, p.block_h)) != PXZ_OK) return rc;
		out[i].width = scaled_extent(descs[i].width, scale_log2[i]);
		out[i].height = scaled_extent(descs[i].height, scale_log2[i]);
		if ((uint64_t)out[i].pitch_bytes < (uint64_t)out[i].width * channels) return fail(h, PXZ_ERR_INVALID_ARG, "image %u: pitch smaller than a row", i);
	}
	uint64_t file_bytes = 0;
	if ((rc = check_file_headers(h, files, lens, descs, n_images, channels, p, "batch", &file_bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	// device side: the files back to back behind their offsets; the scaled images tightly packed
	std::vector<pxz_image_desc> packed(out);
	const uint64_t img_bytes = pack_owners(&packed, channels);
	std::vector<pxz_image_desc> dev(descs, descs + n_images);  // the files' geometry, the packed images' places
	for (uint32_t i = 0; i < n_images; ++i) {
		dev[i].pitch_bytes = packed[i].pitch_bytes;
		dev[i].offset_bytes = packed[i].offset_bytes;
	}
	const uint32_t n_tiles = varied_n_tiles(images);
	const uint64_t slot = (uint64_t)p.block_w * p.block_h * channels;
	const uint64_t flags_at = TileSet::bytes(n_tiles, slot);
	SentFiles sent;
	if ((rc = send_files(h, h->varied_files, sent_bytes(n_images, file_bytes), files, lens, n_images, file_bytes, img_bytes, &sent)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->varied_out, flags_at + 8ull * n_images)) != PXZ_OK) return rc;
	if ((rc = ensure(h, h->varied_in, img_bytes)) != PXZ_OK) return rc;
	uint8_t *d_out = (uint8_t *)h->varied_out.ptr, *d_img = (uint8_t *)h->varied_in.ptr;
	const TileSet m(d_out, n_tiles);
	PXZ_HIP(h, hipMemsetAsync(m.slots, 0, (size_t)n_tiles * slot, h->stream));
	PXZ_HIP(h, hipMemsetAsync(d_img, 0, img_bytes, h->stream));  // (the place of a tile that cannot be expanded stays zero)
	uint32_t *d_flags = (uint32_t *)(d_out + flags_at);
	if ((rc = pxz_decode_varied_frames_device(h, dev.data(), n_images, channels, &p, sent.d_files, sent.d_offsets, m.value, m.w, m.h, m.slots,
	                                          d_flags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_expand_varied_scaled_frames_device(h, dev.data(), n_images, channels, &p, scale_log2, m.w, m.h, m.slots, d_img,
	                                                 d_flags + n_images)) != PXZ_OK)
		return rc;
	std::vector<uint32_t> flags(2u * (size_t)n_images);
	PXZ_HIP(h, hipStreamSynchronize(h->stream));  // the files have left the staging buffer
	PXZ_HIP(h, hipMemcpyAsync(sent.stage.data(), d_img, img_bytes, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(flags.data(), d_flags, flags.size() * 4u, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	uint32_t first_flags = 0;
	const uint32_t first_bad = copy_out_owners(out.data(), packed.data(), n_images, channels, sent.stage.data(), out_base, flags.data(), image_flags,
	                                           &first_flags);
	if (first_bad != n_images)
		return fail(h, PXZ_ERR_INVALID_ARG, "image %u: malformed .pixlzr file or record (flags %u); the other images are complete", first_bad,
		            first_flags);
	return PXZ_OK;
}

int pxz_decode_windows_files_scaled(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs, uint32_t n_images,
                                    const pxz_window *windows, uint32_t n_windows, uint32_t channels, const pxz_params *params,
                                    const uint32_t *scale_log2, uint8_t *out_base, uint64_t out_bytes, uint32_t *window_flags)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!files || !lens || !params || !out_base || !scale_log2) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	const pxz_params p = decode_side_params(params, true);
	int rc = varied_check_params(h, channels, &p);
	if (rc != PXZ_OK) return rc;
	std::vector<pxz::WindowEntry> entries;
	if ((rc = window_plan(h, descs, n_images, windows, n_windows, p.block_w, p.block_h, 0, &entries, nullptr, nullptr)) != PXZ_OK) return rc;
	std::vector<pxz_window> out(windows, windows + n_windows);  // the scaled crops at the caller's places
	for (uint32_t k = 0; k < n_windows; ++k) {
		const pxz_window &g = windows[k];
		const uint32_t sh = scale_log2[k];
		if ((rc = scaled_check_shift(h, "window", k, sh, p.block_w, p.block_h)) != PXZ_OK) return rc;
		if ((rc = scaled_check_window(h, k, g, entries[k].img_w, entries[k].img_h, sh)) != PXZ_OK) return rc;
		out[k].width = scaled_extent(g.x + g.width, sh) - (g.x >> sh);
		out[k].height = scaled_extent(g.y + g.height, sh) - (g.y >> sh);
		if ((uint64_t)g.pitch_bytes < (uint64_t)out[k].width * channels) return fail(h, PXZ_ERR_INVALID_ARG, "window %u: pitch smaller than a row", k);
		if (g.offset_bytes > out_bytes ||
		    (uint64_t)(out[k].height - 1u) * g.pitch_bytes + (uint64_t)out[k].width * channels > out_bytes - g.offset_bytes)
			return fail(h, PXZ_ERR_BUFFER_TOO_SMALL, "window %u: its output ends behind the %llu bytes of the buffer", k, (unsigned long long)out_bytes);
	}
	uint64_t file_bytes = 0;
	if ((rc = check_file_headers(h, files, lens, descs, n_images, channels, p, "call", &file_bytes)) != PXZ_OK) return rc;
	PXZ_HIP(h, hipSetDevice(h->device));
	// device side, one buffer, as pxz_decode_windows_files: files | covered tiles | the scaled crops tightly packed, the flags
	std::vector<pxz_window> packed(out);
	const uint64_t crop_bytes = pack_owners(&packed, channels);
	std::vector<pxz_window> dev(windows, windows + n_windows);  // the full-resolution rectangles, the packed crops' places
	for (uint32_t k = 0; k < n_windows; ++k) {
		dev[k].pitch_bytes = packed[k].pitch_bytes;
		dev[k].offset_bytes = packed[k].offset_bytes;
	}
	const uint32_t n_tiles = window_n_tiles(entries);
	const uint64_t slot = (uint64_t)p.block_w * p.block_h * channels;
	const uint64_t tiles_at = up256(sent_bytes(n_images, file_bytes)), crops_at = tiles_at + up256(TileSet::bytes(n_tiles, slot));
	const uint64_t flags_at = crops_at + crop_bytes, down_bytes = crop_bytes + 8ull * n_windows;
	SentFiles sent;
	if ((rc = send_files(h, h->window_host, flags_at + 8ull * n_windows, files, lens, n_images, file_bytes, down_bytes, &sent)) != PXZ_OK) return rc;
	uint8_t *d = (uint8_t *)h->window_host.ptr;
	PXZ_HIP(h, hipMemsetAsync(d + crops_at, 0, down_bytes, h->stream));  // (the place of a tile that cannot be expanded stays zero)
	const TileSet m(d + tiles_at, n_tiles);
	uint32_t *d_flags = (uint32_t *)(d + flags_at);
	if ((rc = pxz_decode_windows_device(h, descs, n_images, dev.data(), n_windows, channels, &p, sent.d_files, sent.d_offsets, m.value, m.w, m.h, m.slots,
	                                    d_flags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_expand_windows_scaled_device(h, descs, n_images, dev.data(), n_windows, channels, &p, scale_log2, m.w, m.h, m.slots, d + crops_at,
	                                           d_flags + n_windows)) != PXZ_OK)
		return rc;
	PXZ_HIP(h, hipStreamSynchronize(h->stream));  // the files have left the staging buffer
	PXZ_HIP(h, hipMemcpyAsync(sent.stage.data(), d + crops_at, down_bytes, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	const uint32_t *flags = reinterpret_cast<const uint32_t *>(sent.stage.data() + crop_bytes);
	uint32_t first_flags = 0;
	const uint32_t first_bad = copy_out_owners(out.data(), packed.data(), n_windows, channels, sent.stage.data(), out_base, flags, window_flags,
	                                           &first_flags);
	if (first_bad != n_windows)
		return fail(h, PXZ_ERR_INVALID_ARG, "window %u: malformed .pixlzr file or record in what it reads of image %u (flags %u); the other windows are complete",
		            first_bad, windows[first_bad].image, first_flags);
	return PXZ_OK;
}

// ---- patch: host files and host rectangles of new pixels in, host files out.  Composition only: one upload (the files whole, the
// patches behind them), reader of the windows, patch in place, splice, and what comes down: the offsets and flags, then the files.
int pxz_patch_windows_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images, const pxz_window *windows,
                            uint32_t n_windows, const uint8_t *const *patches, const pxz_params *params, uint32_t expand_filter, uint8_t *out,
                            uint64_t out_capacity, uint64_t *file_offsets)
{
	if (!h) return PXZ_ERR_INVALID_ARG;
	if (!files || !lens || !params || !file_offsets || !patches) return fail(h, PXZ_ERR_INVALID_ARG, "null pointer");
	if (n_images == 0) return fail(h, PXZ_ERR_INVALID_ARG, "empty image batch");
	int rc = check_params(h, params);
	if (rc != PXZ_OK) return rc;
	if (expand_filter > 4) return fail(h, PXZ_ERR_INVALID_ARG, "expand_filter must be 0..4, got %u", expand_filter);
	FileScan scan;
	if ((rc = scan_files(h, files, lens, n_images, &scan)) != PXZ_OK) return rc;
	const uint32_t ch = scan.channels;
	if (scan.block_w != params->block_w || scan.block_h != params->block_h)
		return fail(h, PXZ_ERR_INVALID_ARG, "the files hold %ux%u blocks, params ask for %ux%u: a patch keeps the block size", scan.block_w, scan.block_h,
		            params->block_w, params->block_h);
	if ((rc = reshrink_check_block(h, params->mode, params->block_w, params->block_h, 0u, 1u)) != PXZ_OK) return rc;
	std::vector<pxz::WindowEntry> entries;
	if ((rc = patch_plan(h, scan.descs.data(), n_images, windows, n_windows, params->block_w, params->block_h, ch, &entries, nullptr, nullptr)) != PXZ_OK)
		return rc;
	for (uint32_t k = 0; k < n_windows; ++k)
		if (!patches[k]) return fail(h, PXZ_ERR_INVALID_ARG, "window %u: null patch", k);
	PXZ_HIP(h, hipSetDevice(h->device));

	// device side, one buffer: the files back to back behind their offsets | the patches tightly packed | the covered tiles | both
	// flag arrays, the new files' offsets | the new files, at most the old bytes and every covered record at its largest
	std::vector<pxz_window> dev(windows, windows + n_windows);
	const uint64_t patch_bytes = pack_owners(&dev, ch);
	const uint32_t n_tiles = window_n_tiles(entries);
	const uint64_t slot = (uint64_t)params->block_w * params->block_h * ch;
	const uint64_t offs_bytes = 8ull * ((uint64_t)n_images + 1u);
	const uint64_t patches_at = up256(offs_bytes + scan.file_bytes + 16u), tiles_at = patches_at + up256(patch_bytes);
	const uint64_t flags_at = tiles_at + up256(TileSet::bytes(n_tiles, slot)), new_offs_at = flags_at + up256(8ull * n_windows);
	const uint64_t new_files_at = new_offs_at + up256(offs_bytes);
	const uint64_t room = scan.file_bytes + (uint64_t)n_tiles * (13u + pxz_qoi_bound(params->block_w, params->block_h, ch));
	if ((rc = ensure(h, h->patch_host, new_files_at + room)) != PXZ_OK) return rc;
	uint8_t *d = (uint8_t *)h->patch_host.ptr;
	std::vector<uint8_t> stage((size_t)(patches_at + patch_bytes));
	uint64_t *offs = reinterpret_cast<uint64_t *>(stage.data());
	offs[0] = 0;
	for (uint32_t i = 0; i < n_images; ++i) {
		std::memcpy(stage.data() + offs_bytes + offs[i], files[i], lens[i]);
		offs[i + 1] = offs[i] + lens[i];
	}
	for (uint32_t k = 0; k < n_windows; ++k) {
		const size_t row = (size_t)windows[k].width * ch;
		for (uint32_t y = 0; y < windows[k].height; ++y)
			std::memcpy(stage.data() + patches_at + dev[k].offset_bytes + (size_t)y * row, patches[k] + (size_t)y * windows[k].pitch_bytes, row);
	}
	PXZ_HIP(h, hipMemcpyAsync(d, stage.data(), stage.size(), hipMemcpyHostToDevice, h->stream));
	const uint64_t *d_offsets = (const uint64_t *)d;
	const uint8_t *d_files = d + offs_bytes;
	const TileSet m(d + tiles_at, n_tiles);
	uint32_t *d_flags = (uint32_t *)(d + flags_at);
	uint64_t *d_new_offs = (uint64_t *)(d + new_offs_at);
	PXZ_HIP(h, hipMemsetAsync(m.value, 0, TileSet::meta_bytes(n_tiles), h->stream));  // (a tile the reader cannot reach keeps size 0 and is flagged)
	pxz_params pin = *params;  // (the reader takes the block size alone)
	if ((rc = pxz_decode_windows_device(h, scan.descs.data(), n_images, dev.data(), n_windows, ch, &pin, d_files, d_offsets, m.value, m.w, m.h, m.slots,
	                                    d_flags)) != PXZ_OK)
		return rc;
	if ((rc = pxz_patch_windows_device(h, scan.descs.data(), n_images, dev.data(), n_windows, ch, params, expand_filter, d + patches_at, m.w, m.h, m.slots,
	                                   m.value, m.w, m.h, m.slots, d_flags + n_windows)) != PXZ_OK)
		return rc;
	if ((rc = pxz_splice_windows_device(h, scan.descs.data(), n_images, dev.data(), n_windows, ch, params, d_files, d_offsets, m.value, m.w, m.h, m.slots,
	                                    d_flags, d_flags + n_windows, d + new_files_at, room, d_new_offs, nullptr)) != PXZ_OK)
		return rc;
	// all or nothing: the flags and the offsets first
	std::vector<uint32_t> flags(2u * (size_t)n_windows);
	std::vector<uint64_t> got((size_t)n_images + 1u);
	PXZ_HIP(h, hipMemcpyAsync(flags.data(), d_flags, flags.size() * 4u, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipMemcpyAsync(got.data(), d_new_offs, got.size() * 8u, hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	for (uint32_t k = 0; k < n_windows; ++k)
		if (flags[k] | flags[n_windows + k])
			return fail(h, PXZ_ERR_INVALID_ARG, "window %u: malformed .pixlzr file or record in what it reads of image %u (flags %u); nothing was written", k,
			            windows[k].image, flags[k] | flags[n_windows + k]);
	if (got[n_images] > room) return fail(h, PXZ_ERR_INTERNAL, "the spliced files exceed their bound");
	std::memcpy(file_offsets, got.data(), got.size() * 8u);
	if (!out || out_capacity < got[n_images])
		return fail(h, PXZ_ERR_BUFFER_TOO_SMALL, "the patched files need %llu bytes, the buffer has %llu", (unsigned long long)got[n_images],
		            (unsigned long long)(out ? out_capacity : 0));
	PXZ_HIP(h, hipMemcpyAsync(out, d + new_files_at, got[n_images], hipMemcpyDeviceToHost, h->stream));
	PXZ_HIP(h, hipStreamSynchronize(h->stream));
	return PXZ_OK;
}

}  // extern "C"
