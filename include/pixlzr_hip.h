/*
 * pixlzr_hip.h — C ABI of libpixlzr_hip.so, the MI355X (gfx950) implementation of
 * the pixlzr encode hot path: per-tile level-of-detail detection + power-of-two
 * down-sampling over the regular tile grid, and the .pixlzr bitstream writer.
 *
 * The reference (guiga-zalu/pixlzr-rust 0.3.1) has no FFI of its own; these are
 * the entry points a Rust `extern "C"` block inside `Pixlzr::shrink_by` /
 * `Pixlzr::shrink_directionally` / `Pixlzr::encode_to_vec` would bind (see
 * INTEGRATION.md for that binding).  Each declaration cites the reference
 * interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *  - every function returns PXZ_OK (0) or a negative pxz_status; nothing aborts.
 *    (The reference panics on the same conditions: unwrap() inside the path.)
 *  - plain pointers and sizes only; "device" pointers are HIP device addresses
 *    on the handle's GPU.  *_device entry points are asynchronous on the
 *    handle's stream (pxz_set_stream); host-buffer entry points synchronise.
 *  - a handle is bound to one GPU and may be used by one thread at a time;
 *    distinct handles are independent (mirrors: concurrent calls on different
 *    `Pixlzr` objects are legal, src/data_types/pixlzr.rs:17-25).
 *  - tile order is the reference's: row-major, tile = ty*cols + tx
 *    (src/data_types/iter.rs:64-76); grid = ceil(w/bw) x ceil(h/bh).
 *  - there is no CPU fallback: without a gfx950 device pxz_create fails.
 */
#ifndef PIXLZR_HIP_H
#define PIXLZR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pxz_handle pxz_handle;

typedef enum pxz_status {
	PXZ_OK = 0,
	PXZ_ERR_INVALID_ARG = -1,   /* null pointer, channels not 3|4, zero sizes, non-finite factor */
	PXZ_ERR_NO_DEVICE = -2,     /* no HIP device / not gfx950 */
	PXZ_ERR_HIP = -3,           /* a HIP runtime call failed; see pxz_last_error */
	PXZ_ERR_TILE_TOO_SMALL = -4,/* directional mode with a tile narrower/lower than 2 px:
	                               the reference underflows usize and panics (operations.rs:220-221) */
	PXZ_ERR_UNSUPPORTED = -5,   /* a tile of 2^20 pixels or more (smaller tiles whose image exceeds the 160 KB of LDS run from an
	                             * HBM-resident image, slowly), an image side above 2^24, tree blocks above 128 px */
	PXZ_ERR_NOMEM = -6,
	PXZ_ERR_BUFFER_TOO_SMALL = -7,
	PXZ_ERR_INTERNAL = -8       /* a device-side consistency check failed (never expected; see pxz_last_error) */
} pxz_status;

/* FilterType, repr(u8): src/data_types/mod.rs:10-30 */
typedef enum pxz_filter {
	PXZ_FILTER_NEAREST = 0,
	PXZ_FILTER_TRIANGLE = 1,    /* down-scales with fir Hamming (data_types/mod.rs:93-95) */
	PXZ_FILTER_CATMULLROM = 2,
	PXZ_FILTER_GAUSSIAN = 3,
	PXZ_FILTER_LANCZOS3 = 4
} pxz_filter;

/* which caller of the hot path is replaced */
typedef enum pxz_mode {
	PXZ_MODE_SHRINK_BY = 0,            /* Pixlzr::shrink_by, pixlzr.rs:155-185 (Oklab MAD, isotropic) */
	PXZ_MODE_SHRINK_DIRECTIONALLY = 1  /* Pixlzr::shrink_directionally, pixlzr.rs:187-205 */
} pxz_mode;

/* ---- library / handle ------------------------------------------------- */
const char *pxz_version(void);
/* number of usable gfx950 devices (0 if none / no HIP runtime) */
int pxz_device_count(void);
int pxz_create(int device_id, pxz_handle **out);
void pxz_destroy(pxz_handle *h);
/* text of the last error on this handle ("" if none) */
const char *pxz_last_error(const pxz_handle *h);
/* run device entry points on the caller's hipStream_t (NULL = default stream) */
int pxz_set_stream(pxz_handle *h, void *hip_stream);
int pxz_synchronize(pxz_handle *h);

/* ---- geometry --------------------------------------------------------- */
/* ImageBlockIterator::new grid math, src/data_types/iter.rs:38-41 / src/split.rs:45-46 */
int pxz_grid(uint32_t width, uint32_t height, uint32_t block_w, uint32_t block_h,
             uint32_t *cols, uint32_t *rows);

/* A batch of equally sized, pitch-linear, interleaved 8-bit frames
 * (what `image::DynamicImage::ImageRgba8|ImageRgb8` holds, src/split.rs:10-27). */
typedef struct pxz_frames {
	uint32_t width, height;
	uint32_t channels;          /* 3 (RGB8) or 4 (RGBA8) */
	uint32_t pitch_bytes;       /* >= width*channels */
	uint32_t n_frames;          /* >= 1 */
	uint32_t reserved;          /* 0 */
	uint64_t frame_stride_bytes;/* distance between frames (ignored when n_frames==1) */
} pxz_frames;

typedef struct pxz_params {
	uint32_t block_w, block_h;  /* CLI -b / --block-height, src/bin/main.rs:19-24 */
	uint32_t mode;              /* pxz_mode */
	uint32_t filter;            /* pxz_filter (filter_downscale) */
	float factor;               /* shrinking factor, src/bin/main.rs:26-29 */
	uint32_t reserved;          /* 0, or PXZ_HINT_* bits */
} pxz_params;

/* Performance hints (pxz_params.reserved); results never depend on them.
 * PXZ_HINT_TRANSPARENCY: many tiles of these RGBA frames carry alpha < 255.  32x32 tiles with transparency are
 * then resampled by a dedicated kernel (four LDS planes, premultiplied matrix-core convolution) instead of the
 * generic one, at the price of one more launch per call.  pxz_shrink_image samples the image and sets it itself;
 * without the hint a handle switches to that kernel by itself once a finished launch has reported >= 2048 such
 * tiles (and back when a launch reports fewer). */
#define PXZ_HINT_TRANSPARENCY 1u

/* ---- the hot path ----------------------------------------------------- */

/* Pixlzr::from_image (pixlzr_image.rs:6-22) + shrink_by | shrink_directionally
 * (pixlzr.rs:155-205) for ALL tiles of one host-resident image:
 * get_block_variance[_directionally] (operations.rs:26-126,192-259) ->
 * reduce_image_section (operations.rs:140-156) -> PixlzrBlock::resize
 * (block.rs:273-334, fast_image_resize convolution / nearest).
 * Outputs (caller-allocated, tile order):
 *   block_value[t]  Some(value) of the shrunk tile = hypot(v0,v1) (operations.rs:154)
 *   out_w/out_h[t]  reduced tile dimensions
 *   out_pixels      fixed slots of block_w*block_h*channels bytes per tile, of
 *                   which out_w*out_h*channels are valid (tightly packed rows);
 *                   the rest of a slot is unspecified and may be written (shrink_by
 *                   leaves the tile's own pixels there on its way).
 *                   May be NULL: LOD + dimensions only. */
int pxz_shrink_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height,
                     uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h,
                     uint32_t mode, uint32_t filter, float factor,
                     float *block_value, uint32_t *out_w, uint32_t *out_h, uint8_t *out_pixels);

/* The same call with the pixels as ONE tightly packed stream (tile order, each tile out_w*out_h*channels
 * bytes) instead of fixed slots: what the reference keeps per block (PixlzrBlock's pixel Vec, block.rs) and
 * a fraction of the slot array over PCIe.  Two steps so that the caller allocates exactly what comes back:
 * pxz_shrink_image_packed runs the path, returns values and dimensions and *packed_len; the stream stays in
 * the handle until pxz_fetch_packed copies it out (capacity >= packed_len) or the next call on the handle.
 * Tile t starts at the sum of out_w*out_h*channels over the tiles before it. */
int pxz_shrink_image_packed(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height,
                            uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h,
                            uint32_t mode, uint32_t filter, float factor,
                            float *block_value, uint32_t *out_w, uint32_t *out_h, uint64_t *packed_len);
int pxz_fetch_packed(pxz_handle *h, uint8_t *dst, uint64_t capacity);

/* Releases every scratch buffer the handle has grown (inputs, tile slots, worklists, the rings of the pipelined list
 * calls, the writer's scratch ...) after finishing what is queued on its stream; tables stay.  The next call allocates
 * what it needs again.  Nothing in the reference corresponds to it (its Vecs are freed when a Pixlzr is dropped). */
int pxz_trim(pxz_handle *h);

/* pxz_shrink_image / pxz_shrink_image_packed over a LIST of equally sized host images (a folder of frames, what
 * src/bin/whole-folder.rs:69-117 loops over): outputs as for the single-image calls, one set of caller-allocated arrays
 * per image (out_pixels may be NULL, or hold NULLs, for detector + dimensions only; packed[k] needs packed_capacity
 * bytes -- width*height*channels always suffices -- and packed_len[k] receives the stream's length).  The images go
 * through a three-stage pipeline on the device -- upload of image k+1, kernels of image k, download of image k-1 at the
 * same time -- so that a list costs about one PCIe direction per image rather than the sum of both.  Synchronous.
 * On an error the arrays of the images that were finished before it are complete, those of later images are untouched
 * or partly written, and packed_len[k] is written for every image that was downloaded even when the call then returns
 * PXZ_ERR_BUFFER_TOO_SMALL (it names the capacity that would have sufficed).  The three sets of device buffers of
 * the pipeline stay with the handle for the next list (about 1.2 GB for 8K RGBA): pxz_trim releases them. */
int pxz_shrink_images(pxz_handle *h, const uint8_t *const *pixels, uint32_t n_images, uint32_t width, uint32_t height,
                      uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode,
                      uint32_t filter, float factor, float *const *block_value, uint32_t *const *out_w,
                      uint32_t *const *out_h, uint8_t *const *out_pixels);
int pxz_shrink_images_packed(pxz_handle *h, const uint8_t *const *pixels, uint32_t n_images, uint32_t width, uint32_t height,
                             uint32_t channels, uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode,
                             uint32_t filter, float factor, float *const *block_value, uint32_t *const *out_w,
                             uint32_t *const *out_h, uint8_t *const *packed, uint64_t packed_capacity, uint64_t *packed_len);

/* Same over a batch of device-resident frames: the measured path (frames come
 * from a GPU decoder / stay in HBM).  All pointers are device pointers; outputs
 * are frame-major: index = frame*tiles + tile; out_pixels slot stride as above.
 * Asynchronous on the handle's stream; one kernel launch for the whole batch. */
int pxz_shrink_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                             const uint8_t *d_pixels, float *d_block_value, uint32_t *d_out_w,
                             uint32_t *d_out_h, uint8_t *d_out_pixels);

/* ---- factor ladder: one batch at several factors ------------------------- */
#define PXZ_LADDER_MAX_RUNGS 16u

/* Pixlzr::shrink_by | shrink_directionally of the same frames at n_factors factors (one "rung" per factor): what
 * src/bin/whole-folder.rs:69-117 sweeps with k = i/20, in one call.  Rung r is bit-identical to pxz_shrink_frames_device
 * with params->factor = factors[r]: values (as bits), out_w, out_h, and the valid out_w*out_h*channels bytes of every slot.
 * params->factor is ignored; factors is a HOST array (1 <= n_factors <= PXZ_LADDER_MAX_RUNGS, each finite; any order,
 * repeats allowed).  Outputs are rung-major: index = (r * n_frames + f) * tiles + t, slots of block_w*block_h*channels
 * bytes as before (64-bit offsets), so the K*N rung sets are a batch of K*N frames to pxz_encode_frames_device.
 * d_out_pixels may be NULL (values + dims).  Asynchronous on the handle's stream.
 * Errors: PXZ_ERR_INVALID_ARG for a null factors, n_factors 0 or above the maximum, a non-finite factor; and every
 * error pxz_shrink_frames_device returns for the same frames and params (e.g. PXZ_ERR_TILE_TOO_SMALL).
 * shrink_by runs the detector ONCE (its result does not depend on the factor: x * factor * BASE_FACTOR, pixlzr.rs:160-162)
 * and then one kernel that stages every tile once and resamples it once per distinct level among the rungs -- for every
 * tile geometry whose LDS image fits (16x16, 32x32, 64x64 and most others; RGB and RGBA, any pitch).  Larger tiles, and
 * shrink_directionally (whose detector is a few integer operations fused into the shrink kernels), run one single-factor
 * call per rung: correct, with no amortisation. */
int pxz_shrink_ladder_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                                    const float *factors, uint32_t n_factors, const uint8_t *d_pixels,
                                    float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels);

/* The same for one host-resident image (as pxz_shrink_image: uploads, runs, downloads; synchronous).  Arrays rung-major:
 * n_factors * tiles values / dims, n_factors * tiles slots. */
int pxz_shrink_image_ladder(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                            uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter,
                            const float *factors, uint32_t n_factors, float *block_value, uint32_t *out_w,
                            uint32_t *out_h, uint8_t *out_pixels);

/* ---- batches of differently sized images ------------------------------------ */

/* One image of a varied batch: an interleaved 8-bit image (RGB8 or RGBA8, the batch's `channels`) at offset_bytes from the
 * batch's base pointer (any alignment).  What src/bin/whole-folder.rs:69-117 holds for each file of a folder. */
typedef struct pxz_image_desc {
	uint32_t width, height;
	uint32_t pitch_bytes;   /* >= width*channels */
	uint32_t reserved;      /* 0 */
	uint64_t offset_bytes;  /* image start relative to the batch's base pointer (any alignment) */
} pxz_image_desc;

/* Layout of a varied batch's per-tile outputs (host only: no handle, no GPU, like pxz_grid).  Image i has the grid
 * pxz_grid(width_i, height_i, block_w, block_h); its tile t (reference row-major order, iter.rs:64-76) lives at output index
 * tile_offsets[i] + t, and tile_offsets[n_images] is the batch's tile count.  Slots stay block_w*block_h*channels bytes,
 * addressed with 64-bit offsets.  PXZ_ERR_INVALID_ARG for a null pointer, n_images 0, a zero block side, a zero image side
 * or a non-zero reserved field; PXZ_ERR_UNSUPPORTED for an image side above 2^24 or more than 2^32-1 tiles in all.  The
 * error names no image (there is no handle to carry the text); the device entry points below do. */
int pxz_varied_layout(const pxz_image_desc *descs, uint32_t n_images, uint32_t block_w, uint32_t block_h,
                      uint64_t *tile_offsets);

/* Pixlzr::from_image + shrink_by | shrink_directionally (pixlzr.rs:155-205) of EVERY image of a batch of differently sized
 * device-resident images, in one call whose number of kernel launches does not depend on n_images.  All images share
 * `channels` (3 or 4) and params (block size, mode, filter, factor; params->reserved hints are ignored).  descs is a HOST
 * array; image i starts at d_base + descs[i].offset_bytes.  Outputs in the pxz_varied_layout order: d_block_value, d_out_w,
 * d_out_h per tile, d_out_pixels slots of block_w*block_h*channels bytes (may be NULL: values and sizes only).  Each image's
 * results equal pxz_shrink_frames_device on that image alone, bit for bit (value bits, sizes, the valid slot bytes).
 * Asynchronous on the handle's stream.
 * Validation runs on the host before anything is launched, for every image, and names the failing image's index in
 * pxz_last_error; on an error nothing is written.  The rules are pxz_shrink_frames_device's: PXZ_ERR_INVALID_ARG for null
 * pointers, n_images 0, channels not 3|4, zero sides, a pitch below one row, a non-zero reserved field, a bad mode / filter /
 * non-finite factor; PXZ_ERR_UNSUPPORTED for a side above 2^24 or more than 2^32-1 tiles in all; PXZ_ERR_TILE_TOO_SMALL for
 * shrink_directionally with a tile (edge tiles included) narrower or lower than 2 px.
 * Limit of this path: every tile is staged whole in LDS, so block_w*block_h*channels must not exceed 65536 bytes (128x128
 * RGBA, 147x147 RGB); larger blocks give PXZ_ERR_UNSUPPORTED (the single-geometry call runs them from HBM).
 * A varied call reads and writes none of the state the single-geometry fast paths keep in the handle (kernel-selection
 * statistics, worklist counters, the per-tile detector scratch with its "copied" flags). */
int pxz_shrink_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, const uint8_t *d_base, float *d_block_value, uint32_t *d_out_w,
                                    uint32_t *d_out_h, uint8_t *d_out_pixels);

/* Pixlzr::encode_to_vec (src/encoding/mod.rs:40-89) of every image of a varied batch, on the device: the tiles as
 * pxz_shrink_varied_frames_device leaves them become one complete .pixlzr file per image, back to back in d_out; file i is
 * [d_file_offsets[i], d_file_offsets[i+1]) (n_images + 1 u64 offsets).  Only width and height of the descriptors are read.
 * File i equals pxz_encode_frames_device of image i alone.  If out_capacity is too small the files are truncated but the
 * offsets are still exact (retry with d_file_offsets[n_images] bytes).  Asynchronous on the handle's stream. */
int pxz_encode_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, uint32_t filter_byte, const float *d_block_value,
                                    const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_out,
                                    uint64_t out_capacity, uint64_t *d_file_offsets);

/* Host images in, .pixlzr files out, synchronously: what a Rust loop over a folder (whole-folder.rs:69-117) calls once
 * instead of once per file.  pixels[i] is image i (descs[i].offset_bytes is ignored).  file_offsets (n_images + 1) are
 * always written; the files go to out when out_capacity >= file_offsets[n_images], else the call returns
 * PXZ_ERR_BUFFER_TOO_SMALL and writes nothing to out (retry with file_offsets[n_images] bytes; out may be NULL for that
 * size query).  Errors and limits as pxz_shrink_varied_frames_device. */
int pxz_encode_varied_images(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                             uint32_t channels, const pxz_params *params, uint32_t filter_byte, uint8_t *out,
                             uint64_t out_capacity, uint64_t *file_offsets);

/* Varied ladder: the sweep of src/bin/whole-folder.rs:69-117 -- a folder of differently sized images x several factors -- in
 * ONE launch, whatever n_images and n_factors are.  Every tile is staged and measured once (the detector's raw result does
 * not depend on the factor, in either mode); each rung only decides its levels, and a tile is resampled once per distinct
 * pair of levels among its rungs.  params->factor is ignored; factors is a HOST array (1 <= n_factors <=
 * PXZ_VARIED_LADDER_MAX_RUNGS, each finite; any order, repeats allowed).  Outputs are rung-major: with tile_offsets and
 * tiles = tile_offsets[n_images] from pxz_varied_layout, rung r of tile t of image i is index r*tiles + tile_offsets[i] + t
 * of d_block_value, d_out_w, d_out_h and of the slots of d_out_pixels (block_w*block_h*channels bytes each, 64-bit offsets;
 * may be NULL: values and sizes only).  That is the layout of a varied batch of n_factors*n_images images whose descriptors
 * are descs repeated n_factors times, so pxz_encode_varied_frames_device and pxz_distortion_varied_frames_device take the
 * result as it is.  Rung r equals pxz_shrink_varied_frames_device with factor = factors[r] bit for bit (value bits, sizes,
 * the valid bytes of every slot).  Asynchronous on the handle's stream.
 * Validation runs on the host before anything is launched; on an error nothing is written.  Codes and "image i" texts are
 * pxz_shrink_varied_frames_device's, its limit (block_w*block_h*channels <= 65536 bytes) included; PXZ_ERR_INVALID_ARG for
 * factors null, n_factors 0 or above the maximum, or a non-finite factor; PXZ_ERR_UNSUPPORTED when n_factors * tiles exceeds
 * 2^32-1.  The call reads and writes none of the state the single-geometry fast paths keep in the handle; pxz_trim gives
 * back what it grew.  PXZ_LADDER_MAX_RUNGS and the single-geometry ladder are not affected. */
#define PXZ_VARIED_LADDER_MAX_RUNGS 32u   /* the reference's sweep of 20 fits */
int pxz_shrink_varied_ladder_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                           const pxz_params *params, const float *factors, uint32_t n_factors,
                                           const uint8_t *d_base, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                           uint8_t *d_out_pixels);

/* The colour conversion inside get_block_variance, per pixel (operations.rs:56-59: Srgba<u8>::into_linear()
 * .into_color::<Oklaba<f32>>(), palette 0.7.6 + the platform's cbrtf): d_laba[4i..4i+3] = {l, a, b, alpha} of
 * RGBA pixel i.  The same device function the Oklab detector kernels call -- exposed so that its bits can be
 * checked for every one of the 2^24 colours.  Device pointers (pixels 4-byte, output 16-byte aligned); async. */
int pxz_oklab_pixels_device(pxz_handle *h, const uint8_t *d_rgba, uint32_t n_pixels, float *d_laba);

/* Detector only: get_block_variance_directionally (operations.rs:192-259) ->
 * lod0 = hz, lod1 = vr (raw, before `* factor`); get_block_variance with the
 * shrink_by closures (operations.rs:26-126, pixlzr.rs:160-162) -> lod0 = lod1 =
 * value (params->factor applied).  Device pointers, frame-major. */
int pxz_lod_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                          const uint8_t *d_pixels, float *d_lod0, float *d_lod1);

/* ---- decode side ---------------------------------------- */

/* Pixlzr::expand (pixlzr.rs:77-122) + Pixlzr::to_image (pixlzr_image.rs:24-74) on device-resident
 * tiles: every stored tile (tile_w x tile_h pixels, tightly packed, in a slot of block_w*block_h*channels
 * bytes -- the layout pxz_shrink_frames_device leaves and decode_block (encoding/mod.rs:202-242) yields)
 * is resized back to its full size by PixlzrBlock::resize (block.rs:273-334: clone | ResizeAlg::Nearest |
 * SuperSampling(filter, 2), which is a plain convolution when nothing shrinks; Triangle means Bilinear here,
 * mod.rs:72-90) and written to its place in the frame.  `frames` describes the OUTPUT; params->block_w,
 * block_h and filter are used.  Tiles whose stored size is zero or exceeds their place are skipped and
 * flagged (pxz_decode_status).  Asynchronous on the handle's stream. */
int pxz_expand_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                             const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                             uint8_t *d_out_pixels);

/* Pixlzr::decode_from_vec (src/encoding/mod.rs:95-165) + decode_block (:202-242) + the `qoi` decoder it
 * calls, on the device: n_frames .pixlzr files, back to back in d_files (file f = [off[f], off[f+1])),
 * become the per-tile values, stored sizes and pixel slots (the layout pxz_expand_frames_device and
 * pxz_encode_frames_device use).  `frames` gives the geometry every file must carry (width, height,
 * channels; pitch fields unused), params block_w/block_h.  A malformed file or record is flagged
 * (pxz_decode_status) and its tiles get size 0x0.  Asynchronous on the handle's stream. */
int pxz_decode_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                             const uint8_t *d_files, const uint64_t *d_file_offsets, float *d_block_value,
                             uint32_t *d_tile_w, uint32_t *d_tile_h, uint8_t *d_slots);

/* The same for one host-resident file (Pixlzr::decode_from_vec, mod.rs:95-165).  The header fields are
 * always returned; with all four output pointers NULL the call stops there (size query: the grid is
 * pxz_grid(width, height, block_w, block_h), slots need block_w*block_h*channels bytes per tile).
 * PXZ_ERR_INVALID_ARG for a malformed file (the reference panics / returns the qoi error). */
int pxz_decode_file(pxz_handle *h, const uint8_t *file, size_t len, uint32_t *width, uint32_t *height,
                    uint32_t *block_w, uint32_t *block_h, uint32_t *channels, uint32_t *filter_byte,
                    float *block_value, uint32_t *tile_w, uint32_t *tile_h, uint8_t *slots);

/* Waits for the handle's stream; flags of the last decode-side call on this handle:
 * bit 0  pxz_expand_frames_device met a tile whose stored size is zero or exceeds its place,
 * bit 1  pxz_decode_frames_device met a malformed file or record.
 * After a varied call (below) the bits are the OR over the images of its batch. */
int pxz_decode_status(pxz_handle *h, uint32_t *flags);

/* The header fields of one host-resident .pixlzr file (host only: no handle, no GPU, like pxz_grid): what pxz_decode_file
 * returns when all its output pointers are NULL, with the same checks.  channels is the channel byte of the first record's
 * QOI header (decode_block, mod.rs:202-242).  PXZ_ERR_INVALID_ARG for a null pointer, a file shorter than its header, a
 * wrong magic or version, a zero image or block side, a file that ends inside its first record, a channel byte that is
 * neither 3 nor 4.  What a caller of the varied reader needs to fill its descriptors before anything is allocated. */
int pxz_file_header(const uint8_t *file, size_t len, uint32_t *width, uint32_t *height, uint32_t *block_w, uint32_t *block_h,
                    uint32_t *channels, uint32_t *filter_byte);

/* ---- decode side of batches of differently sized images ---------------------- */

/* Pixlzr::decode_from_vec (encoding/mod.rs:95-165) + decode_block (:202-242) of the n_images files of a varied batch, back
 * to back in d_files (file i = [d_file_offsets[i], d_file_offsets[i+1])), in one call whose number of kernel launches and
 * copies does not depend on n_images: the read half of src/bin/whole-folder.rs:155-163.  All files share `channels` (3 or 4)
 * and params->block_w / block_h (nothing else of params is used); of descs[i] only width and height are read (as by the
 * varied writer).  Outputs in the pxz_varied_layout order: d_block_value, d_tile_w, d_tile_h per tile, d_slots of
 * block_w*block_h*channels bytes.  Each image's results equal pxz_decode_frames_device on that file alone, bit for bit.
 * A file whose header does not carry descs[i]'s size and the batch's block size, or that is malformed anywhere, is flagged
 * and its unusable tiles get size 0x0 exactly as in the single-geometry call; the other images are not affected.
 * d_image_flags (n_images dwords, may be NULL) receives 0 or 2 per image; pxz_decode_status reports the OR over the batch.
 * Asynchronous on the handle's stream.  Descriptors are validated on the host before anything is launched, with the rules,
 * codes and "image i" texts of pxz_shrink_varied_frames_device; on such an error nothing is written.  No limit on the
 * block size beyond a slot of less than 4 GiB (nothing of a tile is staged). */
int pxz_decode_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, const uint8_t *d_files, const uint64_t *d_file_offsets,
                                    float *d_block_value, uint32_t *d_tile_w, uint32_t *d_tile_h, uint8_t *d_slots,
                                    uint32_t *d_image_flags);

/* Pixlzr::expand (pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) of every image of a varied batch: the stored tiles
 * (varied layout, as the call above or pxz_shrink_varied_frames_device leaves them) are resized back to their full sizes
 * with params->filter (what to_image(filter) takes) and image i is written at d_base + descs[i].offset_bytes with
 * descs[i].pitch_bytes between rows, any alignment.  Bytes of the buffer that belong to no image (row padding, gaps) are not
 * written.  Each image equals pxz_expand_frames_device on its tiles alone, byte for byte.  A tile whose stored size is zero
 * or exceeds its place is skipped (its pixels stay as they were) and flagged: d_image_flags (may be NULL) receives 0 or 1
 * per image, pxz_decode_status the OR.  Asynchronous; validation as above (here the pitch counts too).  Limit of this path:
 * block_w*block_h*channels <= 65536 bytes as on the encode side (PXZ_ERR_UNSUPPORTED beyond; the single-geometry call
 * runs larger tiles), so whatever the varied writer wrote the varied reader reads. */
int pxz_expand_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    const pxz_params *params, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                    const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_image_flags);

/* Host files in, host images out, synchronously: what a Rust loop over a folder (whole-folder.rs:155-163) calls once
 * instead of pxz_decode_file + pxz_expand_image per file.  files[i] / lens[i] is file i; image i is written at
 * out_base + descs[i].offset_bytes with descs[i].pitch_bytes between rows.  Every header is parsed on the host first
 * (pxz_file_header): a file whose size, block size or channels disagree with descs[i] and the batch is refused
 * (PXZ_ERR_INVALID_ARG, "image i" in pxz_last_error) and nothing is written.  Files that pass that check but are malformed
 * further in come back flagged -- image_flags[i] (may be NULL), bits as pxz_decode_status -- with the tiles that could not
 * be read left zero; the call then returns PXZ_ERR_INVALID_ARG naming the first such image, and every other image is
 * complete.  Errors and limits as pxz_expand_varied_frames_device. */
int pxz_decode_varied_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs,
                            uint32_t n_images, uint32_t channels, const pxz_params *params, uint8_t *out_base,
                            uint32_t *image_flags);

/* ---- re-shrink: .pixlzr tiles to .pixlzr tiles without the image --------------- */

/* The reference CLI's pix_to_pix (src/bin/main.rs:233-265: to_image(filter), from_image, shrink) on the stored tiles of a
 * varied batch, for a block size that stays the same: tile t of the rebuilt image is then exactly the expansion of stored
 * tile t, so every tile is expanded to its full size in LDS, measured, and resampled into its new slot by one kernel, and
 * nothing of image size is read, written or allocated.  Inputs d_tile_w, d_tile_h, d_slots and outputs d_block_value,
 * d_out_w, d_out_h, d_out_pixels are in the pxz_varied_layout order with slots of block_w*block_h*channels bytes: the
 * inputs are what pxz_decode_varied_frames_device or a varied shrink leaves.  Of descs[i] only width and height are read.
 * expand_filter is what to_image(filter) takes; params carries what the shrink takes (block size, mode, filter, factor).
 * For every image without a flagged tile the results equal, bit for bit (value bits, sizes, the valid bytes of every slot),
 * pxz_expand_varied_frames_device with expand_filter into a tightly packed image followed by
 * pxz_shrink_varied_frames_device with params on that image.
 * A tile whose stored size is zero or exceeds its place is flagged as by pxz_expand_varied_frames_device -- d_image_flags
 * (n_images dwords, may be NULL) receives 0 or 1 per image, pxz_decode_status reports bit 0 -- and gets d_out_w = d_out_h =
 * 0 and value bits 0; its slot is left as it was.  d_out_pixels may be NULL (values and sizes only).
 * In place: d_out_w, d_out_h and d_out_pixels may be d_tile_w, d_tile_h and d_slots themselves.  Tile t's inputs are read
 * only by the block that writes tile t's outputs, into LDS and before its first store.
 * Asynchronous on the handle's stream; the number of launches does not depend on n_images.  Validation runs on the host
 * before anything is launched, with the rules, codes and "image i" texts of pxz_shrink_varied_frames_device
 * (PXZ_ERR_TILE_TOO_SMALL included), and PXZ_ERR_INVALID_ARG for an expand_filter above 4; on an error nothing is written.
 * Limit of this path: a tile is expanded as one dword per pixel in two LDS planes, for RGB as for RGBA, so
 * block_w*block_h*4 must not exceed 65536 bytes (128x128); larger blocks give PXZ_ERR_UNSUPPORTED, and so does a block so
 * oblong (block_w + block_h above about 900) that the staged windows of both axes no longer fit beside the planes
 * (pxz_reshrink_lds_bytes says which).
 * The call reads and writes none of the state the single-geometry fast paths keep in the handle; pxz_trim gives back what it
 * grew. */
int pxz_reshrink_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                      const pxz_params *params, uint32_t expand_filter, const uint32_t *d_tile_w,
                                      const uint32_t *d_tile_h, const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w,
                                      uint32_t *d_out_h, uint8_t *d_out_pixels, uint32_t *d_image_flags);

/* LDS bytes of one block of the call above for blocks of block_w x block_h (host only: no handle, no GPU): what the entry
 * point holds against the CU's 160 KB before it launches, from the function the launch itself uses.  A value above
 * 163840 (0xffffffff beyond the documented limit) means PXZ_ERR_UNSUPPORTED.  PXZ_ERR_INVALID_ARG for a null pointer, a zero
 * side, a mode above 1 or a filter above 4. */
int pxz_reshrink_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t expand_filter, uint32_t *lds_bytes);

/* Re-tile: pix_to_pix with -b, a block size that CHANGES, on the stored tiles of a varied batch.  A tile of the rebuilt
 * image's new grid is put together, in LDS, from the parts of the stored tiles that cover it -- each part expanded with the
 * arithmetic of pxz_expand_varied_frames_device, or copied when its tile is stored at full size -- then measured and
 * resampled into its new slot by the same kernel: nothing of image size is read, written or allocated.  Inputs d_tile_w,
 * d_tile_h, d_slots are in the pxz_varied_layout order for src_block_w x src_block_h with slots of
 * src_block_w*src_block_h*channels bytes (what pxz_decode_varied_frames_device or a varied shrink at that block leaves);
 * outputs d_block_value, d_out_w, d_out_h, d_out_pixels are in the pxz_varied_layout order for params->block_w x block_h
 * with slots of block_w*block_h*channels bytes.  Of descs[i] only width and height are read.  expand_filter is what
 * to_image(filter) takes; params carries what the shrink takes (the NEW block size, mode, filter, factor).
 * For every image without a flagged tile the results equal, bit for bit (value bits, sizes, the valid bytes of every slot),
 * pxz_expand_varied_frames_device at the source block with expand_filter into a tightly packed image followed by
 * pxz_shrink_varied_frames_device with params on that image.  When both blocks are equal, the results equal
 * pxz_reshrink_varied_frames_device.
 * A SOURCE tile whose stored size is zero or exceeds its place in the source grid is flagged as by
 * pxz_expand_varied_frames_device -- d_image_flags (n_images dwords, may be NULL) receives 0 or 1 per image,
 * pxz_decode_status reports bit 0 -- and every destination tile that it covers gets d_out_w = d_out_h = 0 and value bits 0;
 * their slots are left as they were.  d_out_pixels may be NULL (values and sizes only).
 * The two layouts differ, so there is no in-place form: inputs and outputs must not overlap.
 * Asynchronous on the handle's stream; the number of launches does not depend on n_images.  Validation runs on the host
 * before anything is launched, with the rules, codes and "image i" texts of pxz_shrink_varied_frames_device for the
 * destination geometry (PXZ_ERR_TILE_TOO_SMALL included), and PXZ_ERR_INVALID_ARG for a zero source block or an
 * expand_filter above 4; on an error nothing is written.
 * Limit of this path: a block keeps the destination tile image (D = block_w*block_h*4 bytes: a dword per pixel, for RGB as
 * for RGBA) and one more region in LDS: while the tile is assembled, the stored pixels that one part's windows read (at most
 * about min(src, dst block) plus a window on each axis), the horizontal pass's intermediate and the windows of both source
 * axes; afterwards the image's other plane (D) and in shrink_by mode the detector's planes (16 KB), beside shrink_by's tables
 * (14 KB).  D and src_block_w*src_block_h*4 must not exceed 65536 bytes each and the sum not 160 KB; a pair beyond that gives
 * PXZ_ERR_UNSUPPORTED (pxz_retile_lds_bytes says which).  With Lanczos3 every pair of square blocks up to 109x109 fits, and
 * 128x128 on one side with up to 99x99 on the other; 128x128 <-> 128x127 does not.
 * The call touches only the varied scratch and none of the state the single-geometry fast paths keep in the handle;
 * pxz_trim gives back what it grew. */
int pxz_retile_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                    uint32_t src_block_w, uint32_t src_block_h, const pxz_params *params,
                                    uint32_t expand_filter, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                    const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                    uint8_t *d_out_pixels, uint32_t *d_image_flags);

/* LDS bytes of one block of the call above (host only: no handle, no GPU), from the layout function the kernel and its launch
 * use; conventions of pxz_reshrink_lds_bytes: a value above 163840 (0xffffffff when a plane of either block exceeds 65536
 * bytes) means PXZ_ERR_UNSUPPORTED.  PXZ_ERR_INVALID_ARG for a null pointer, a zero side, a mode above 1 or a filter above 4. */
int pxz_retile_lds_bytes(uint32_t src_block_w, uint32_t src_block_h, uint32_t block_w, uint32_t block_h, uint32_t mode,
                         uint32_t expand_filter, uint32_t *lds_bytes);

/* pix_to_pix for a folder, host files in, host files out, synchronously.  Every header is parsed on the host first
 * (pxz_file_header); the files must share channels and block size (PXZ_ERR_INVALID_ARG, "image i" otherwise), and the
 * descriptors come from the headers.  When the files' block size equals params->block_w / block_h the files go through the
 * varied reader, the re-shrink above in place and the varied writer: no allocation of image size anywhere.  With another
 * block size (the CLI's -b on a .pix input) they go through the varied reader at their own geometry, the re-tile above and
 * the writer whenever the new block divides the files' block on both axes (64x64 files to 32x32 tiles: every new tile lies
 * inside one tile of the files) and pxz_retile_lds_bytes says the pair fits: again nothing of image size is allocated.  Any
 * other pair goes through the reader, pxz_expand_varied_frames_device into a scratch image batch of the handle,
 * pxz_shrink_varied_frames_device at the new geometry and the writer -- new tiles that merge or straddle tiles of the files
 * measured slower through the re-tile, files to files; the files are byte for byte the same either way.
 * filter_byte goes into the new headers.  file_offsets (n_images + 1) are always written; the
 * files go to out when out_capacity >= file_offsets[n_images], else the call returns PXZ_ERR_BUFFER_TOO_SMALL and writes
 * nothing to out (out may be NULL for that size query), as pxz_encode_varied_images.  All or nothing: a malformed file or a
 * flagged tile gives PXZ_ERR_INVALID_ARG naming the first such image, and nothing is written to out or file_offsets.
 * Errors and limits otherwise as the calls it is made of. */
int pxz_transcode_varied_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                               const pxz_params *params, uint32_t expand_filter, uint32_t filter_byte, uint8_t *out,
                               uint64_t out_capacity, uint64_t *file_offsets);

/* Re-shrink ladder: pxz_reshrink_varied_frames_device at several factors in ONE launch, whatever n_images and n_factors are --
 * an archive of .pixlzr files, no source images, and the question how far it can be squeezed.  Every stored tile is expanded
 * once and measured once (neither depends on the factor); each rung only decides its levels, and a tile is resampled once per
 * distinct pair of levels among its rungs.  params->factor is ignored; factors is a HOST array (1 <= n_factors <=
 * PXZ_VARIED_LADDER_MAX_RUNGS, each finite; any order, repeats allowed).  Inputs as pxz_reshrink_varied_frames_device.  Outputs
 * are rung-major, exactly as pxz_shrink_varied_ladder_frames_device lays them out: rung r of tile t of image i is index
 * r*tiles + tile_offsets[i] + t of d_block_value, d_out_w, d_out_h and of the slots of d_out_pixels (64-bit offsets; may be
 * NULL), so the writer takes them with descs repeated n_factors times.  Rung r equals pxz_reshrink_varied_frames_device with
 * factor = factors[r] bit for bit (value bits, sizes, the valid bytes of every slot).
 * A flagged tile (stored size zero or beyond its place) sets d_image_flags and status bit 0 as there, and gets 0 x 0 and
 * value bits 0 at EVERY rung; every rung's slot is left as it was.
 * In place: rung 0 of d_out_w, d_out_h and d_out_pixels may be d_tile_w, d_tile_h and d_slots themselves (the arrays then
 * hold n_factors*tiles entries, the inputs in the first tiles of them).  Tile t's inputs are read only by tile t's block,
 * into registers and LDS before its first store, and the rungs from 1 on lie beyond the inputs.
 * Asynchronous on the handle's stream.  Validation runs on the host before anything is launched; on an error nothing is
 * written.  Rules, codes and "image i" texts are pxz_reshrink_varied_frames_device's; PXZ_ERR_INVALID_ARG for factors null,
 * n_factors 0 or above the maximum, a non-finite factor, or an expand_filter above 4; PXZ_ERR_UNSUPPORTED beyond the LDS
 * limit -- block_w*block_h*4 <= 65536 bytes for RGB and RGBA alike, and the oblong-block caveat of the re-shrink
 * (pxz_reshrink_ladder_lds_bytes says which) -- or when n_factors * tiles exceeds 2^32-1.  Of the handle's state the call
 * touches what the re-shrink touches: the varied scratch, none of what the single-geometry fast paths keep; pxz_trim gives
 * back what it grew. */
int pxz_reshrink_varied_ladder_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                             const pxz_params *params, uint32_t expand_filter, const float *factors,
                                             uint32_t n_factors, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                             const uint8_t *d_slots, float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                             uint8_t *d_out_pixels, uint32_t *d_image_flags);

/* LDS bytes of one block of the call above (host only: no handle, no GPU), from the layout function the kernel and its launch
 * use; conventions of pxz_reshrink_lds_bytes: above 163840 (0xffffffff beyond the documented limit) means
 * PXZ_ERR_UNSUPPORTED.  The footprint depends on the channel count: beside the two planes of a dword per pixel, a block keeps
 * its resampled images, in the plane the expand leaves free when they fit there.  PXZ_ERR_INVALID_ARG for a null pointer, a
 * zero side, channels other than 3 or 4, a mode above 1 or a filter above 4. */
int pxz_reshrink_ladder_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t mode, uint32_t expand_filter,
                                  uint32_t *lds_bytes);

/* Re-tile ladder: pxz_retile_varied_frames_device at several factors in ONE launch, whatever n_images and n_factors are -- an
 * archive written at one block size, no source images, and the question how far it can be squeezed at another.  Every tile of
 * the new grid is assembled once from the parts of the stored tiles that cover it and measured once (neither depends on the
 * factor); each rung only decides its levels, and a tile is resampled once per distinct pair of levels among its rungs.
 * Inputs (d_tile_w, d_tile_h, d_slots in the pxz_varied_layout order for src_block_w x src_block_h, descs, channels,
 * expand_filter, params with the NEW block size, mode and filter) are those of pxz_retile_varied_frames_device;
 * params->factor is ignored.  factors is a HOST array as in pxz_reshrink_varied_ladder_frames_device (1 <= n_factors <=
 * PXZ_VARIED_LADDER_MAX_RUNGS, each finite; any order, repeats allowed).
 * Outputs are rung-major in the DESTINATION layout, exactly as pxz_shrink_varied_ladder_frames_device lays them out for
 * params->block_w x block_h: rung r of tile t of image i is index r*tiles + tile_offsets[i] + t of d_block_value, d_out_w,
 * d_out_h and of the slots (block_w*block_h*channels bytes, 64-bit offsets) of d_out_pixels, which may be NULL (values and
 * sizes only); the writer takes them with descs repeated n_factors times.
 * Rung r equals pxz_retile_varied_frames_device with factor = factors[r] bit for bit (value bits, sizes, the valid bytes of
 * every slot), and therefore rung r of pxz_expand_varied_frames_device at the source block followed by
 * pxz_shrink_varied_ladder_frames_device at the new one.  When both blocks are equal the results equal
 * pxz_reshrink_varied_ladder_frames_device out of place.
 * A SOURCE tile whose stored size is zero or exceeds its place in the source grid sets d_image_flags (n_images dwords, may be
 * NULL) and status bit 0 as in the re-tile, and every destination tile that it covers gets d_out_w = d_out_h = 0 and value
 * bits 0 at EVERY rung; every rung's slot of such a tile is left as it was.
 * The two layouts differ, so there is no in-place form: inputs and outputs must not overlap.
 * Asynchronous on the handle's stream; one launch.  Validation runs on the host before anything is launched; on an error
 * nothing is written.  Rules, codes and "image i" texts are pxz_retile_varied_frames_device's for the destination geometry
 * (PXZ_ERR_TILE_TOO_SMALL included; PXZ_ERR_INVALID_ARG for a zero source block or an expand_filter above 4);
 * PXZ_ERR_INVALID_ARG for factors null, n_factors 0 or above the maximum, or a non-finite factor; PXZ_ERR_UNSUPPORTED beyond
 * the LDS limit (pxz_retile_ladder_lds_bytes says which pairs) or when n_factors * tiles exceeds 2^32-1.
 * Limit of this path: a block keeps the destination tile image (D = block_w*block_h*4 bytes) and one more region: the
 * re-tile's staging while the tile is assembled, afterwards the detector's planes (16 KB, shrink_by) and the resampled
 * images of one pair of levels (about 3/4 of block_w*block_h*channels bytes: a half and a quarter) -- the larger of the two,
 * beside shrink_by's tables (14 KB).  D and src_block_w*src_block_h*4 must not exceed 65536 bytes each and the sum not 160
 * KB.  The image's other plane, which the one-factor call keeps, is not needed, so every pair pxz_retile_lds_bytes admits is
 * admitted here (blocks of a few pixels take some bytes more: 3x5 RGBA 80 against 64).
 * The call touches only the varied scratch and none of the state the single-geometry fast paths keep in the handle;
 * pxz_trim gives back what it grew. */
int pxz_retile_varied_ladder_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                           uint32_t src_block_w, uint32_t src_block_h, const pxz_params *params,
                                           uint32_t expand_filter, const float *factors, uint32_t n_factors,
                                           const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                                           float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels,
                                           uint32_t *d_image_flags);

/* LDS bytes of one block of the call above (host only: no handle, no GPU), from the layout function the kernel and its launch
 * use; conventions of pxz_retile_lds_bytes: a value above 163840 (0xffffffff when a plane of either block exceeds 65536
 * bytes) means PXZ_ERR_UNSUPPORTED.  The footprint depends on the channel count (the resampled images).
 * PXZ_ERR_INVALID_ARG for a null pointer, a zero side, channels other than 3 or 4, a mode above 1 or a filter above 4. */
int pxz_retile_ladder_lds_bytes(uint32_t src_block_w, uint32_t src_block_h, uint32_t block_w, uint32_t block_h,
                                uint32_t channels, uint32_t mode, uint32_t expand_filter, uint32_t *lds_bytes);

/* pxz_transcode_varied_files at several factors: host files in, host files out, synchronously.  params->factor is ignored;
 * factors as above.  The new files are rung-major: file_offsets has n_factors*n_images + 1 entries, and the file of image i at
 * factors[r] is out[file_offsets[r*n_images + i] .. file_offsets[r*n_images + i + 1]), byte for byte what
 * pxz_transcode_varied_files gives for it at that factor.  With out == NULL or out_capacity below the last offset the call
 * returns PXZ_ERR_BUFFER_TOO_SMALL with the offsets exact and nothing written to out: that size query is the rate table -- file
 * length per file and factor, no file kept -- as pxz_rate_distortion_varied_images gives its lengths.  There is no distortion
 * column here; pxz_rate_distortion_varied_files adds it, measured against what each file decodes to, still without the image.
 * Same block size: the varied reader into rung 0 of the handle's tile scratch, the re-shrink ladder in place, the varied writer
 * over the descriptors repeated n_factors times.  Another block size: reader at the files' geometry, the re-tile ladder
 * above and the writer whenever the new block divides the files' block on both axes and pxz_retile_ladder_lds_bytes says the
 * pair fits -- nothing of image size is allocated; any other pair goes through reader, pxz_expand_varied_frames_device into
 * a scratch image batch of the handle, pxz_shrink_varied_ladder_frames_device and the writer.  That is the rule of
 * pxz_transcode_varied_files, and the measurement of DESIGN.md 8p supports it: from the same tiles the re-tile ladder is
 * 1.06-1.68x faster than expand + varied ladder where new tiles split tiles of the files (files to files level to 1.04x
 * on strongly shrunk files), but 0.91-1.27x where they merge and 0.72-1.06x where they straddle them, behind on strongly
 * shrunk files in two runs.  The files are byte for byte the same either way.  All or nothing as pxz_transcode_varied_files: a malformed file or a flagged
 * tile gives PXZ_ERR_INVALID_ARG naming the first such image, and nothing is written to out or file_offsets.  Errors and limits
 * otherwise as the calls it is made of. */
int pxz_transcode_varied_ladder_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                      const pxz_params *params, uint32_t expand_filter, const float *factors, uint32_t n_factors,
                                      uint32_t filter_byte, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets);

/* The same for one host-resident image (copies in, expands, copies out; PXZ_ERR_INVALID_ARG on an
 * invalid stored size). */
int pxz_expand_image(pxz_handle *h, uint32_t width, uint32_t height, uint32_t channels, uint32_t pitch_bytes,
                     uint32_t block_w, uint32_t block_h, uint32_t filter, const uint32_t *tile_w,
                     const uint32_t *tile_h, const uint8_t *slots, uint8_t *out_pixels);

/* ---- windows of files: pixel rectangles of .pixlzr files, without reading the rest ---- */

/* One pixel rectangle of one file of a call.  The container is built for random access -- the header carries one length per
 * tile row (encode_to_vec, src/encoding/mod.rs:77-82) and every record its own (encode_block, :193-197) -- and the reference
 * never uses it: decode_from_vec (mod.rs:95-165) reads whole images.  A viewer wants a viewport of a large frame, a data
 * loader one crop from each of a few hundred files. */
typedef struct pxz_window {
	uint32_t image;                 /* index into descs / the files of the call; several windows may name one image */
	uint32_t x, y, width, height;   /* pixel rectangle in that image: non-empty, wholly inside it */
	uint32_t pitch_bytes;           /* of the OUTPUT rows, >= width*channels */
	uint64_t offset_bytes;          /* output start relative to the call's base pointer, any alignment */
} pxz_window;

/* Layout of the per-tile outputs of a call over windows (host only: no handle, no GPU, like pxz_varied_layout).  Window k
 * covers tile columns x/block_w .. (x+width-1)/block_w and tile rows y/block_h .. (y+height-1)/block_h of its image; its
 * covered tiles are numbered row-major inside that covered grid, starting at tile_offsets[k], and tile_offsets[n_windows] is
 * the call's tile count.  A tile that two windows cover is there twice.  Slots stay block_w*block_h*channels bytes.
 * PXZ_ERR_INVALID_ARG for a null pointer, n_windows 0, an image index out of range, an empty rectangle or one that leaves its
 * image, and everything pxz_varied_layout refuses for the descriptors; PXZ_ERR_UNSUPPORTED for more than 2^32-1 covered tiles
 * (and what pxz_varied_layout answers with it). */
int pxz_window_layout(const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows,
                      uint32_t block_w, uint32_t block_h, uint64_t *tile_offsets);

/* Pixlzr::decode_from_vec (encoding/mod.rs:95-165) + decode_block (:202-242) for the covered tiles of the windows only, in
 * the pxz_window_layout order.  The files are given as for pxz_decode_varied_frames_device: n_images files back to back in
 * d_files, file i = [d_file_offsets[i], d_file_offsets[i+1]); of descs[i] only width and height are read, of a window its
 * image and rectangle, of params block_w and block_h.  Asynchronous on the handle's stream; the number of launches and
 * copies depends on neither n_images nor n_windows.  Per covered tile the outputs (value bits, stored size, the valid slot
 * bytes) are what pxz_decode_varied_frames_device gives for that tile.
 * What is read of a file: its 26-byte header, with the checks of the varied reader; its line table, which must sum to the
 * file's length; and in each covered tile row the records from the row's start up to the window's last column.  Records
 * left of the window are walked by their length fields and header-checked (a broken one ends the walk) but neither
 * published nor decoded; records right of the window, and tile rows outside it, are not touched.
 * So damage outside that range does not flag a window: a file that pxz_decode_varied_frames_device flags may give clean
 * windows.  Damage inside it flags the window and gives the affected covered tiles size 0x0, exactly as the varied reader
 * does for its image (a broken record takes the rest of its tile row with it).  d_window_flags (n_windows dwords, may be
 * NULL) receives 0 or 2 per window; pxz_decode_status reports the OR over the windows.
 * Validation runs on the host before anything is launched, with the codes of the varied reader and pxz_window_layout's
 * rules; the texts name "image i" or "window k"; on an error nothing is written. */
int pxz_decode_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows,
                              uint32_t n_windows, uint32_t channels, const pxz_params *params, const uint8_t *d_files,
                              const uint64_t *d_file_offsets, float *d_block_value, uint32_t *d_tile_w, uint32_t *d_tile_h,
                              uint8_t *d_slots, uint32_t *d_window_flags);

/* Pixlzr::expand (pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) for the windows: every covered tile (as the call above
 * leaves them) is resized to its full size with params->filter as PixlzrBlock::resize does (block.rs:273-334), and the
 * intersection of the tile with the window is written: pixel (px, py) of the image goes to d_base + offset_bytes +
 * (py - y)*pitch_bytes + (px - x)*channels.  No byte outside the window's width*channels bytes per row, for height rows, is
 * written.  Window k equals the same rectangle of what pxz_expand_varied_frames_device writes for its image, byte for byte.
 * Overlapping output rectangles are the caller's business: which window's bytes such a place ends up with is not defined.
 * A covered tile whose stored size is zero or exceeds its place is skipped (its pixels stay as they were) and flagged:
 * d_window_flags (may be NULL) receives 0 or 1 per window, pxz_decode_status bit 0 the OR.  Asynchronous; validation as above
 * (here the windows' pitches count too, and params->filter).  Limits are those of pxz_distortion_*: a wave keeps the tile in
 * LDS, so block_w*block_h*channels must not exceed 65536 bytes and RGB blocks must stay below the size (about 19 400
 * pixels) where pxz_expand_varied_frames_device moves its tiles to HBM; PXZ_ERR_UNSUPPORTED beyond.  There is no HBM form. */
int pxz_expand_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows,
                              uint32_t n_windows, uint32_t channels, const pxz_params *params, const uint32_t *d_tile_w,
                              const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_window_flags);

/* Host files in, host crops out, synchronously.  files[i] / lens[i] is file i; window k is written at out_base +
 * windows[k].offset_bytes with windows[k].pitch_bytes between rows, and must end inside the out_bytes bytes at out_base
 * (PXZ_ERR_BUFFER_TOO_SMALL, "window k").  Composition only, as pxz_decode_varied_files: every header is parsed on the host
 * first (pxz_file_header) and a file whose size, block size or channels disagree with descs[i] and the call is refused
 * (PXZ_ERR_INVALID_ARG, "image i"), nothing written; then one upload (the files go whole), the two calls above, one download.
 * Windows that come back flagged -- window_flags[k] (may be NULL), bits as pxz_decode_status -- have the tiles that could not
 * be read left zero; the call then returns PXZ_ERR_INVALID_ARG naming the first such window, and every other window is
 * complete.  Errors and limits as pxz_expand_windows_device.  pxz_trim returns the scratch. */
int pxz_decode_windows_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs,
                             uint32_t n_images, const pxz_window *windows, uint32_t n_windows, uint32_t channels,
                             const pxz_params *params, uint8_t *out_base, uint64_t out_bytes, uint32_t *window_flags);

/* ---- decode at reduced scale: images and windows at 1/2^k from the stored tiles ---------------- */

/* A .pixlzr file is a level-of-detail format; the calls above rebuild every tile at its full size, and both callers named
 * above want fewer pixels than the file holds: the viewer a zoomed-out viewport, the data loader a thumbnail or a small crop.
 * The reference has the semantics already: Pixlzr::expand (pixlzr.rs:77-122) resizes each block to whatever the struct's public
 * width, height, block_width and block_height say, through PixlzrBlock::resize (block.rs:273-334), which takes any source and
 * target size.  With s = 2^scale_log2: set block_width /= s, block_height /= s, width = ceil(width/s), height = ceil(height/s)
 * on an opened file, and expand(filter).to_image() is the image these calls return.
 *   - s must divide block_w and block_h (PXZ_ERR_INVALID_ARG otherwise);
 *   - a tile whose full place is fw x fh at (x0, y0) is resized to ceil(fw/s) x ceil(fh/s) and written at (x0/s, y0/s); the
 *     scaled image is ceil(W/s) x ceil(H/s); the tile grid, and so pxz_varied_layout and pxz_window_layout, are unchanged;
 *   - the resize is PixlzrBlock::resize for ANY size pair: a clone when both sizes agree (bytes as they are), the Nearest pick,
 *     or the horizontal then the vertical convolution pass with a u8 intermediate, RGBA premultiplied around them.  One flag,
 *     target wider than stored || target higher than stored, picks the kernel of Triangle for BOTH axes (block.rs:301-304,
 *     mod.rs:65-107): Hamming when nothing grows, Bilinear when any axis grows -- then also on the axis that shrinks;
 *   - a stored size is impossible only when it is zero or exceeds the FULL place fw x fh; above the target it is ordinary.
 *
 * pxz_scaled_size: the scaled image's size (host only, like pxz_grid).  PXZ_ERR_INVALID_ARG for a null pointer, a zero size or
 * block, scale_log2 > 31, or a scale that does not divide both block sides; PXZ_ERR_UNSUPPORTED as pxz_grid. */
int pxz_scaled_size(uint32_t width, uint32_t height, uint32_t block_w, uint32_t block_h, uint32_t scale_log2, uint32_t *out_w,
                    uint32_t *out_h);

/* The axis table the scaled kernels use for in_size stored samples -> out_size (host only, beside pxz_axis_table, same
 * outputs).  other_axis_grows: the tile's other axis grows, which sets PixlzrBlock::resize's flag for this one too; it matters
 * only for Triangle on an axis that shrinks.  With other_axis_grows == 0 this is pxz_axis_table. */
int pxz_scaled_axis_table(uint32_t in_size, uint32_t out_size, uint32_t filter, uint32_t other_axis_grows, int32_t *starts,
                          int32_t *sizes, int16_t *coeffs, int32_t *window, int32_t *precision);

/* LDS bytes of one wave's image in the scaled kernels for blocks of block_w x block_h decoded at scales up to
 * 2^max_scale_log2 with `filter` (host only): two planes of a dword per block pixel, the staged windows of both axes -- sized
 * by the taps the largest scale needs -- and a row of padding.  *lds_bytes is written whenever the arguments are valid;
 * PXZ_ERR_UNSUPPORTED when the image, with the 8 KB of owners' first tiles beside it, exceeds the 160 KB of a block (the two
 * calls below answer the same), or when block_w*block_h*channels exceeds 65536 bytes; PXZ_ERR_INVALID_ARG for a scale that
 * does not divide the block.  Blocks up to 128x128 fit; there is no HBM form. */
int pxz_expand_scaled_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t filter, uint32_t max_scale_log2,
                                uint32_t *lds_bytes);

/* pxz_expand_varied_frames_device at reduced scale: image i of the batch is written at 1/2^scale_log2[i] (a HOST array of
 * n_images entries).  descs[i].width and .height are the FILE's, so the tiles are pxz_varied_layout's; pitch_bytes and
 * offset_bytes describe the SCALED output, pitch_bytes >= ceil(width/s)*channels.  Otherwise the call behaves as
 * pxz_expand_varied_frames_device: validation on the host before any launch with its codes and texts ("image i"), bytes that
 * belong to no image are not written, flags as there, one launch whatever n_images.  With every scale 0 the output equals that
 * call's byte for byte.  A wave's image beyond LDS (pxz_expand_scaled_lds_bytes) is PXZ_ERR_UNSUPPORTED. */
int pxz_expand_varied_scaled_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                           const pxz_params *params, const uint32_t *scale_log2, const uint32_t *d_tile_w,
                                           const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_base, uint32_t *d_image_flags);

/* pxz_expand_windows_device at reduced scale: window k is written at 1/2^scale_log2[k] (a HOST array of n_windows entries).
 * The windows are the SAME structs, in full-resolution pixels, that pxz_window_layout and pxz_decode_windows_device took, so
 * the reader is used unchanged.  With s = 2^scale_log2[k]: x and y must be multiples of s, x+width a multiple of s or the
 * image's width, y+height a multiple of s or the image's height (PXZ_ERR_INVALID_ARG, "window k").  The output is
 * ceil((x+width)/s) - x/s pixels wide and ceil((y+height)/s) - y/s high -- pitch_bytes is checked against that -- and equals
 * that rectangle, from (x/s, y/s) on, of the scaled whole image; no byte outside it is written.  Flags, errors and limits as
 * pxz_expand_windows_device and pxz_expand_scaled_lds_bytes. */
int pxz_expand_windows_scaled_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows,
                                     uint32_t n_windows, uint32_t channels, const pxz_params *params, const uint32_t *scale_log2,
                                     const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots, uint8_t *d_base,
                                     uint32_t *d_window_flags);

/* The host forms: pxz_decode_varied_files and pxz_decode_windows_files with a scale per image / per window (host arrays).
 * descs[i] carries the FILE's width and height and the pitch and offset of the SCALED image in out_base; a window its
 * full-resolution rectangle and the pitch and offset of its scaled crop.  Composition through the calls above and the
 * unchanged readers; only the scaled bytes come down.  Errors, flags and the all-or-nothing rules are those of the twins. */
int pxz_decode_varied_files_scaled(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs,
                                   uint32_t n_images, uint32_t channels, const pxz_params *params, const uint32_t *scale_log2,
                                   uint8_t *out_base, uint32_t *image_flags);
int pxz_decode_windows_files_scaled(pxz_handle *h, const uint8_t *const *files, const size_t *lens, const pxz_image_desc *descs,
                                    uint32_t n_images, const pxz_window *windows, uint32_t n_windows, uint32_t channels,
                                    const pxz_params *params, const uint32_t *scale_log2, uint8_t *out_base, uint64_t out_bytes,
                                    uint32_t *window_flags);

/* ---- patch: new pixels into pixel windows of .pixlzr files, the rest untouched ---------------- */

/* The write side of the windows.  The reference has the semantics: decode_block gives every stored block block_value: Some(..)
 * (src/encoding/mod.rs:236-241), and Pixlzr::shrink_by returns such blocks as they are and shrinks only blocks without a value
 * (src/data_types/pixlzr.rs:166-170).  So: open a file, replace the blocks a window covers by fresh full-size blocks -- the stored
 * block resized to its place (PixlzrBlock::resize, as expand does) with the new pixels written over it --, shrink, save.  Exactly
 * the covered blocks are measured and shrunk again; every other block keeps its stored size, its value bits and its bytes.
 * The hull of a window is the tile-aligned rectangle of its covered tiles, clipped to the image.  pxz_window_layout of window k
 * is pxz_varied_layout of ONE image of the hull's size -- same grid, same row-major order, same ragged edge tiles -- so whatever
 * takes a varied batch (the writer, pxz_record_bytes_varied_device, ...) takes the covered tiles as they are, with one
 * descriptor of the hull's size per window.
 *
 * pxz_patch_check (host only: no handle, no GPU, like pxz_window_layout): answers what pxz_window_layout answers, tile_offsets
 * included, and PXZ_ERR_INVALID_ARG when two windows of one image cover a common tile: the covered tile rectangles of one image
 * must be pairwise disjoint (pixel rectangles in different tiles of one tile row are fine; windows of different images never
 * collide).  *bad_window (may be NULL) receives the index of the first window that covers a tile an earlier window of its image
 * covers, PXZ_NO_WINDOW when the call succeeds or fails for another reason.  Every entry point below runs it first. */
#define PXZ_NO_WINDOW 0xffffffffu
int pxz_patch_check(const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows, uint32_t n_windows, uint32_t block_w,
                    uint32_t block_h, uint64_t *tile_offsets, uint32_t *bad_window);

/* Tiles to tiles.  Inputs: the covered tiles as pxz_decode_windows_device leaves them (d_tile_w, d_tile_h, d_slots in the
 * pxz_window_layout order, slots of block_w*block_h*channels bytes) and the same descs and windows -- but for THIS call
 * windows[k].pitch_bytes and offset_bytes describe the INPUT rectangle of new pixels at d_patch_base: width x height pixels of
 * `channels` interleaved bytes, any alignment.  params carries what the shrink takes (block size, mode, filter, factor),
 * expand_filter what to_image(filter) takes.  Outputs in the same layout: d_block_value, d_out_w, d_out_h, d_out_pixels (may be
 * NULL: values and sizes only).
 * For every window without a flagged tile the outputs equal, bit for bit (value bits, sizes, the valid bytes of every slot),
 * this composition: pxz_expand_windows_device of the window's hull (a window struct with the hull's rectangle) with
 * expand_filter into a tightly packed image; the new pixels written over their rectangle of that image;
 * pxz_shrink_varied_frames_device with params over the hulls as a varied batch.  No image exists here: each covered tile is
 * rebuilt in LDS, overlaid, measured and resampled by one block of one kernel; a tile the window covers wholly is not even
 * expanded.  The overlay writes plain bytes over the finished tile image (RGBA: after the expand's un-premultiply, before the
 * shrink's premultiply).
 * A covered tile whose stored size is zero or exceeds its place is flagged and emptied exactly as by
 * pxz_reshrink_varied_frames_device -- d_window_flags (n_windows dwords, may be NULL) receives 0 or 1 per window,
 * pxz_decode_status reports bit 0, the tile gets d_out_w = d_out_h = 0 and value bits 0, its slot is left as it was -- also when
 * the window covers the tile wholly, so that there is one rule.
 * In place: d_out_w, d_out_h and d_out_pixels may be d_tile_w, d_tile_h and d_slots themselves, as in the re-shrink.
 * Asynchronous on the handle's stream; ONE launch whatever n_windows.  Validation runs on the host before anything is launched,
 * with the re-shrink's codes and texts and pxz_patch_check's; the texts name "window k"; a window's pitch below width*channels is
 * PXZ_ERR_INVALID_ARG; PXZ_ERR_TILE_TOO_SMALL (shrink_directionally) is judged on the covered tiles, so an image whose edge tiles
 * are narrower than 2 px can still be patched away from that edge.  On an error nothing is written.
 * Limit: pxz_reshrink_lds_bytes (block_w*block_h*4 <= 65536 and the windows of both axes beside two planes); there is no HBM
 * form.  The call reads and writes none of the state the single-geometry fast paths keep in the handle; pxz_trim gives back what
 * it grew. */
int pxz_patch_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows,
                             uint32_t n_windows, uint32_t channels, const pxz_params *params, uint32_t expand_filter,
                             const uint8_t *d_patch_base, const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                             float *d_block_value, uint32_t *d_out_w, uint32_t *d_out_h, uint8_t *d_out_pixels,
                             uint32_t *d_window_flags);

/* Files plus new covered tiles to files.  Inputs: the old files as the window reader took them (d_files, d_file_offsets), the same
 * descs and windows (image and rectangle are read; of params block_w and block_h), the new covered tiles (d_block_value, d_tile_w,
 * d_tile_h, d_slots in the pxz_window_layout order: what the call above leaves) and the two calls' window flags (d_reader_flags
 * from pxz_decode_windows_device, d_patch_flags from the call above; either may be NULL).  The record bounds of the covered tiles
 * are taken from the scratch pxz_decode_windows_device left in THIS handle: the call must follow that reader, with the same
 * windows and with no other reader call between them (PXZ_ERR_INVALID_ARG when the handle holds no such scratch).
 * Output: the new files back to back in d_out, file i = [d_out_file_offsets[i], d_out_file_offsets[i+1]) (n_images + 1 u64).  File
 * i consists of the old 26-byte header verbatim (the filter byte stays); the line table, in which the length of every tile row a
 * window touches is recomputed; in every tile row each record that no window covers as the OLD BYTES, span by span, never
 * re-encoded; and each covered record as encode_block (src/encoding/mod.rs:168-200) of its new tile, by the writer of
 * pxz_encode_varied_frames_device over the hulls.  An image without a window passes through byte for byte and unread.  An image
 * with a flagged window -- a flag passed in, a covered tile the reader left without a record, a new tile of size zero -- gets a
 * file of length zero; d_image_flags (n_images dwords, may be NULL) receives the OR of its windows' flags.  Damage outside what
 * the windows' reader reads is copied as it is.
 * Capacity as pxz_encode_varied_frames_device: the offsets are always exact and no byte at or beyond out_capacity is written
 * (d_out may be NULL when out_capacity is 0: the size query).  Asynchronous on the handle's stream; the number of launches and
 * copies depends on neither n_images nor n_windows, and nothing is read back to the host.  Validation on the host before any
 * launch, pxz_patch_check's; PXZ_ERR_UNSUPPORTED for more than 2^32-1 pieces (spans of old bytes and rows of new records) in
 * all.  pxz_trim returns the scratch, the staging of the new records included. */
int pxz_splice_windows_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, const pxz_window *windows,
                              uint32_t n_windows, uint32_t channels, const pxz_params *params, const uint8_t *d_files,
                              const uint64_t *d_file_offsets, const float *d_block_value, const uint32_t *d_tile_w,
                              const uint32_t *d_tile_h, const uint8_t *d_slots, const uint32_t *d_reader_flags,
                              const uint32_t *d_patch_flags, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_out_file_offsets,
                              uint32_t *d_image_flags);

/* Host files and host rectangles of new pixels in, host files out, synchronously.  files[i] / lens[i] is file i; patches[k] is
 * window k's new pixels, windows[k].pitch_bytes their pitch (offset_bytes is ignored).  Every header is parsed on the host first
 * and the descriptors come from them, as in pxz_transcode_varied_files: the files must share channels and block size, and
 * params->block_w / block_h must be theirs (PXZ_ERR_INVALID_ARG: a patch keeps the block size).  Composition only: one upload
 * (the files whole, the patches behind them), pxz_decode_windows_device, pxz_patch_windows_device in place,
 * pxz_splice_windows_device, and the way down.  file_offsets (n_images + 1) and out follow the protocol of
 * pxz_encode_varied_images: PXZ_ERR_BUFFER_TOO_SMALL with the offsets written and nothing in out when out_capacity is below
 * file_offsets[n_images] (out may be NULL for that size query).  All or nothing: a flagged window gives PXZ_ERR_INVALID_ARG
 * naming "window k", and nothing is written to out or file_offsets.  Errors and limits as pxz_patch_windows_device. */
int pxz_patch_windows_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                            const pxz_window *windows, uint32_t n_windows, const uint8_t *const *patches, const pxz_params *params,
                            uint32_t expand_filter, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets);

/* ---- rate and distortion: what a factor costs and what it loses ---------------- */

/* The squared error of stored tiles against the frames they were shrunk from.  Nothing in the reference computes it:
 * src/bin/whole-folder.rs:69-117 writes, for every k = i/20, the .pixlzr file and the PNG that comes back, and leaves the
 * comparison to a person.  For every tile and channel: the sum over the tile's pixels of (source - expanded)^2, where
 * `expanded` is exactly what pxz_expand_frames_device writes for that stored tile with params->filter, i.e. Pixlzr::expand
 * (pixlzr.rs:77-122) + to_image (pixlzr_image.rs:24-74) -- the image itself is never written.  An integer; MSE and PSNR are
 * the caller's: 10 log10(255^2 n / sse) over n samples.
 * `frames` describes the SOURCE frames at d_pixels; params->block_w, block_h and filter (the UP-scaling filter) are used.
 * n_sets >= 1 stored versions of every frame's tiles are compared in one call, set-major as pxz_shrink_ladder_frames_device
 * leaves its rungs: index (s * n_frames + f) * tiles + t of d_tile_w, d_tile_h and d_slots (slots of
 * block_w*block_h*channels bytes).  d_tile_sse (n_sets*n_frames*tiles*channels u64, same order, channel last; may be NULL)
 * gets the tiles' sums, d_frame_sse (n_sets*n_frames*channels u64) their totals per frame -- integer sums, so the result does
 * not depend on the order of the additions.  A tile stored at its full size is the source (block.rs:279-281): its sums are 0
 * and neither its slot nor the source is read.  A tile whose stored size is zero or exceeds its place follows
 * pxz_expand_frames_device: skipped and flagged (pxz_decode_status bit 0); its d_tile_sse entries are all-ones
 * (UINT64_MAX) and the frame's totals leave it out.
 * Asynchronous on the handle's stream; the number of launches and copies does not depend on n_frames or n_sets; none of the
 * state the single-geometry fast paths keep in the handle is touched.  Validation runs on the host before anything is
 * launched, with pxz_expand_frames_device's rules and codes, and n_sets == 0 is PXZ_ERR_INVALID_ARG; on an error nothing is
 * written.  Limit: a wave keeps the tile in LDS, so block_w*block_h*channels must not exceed 65536 bytes, and RGB blocks
 * must stay below the size (about 19 400 pixels) where pxz_expand_varied_frames_device moves its tiles to HBM;
 * PXZ_ERR_UNSUPPORTED beyond. */
int pxz_distortion_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, uint32_t n_sets,
                                 const uint8_t *d_pixels, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                 const uint8_t *d_slots, uint64_t *d_tile_sse, uint64_t *d_frame_sse);

/* The same for one set of stored tiles of a batch of differently sized images (no reference line either: see above).  The
 * images are the SOURCE, image i at d_base + descs[i].offset_bytes with descs[i].pitch_bytes between rows, any alignment;
 * tiles in the pxz_varied_layout order.  d_tile_sse (tiles*channels u64, may be NULL), d_image_sse (n_images*channels u64).
 * d_image_flags (n_images dwords, may be NULL) receives 0 or 1 per image as from pxz_expand_varied_frames_device.  Each
 * image's results equal pxz_distortion_frames_device on that image alone.  Validation, "image i" texts and the limit as
 * pxz_expand_varied_frames_device; on an error nothing is written. */
int pxz_distortion_varied_frames_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                        const pxz_params *params, const uint8_t *d_base, const uint32_t *d_tile_w,
                                        const uint32_t *d_tile_h, const uint8_t *d_slots, uint64_t *d_tile_sse,
                                        uint64_t *d_image_sse, uint32_t *d_image_flags);

/* One host-resident image in, one row per factor out: the sweep of src/bin/whole-folder.rs:83-113 as numbers instead of
 * files.  For every factors[r] (1 <= n_factors <= PXZ_LADDER_MAX_RUNGS): file_bytes[r] is the length of the .pixlzr file
 * Pixlzr::from_image + shrink_by | shrink_directionally (filter_down) + encode_to_vec give (filter byte 0), and
 * sse[r*channels + c] the squared error of channel c between the image and what expand + to_image(filter_up) make of that
 * file.  Composition only: upload, pxz_shrink_ladder_frames_device, pxz_encode_frames_device for its offsets (no file is
 * kept), pxz_distortion_frames_device over the n_factors rung sets, one download.  Synchronous.  Errors and limits are
 * those of the three calls. */
int pxz_rate_distortion_image(pxz_handle *h, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                              uint32_t pitch_bytes, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                              uint32_t filter_up, const float *factors, uint32_t n_factors, uint64_t *file_bytes,
                              uint64_t *sse);

/* The same table for a folder: host-resident images of different sizes in, one row per (factor, image) out.  pixels[i] is
 * image i (descs[i].offset_bytes is ignored).  file_bytes[r*n_images + i] and sse[(r*n_images + i)*channels + c] are what
 * pxz_rate_distortion_image gives for image i at factors[r] (1 <= n_factors <= PXZ_VARIED_LADDER_MAX_RUNGS).  Composition
 * only: upload, pxz_shrink_varied_ladder_frames_device, pxz_encode_varied_frames_device over the descriptors repeated
 * n_factors times for its offsets (no file is kept), pxz_distortion_varied_frames_device over the same descriptors, one
 * download.  Synchronous.  Errors and limits are those of the calls it composes. */
int pxz_rate_distortion_varied_images(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs,
                                      uint32_t n_images, uint32_t channels, uint32_t block_w, uint32_t block_h, uint32_t mode,
                                      uint32_t filter_down, uint32_t filter_up, const float *factors, uint32_t n_factors,
                                      uint64_t *file_bytes, uint64_t *sse);

/* ---- fit to a budget: each image at the factor its target picks ---------------------------------------------- */

/* What a caller asks of the table above: "this file in at most N bytes" or "with at least Q dB".  The reference has no line
 * for it either (whole-folder.rs:83-113 writes every factor and leaves the choice to a person).  Per image, over its rungs
 * r = 0 .. n_factors-1, with bytes[r] the length of its file at factors[r] and sse[r] the sum over its channels of the squared
 * error (uint64 integers throughout):
 *   PXZ_FIT_BYTES  target = the largest file length allowed.  Eligible: bytes[r] <= target.  Among the eligible rungs the
 *                  smallest sse, ties by the smaller bytes, then the lower r.  None eligible: the smallest bytes, ties by the
 *                  smaller sse, then the lower r, and bit 0 of the image's fit flags is set.
 *   PXZ_FIT_SSE    target = the largest summed squared error allowed (a PSNR of q dB over n samples is
 *                  sse <= 255^2 n / 10^(q/10)).  Eligible: sse[r] <= target.  Among the eligible rungs the smallest bytes,
 *                  ties by the smaller sse, then the lower r.  None eligible: the smallest sse, ties by the smaller bytes,
 *                  then the lower r, and bit 0 is set.
 * Ties are ordinary: neighbouring factors often give every tile the same pair of levels, hence the same length and error. */
typedef enum { PXZ_FIT_BYTES = 0, PXZ_FIT_SSE = 1 } pxz_fit;

/* The rule on the host (no handle, no GPU, like pxz_grid and pxz_varied_layout), over a table laid out as
 * pxz_rate_distortion_varied_images returns it: file_bytes[r*n_images + i], sse[(r*n_images + i)*channels + c]; targets,
 * choice and fit_flags have n_images entries.  choice[i] is the rung of image i, fit_flags[i] 0 or 1 (bit 0: no rung met the
 * target).  PXZ_ERR_INVALID_ARG for a null pointer, n_images 0, n_factors 0 or above PXZ_VARIED_LADDER_MAX_RUNGS, channels
 * not 3|4 or an unknown criterion; on an error nothing is written.  The device call below runs the same text of the rule. */
int pxz_fit_select(uint32_t n_images, uint32_t n_factors, uint32_t channels, uint32_t criterion, const uint64_t *targets,
                   const uint64_t *file_bytes, const uint64_t *sse, uint32_t *choice, uint32_t *fit_flags);

/* The rule on the device, over what pxz_encode_varied_frames_device (d_file_offsets: n_factors*n_images + 1 offsets; file
 * r*n_images + i is [k], [k+1]) and pxz_distortion_varied_frames_device (d_image_sse: n_factors*n_images*channels sums) leave
 * for the descriptors repeated n_factors times -- a varied ladder's result.  targets is a HOST array of n_images entries; it
 * travels with the call through a handle buffer that pxz_trim gives back.  d_choice and d_fit_flags (n_images dwords each)
 * equal pxz_fit_select on the downloaded table.  One launch; asynchronous on the handle's stream; none of the state the
 * single-geometry fast paths keep in the handle is touched.  Validation as pxz_fit_select, and PXZ_ERR_INVALID_ARG for a null
 * handle or device pointer; on an error nothing is written. */
int pxz_fit_varied_ladder_device(pxz_handle *h, uint32_t n_images, uint32_t n_factors, uint32_t channels, uint32_t criterion,
                                 const uint64_t *targets, const uint64_t *d_file_offsets, const uint64_t *d_image_sse,
                                 uint32_t *d_choice, uint32_t *d_fit_flags);

/* One rung per image out of a varied ladder's result, as an ordinary varied batch: a batch in which every image has its own
 * factor.  The inputs are rung-major as pxz_shrink_varied_ladder_frames_device writes them (n_factors rungs); the outputs are
 * in the pxz_varied_layout order of the n_images images.  With tile_offsets and tiles = tile_offsets[n_images]: output tile
 * tile_offsets[i] + t is input tile d_choice[i]*tiles + tile_offsets[i] + t -- the value's bits, both sizes, and exactly the
 * out_w*out_h*channels valid bytes of the slot (never more than a slot); the rest of the output slot is not written.
 * d_out_pixels may be NULL: values and sizes only (d_slots is not read then).  Only block_w and block_h of params are read.
 * A choice of n_factors or more is read as n_factors-1, so nothing is read out of bounds, and sets bit 1 of
 * d_image_flags[i] (n_images dwords, may be NULL); the flags are otherwise written as 0.  One launch, whatever n_images and
 * n_factors are; slots of block_w*block_h*channels bytes, addressed with 64-bit offsets.  Outputs must not overlap inputs
 * (not checked).  pxz_encode_varied_frames_device takes the result as it is.  Asynchronous on the handle's stream; none of the
 * state the single-geometry fast paths keep in the handle is touched.
 * Validation runs on the host before anything is launched; on an error nothing is written.  Codes and "image i" texts are
 * pxz_shrink_varied_ladder_frames_device's (no factors are passed, and no mode: no tile is too small).  No tile is staged, so
 * there is no LDS limit on the block; PXZ_ERR_UNSUPPORTED for a slot above 2^32-1 bytes or n_factors * tiles above 2^32-1. */
int pxz_gather_varied_rungs_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                   const pxz_params *params, uint32_t n_factors, const uint32_t *d_choice,
                                   const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                   const uint8_t *d_slots, float *d_out_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                   uint8_t *d_out_pixels, uint32_t *d_image_flags);

/* Host images in, one .pixlzr file per image out, each at the factor the rule picks for it; synchronous.  pixels[i] is image
 * i (descs[i].offset_bytes is ignored); factors (1 <= n_factors <= PXZ_VARIED_LADDER_MAX_RUNGS, each finite, any order) are
 * the candidates, targets[i] the budget of image i under `criterion`.  Composition only: upload,
 * pxz_shrink_varied_ladder_frames_device, pxz_encode_varied_frames_device over the n_factors*n_images rung images with no
 * room (for its offsets), pxz_distortion_varied_frames_device over the same (filter_up), pxz_fit_varied_ladder_device,
 * pxz_gather_varied_rungs_device, pxz_encode_varied_frames_device over the n_images gathered images, one download.  Nothing
 * is shrunk or uploaded twice, and nothing comes back to the host before the files and their table.
 * File i is, byte for byte, what pxz_encode_varied_images gives for image i alone at factors[choice[i]] with filter_down and
 * filter_byte.  The output follows pxz_encode_varied_images' protocol: file_offsets (n_images + 1), choice and fit_flags
 * (n_images each; see pxz_fit_select) and, where given, table_bytes (n_factors*n_images) and table_sse
 * (n_factors*n_images*channels) -- what pxz_rate_distortion_varied_images returns -- are always written; the files go to out
 * when out_capacity >= file_offsets[n_images], else the call returns PXZ_ERR_BUFFER_TOO_SMALL and writes nothing to out (out
 * may be NULL for that size query).  Errors and limits are those of the calls it composes (block_w*block_h*channels <= 65536
 * bytes among them); on any other error nothing is written. */
int pxz_encode_varied_images_fit(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                                 uint32_t channels, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                                 uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                                 const uint64_t *targets, uint32_t filter_byte, uint8_t *out, uint64_t out_capacity,
                                 uint64_t *file_offsets, uint32_t *choice, uint32_t *fit_flags, uint64_t *table_bytes /* may be NULL */,
                                 uint64_t *table_sse /* may be NULL */);

/* ---- fit a .pixlzr archive to a budget: the error of a re-shrunk tile without the image ----------------------- */

/* The rule: the error of rung r of a file is measured against what the file decodes to NOW, not against an original nobody
 * has.  For an unchanged block size tile t of the decoded image is exactly the expansion of stored tile t, so the error needs
 * two tile-sized images in LDS and nothing of image size in device memory.
 * For every tile of the flat tile space (pxz_varied_layout order of descs; of a descriptor only width, height and reserved are
 * read) and every one of n_sets stored versions of it, per channel the sum over the tile's full pixels of
 *   (expand(reference stored tile, expand_filter) - expand(set's stored tile, params->filter))^2,
 * both being what pxz_expand_varied_frames_device writes for that stored tile with that filter: the result equals
 * pxz_expand_varied_frames_device of the reference (expand_filter) into a packed image followed by
 * pxz_distortion_varied_frames_device of each set against it (params->filter), bit for bit, and that image is never made.
 * d_ref_w, d_ref_h, d_ref_slots: the archive's tiles (tiles entries, slots of block_w*block_h*channels bytes) as
 * pxz_decode_varied_frames_device leaves them.  d_tile_w, d_tile_h, d_slots: n_sets*tiles entries, set-major -- index
 * s*tiles + t, exactly what pxz_reshrink_varied_ladder_frames_device writes.  A ladder run IN PLACE on rung 0 has overwritten
 * the archive's tiles: the reference must be kept, so run the ladder out of place.
 * d_tile_sse (n_sets*tiles*channels u64, index (s*tiles + t)*channels + c; may be NULL), d_image_sse
 * (n_sets*n_images*channels u64, index (s*n_images + i)*channels + c: what pxz_fit_varied_ladder_device reads; zeroed by the
 * call), d_image_flags (n_images dwords, may be NULL).  Integer sums: the result does not depend on the order of the additions.
 *   reference stored at full size: its bytes are the reference;  set tile stored at full size: sums 0, its slot is not read;
 *   a set's stored size of zero or beyond its place: that entry all-ones (UINT64_MAX), the image's flag and
 *   pxz_decode_status bit 0 set, the totals leave it out;  such a reference tile: every set's entry for the tile all-ones,
 *   flagged, in no total, and nothing of the tile is read.
 * Asynchronous on the handle's stream; the number of launches and copies does not depend on n_images or n_sets; only the varied
 * scratch of the handle is touched (pxz_trim gives it back), none of the state of the single-geometry fast paths.
 * Validation runs on the host before anything is launched, with pxz_distortion_varied_frames_device's rules, codes and
 * "image i" texts (no image, so no pitch rule); PXZ_ERR_INVALID_ARG also for n_sets == 0 or a filter above 4,
 * PXZ_ERR_UNSUPPORTED for n_sets*tiles above 2^32-1 and for a block beyond the limit below; on an error nothing is written.
 * Limit: a wave keeps THREE planes of block_w*block_h dwords and the windows of both axes in LDS, beside the images' first
 * tiles -- pxz_reshrink_distortion_lds_bytes says what that takes.  The largest admitted square block is 112x112 (113x113
 * when both filters are Nearest; the re-shrink itself goes to 128x128). */
int pxz_reshrink_distortion_varied_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                          const pxz_params *params /* block_w, block_h; filter = filter_up */,
                                          uint32_t expand_filter, uint32_t n_sets, const uint32_t *d_ref_w,
                                          const uint32_t *d_ref_h, const uint8_t *d_ref_slots, const uint32_t *d_tile_w,
                                          const uint32_t *d_tile_h, const uint8_t *d_slots, uint64_t *d_tile_sse,
                                          uint64_t *d_image_sse, uint32_t *d_image_flags);

/* Host only (no handle, no GPU), as pxz_reshrink_lds_bytes: *lds_bytes = the LDS a one-wave block of the call above takes for
 * this block and pair of filters -- the images' first tiles (8192 bytes) and the wave's three planes and windows, from the
 * layout function the launch uses.  A value above 163840 means the call returns PXZ_ERR_UNSUPPORTED for that block.
 * PXZ_ERR_INVALID_ARG for a null pointer, a zero side, channels not 3|4 or a filter above 4. */
int pxz_reshrink_distortion_lds_bytes(uint32_t block_w, uint32_t block_h, uint32_t channels, uint32_t expand_filter,
                                      uint32_t filter_up, uint32_t *lds_bytes);

/* The table of pxz_rate_distortion_varied_images for an archive: host-resident .pixlzr files in (files[i], lens[i]; all of one
 * channel count and of params' block size), one row per (factor, file) out.  file_bytes[r*n_images + i] is the length of the
 * file pxz_transcode_varied_ladder_files writes for file i at factors[r], sse[(r*n_images + i)*channels + c] the squared error
 * of channel c between what file i decodes to (expand_filter) and what that new file decodes to (filter_up).  params: block_w,
 * block_h, mode and filter (the down-scaling filter); factor is ignored.  Composition only: the headers, upload,
 * pxz_decode_varied_frames_device into a buffer of its own, pxz_reshrink_varied_ladder_frames_device out of place,
 * pxz_encode_varied_frames_device over the n_factors*n_images rung images with no room (for its offsets),
 * pxz_reshrink_distortion_varied_device, one download.  Synchronous.  A malformed file or a tile that cannot be fails the
 * whole call as in pxz_transcode_varied_files (nothing is written); files of another block size than params' are
 * PXZ_ERR_UNSUPPORTED (pxz_rate_distortion_retile_files and the two fit forms beside it, below, take another block size).
 * Other errors and limits are those of the calls it composes. */
int pxz_rate_distortion_varied_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                     const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                     uint32_t n_factors, uint64_t *file_bytes, uint64_t *sse);

/* "Squeeze every file of this archive under N bytes" (or "keep at least Q dB of what it decodes to now") without the images:
 * the chain above, then pxz_fit_varied_ladder_device, pxz_gather_varied_rungs_device, pxz_encode_varied_frames_device over
 * the n_images gathered images, one download.  targets[i] is the budget of file i under `criterion` (pxz_fit).  File i of the
 * output is, byte for byte, pxz_transcode_varied_files of file i alone at factors[choice[i]], and the whole output equals
 * pxz_decode_varied_files (expand_filter) followed by pxz_encode_varied_images_fit, whose pixels never exist here.  Output
 * protocol, the PXZ_ERR_BUFFER_TOO_SMALL size query and what is always written follow pxz_encode_varied_images_fit; malformed
 * files, flagged tiles and another block size as in pxz_rate_distortion_varied_files. */
int pxz_transcode_varied_files_fit(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                   const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                   uint32_t n_factors, uint32_t criterion, const uint64_t *targets, uint32_t filter_byte,
                                   uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets, uint32_t *choice,
                                   uint32_t *fit_flags, uint64_t *table_bytes /* may be NULL */, uint64_t *table_sse /* may be NULL */);

/* ---- fit to a budget per tile: each tile at the rung its group's target picks ---------------------------------- */

/* A .pixlzr file knows no factors: every record carries its own stored size and value, so a file whose tiles come from
 * different rungs of a ladder is an ordinary file.  One factor per image spends bytes evenly where the error is not even; the
 * calls below choose a rung per TILE, under one target per GROUP -- a run of consecutive images (one image, or a whole folder).
 * Candidate (t, r), rung r of flat tile t, has b = the bytes of its record (u32) and s = the sum over its channels of its
 * squared error.  It is usable when no channel sum is UINT64_MAX, s < 2^32 and b < 2^24 (the library's own calls stay inside
 * both for every block they admit: 65536 * 255^2 < 2^32); unusable candidates are skipped.  A tile with no usable candidate
 * gets choice 0, counts in no total and sets bit 1 of its group's flags.
 *   pick(t, lambda) = the usable r with the smallest (s + lambda*b, b, r), lambda an integer in [0, PXZ_TILEFIT_LAMBDA_MAX];
 *   B(lambda) = the group's fixed bytes + the sum of b(pick) over its tiles, S(lambda) = the sum of s(pick).
 * B never increases with lambda and S never decreases.  All arithmetic is u64 (a cost stays below 2^57).
 *   PXZ_FIT_BYTES  lambda* = the smallest lambda with B(lambda) <= target.  B(2^32) > target: lambda* = 2^32 and bit 0 (missed)
 *                  is set -- every tile has taken its fewest bytes, so no assignment of rungs fits.
 *   PXZ_FIT_SSE    lambda* = the largest lambda with S(lambda) <= target.  S(0) > target: lambda* = 0 and bit 0 is set.
 * Never worse than one factor for the group: when the target was not missed, the totals (B_u(r), S_u(r)) of each rung that is
 * usable for every tile of the group go through pxz_fit_select's rule, and the group takes that one rung for all its tiles
 * (bit 2) when it is eligible and its (minimised, constrained) pair is strictly smaller than that of the pick at lambda*.
 * Flags per group: bit 0 missed, bit 1 a tile without a usable candidate, bit 2 one rung for all. */
#define PXZ_TILEFIT_LAMBDA_MAX 4294967296ull   /* 2^32 */

/* The rule on the host (no handle, no GPU, like pxz_fit_select).  Group g owns the flat tiles [group_tile_offsets[g],
 * group_tile_offsets[g+1]) (n_groups + 1 entries from 0 on, strictly ascending: a group has a tile), tiles =
 * group_tile_offsets[n_groups]; group_fixed_bytes[g] are the headers and line tables of its files, targets[g] its budget under
 * `criterion` (pxz_fit).  tile_bytes[r*tiles + t] (u32) and tile_sse[(r*tiles + t)*channels + c] (u64) are the candidates,
 * 1 <= n_factors <= PXZ_VARIED_LADDER_MAX_RUNGS.  Outputs: tile_choice[t], and per group lambda (lambda*), bytes and sse (the
 * totals of the final choice, fixed bytes included) and flags.  PXZ_ERR_INVALID_ARG for a null pointer, n_groups 0, n_factors 0
 * or above the maximum, channels not 3|4, an unknown criterion, or offsets that do not start at 0 or do not ascend;
 * PXZ_ERR_UNSUPPORTED for n_factors * tiles above 2^32-1; on an error nothing is written.  The device call below runs the same
 * text of the rule. */
int pxz_fit_tiles_select(uint32_t n_groups, const uint64_t *group_tile_offsets, const uint64_t *group_fixed_bytes, uint32_t n_factors,
                         uint32_t channels, uint32_t criterion, const uint64_t *targets, const uint32_t *tile_bytes,
                         const uint64_t *tile_sse, uint32_t *tile_choice, uint64_t *group_lambda, uint64_t *group_bytes,
                         uint64_t *group_sse, uint32_t *group_flags);

/* The record lengths of the writer: the inputs of pxz_encode_varied_frames_device (for a ladder's result: the descriptors
 * repeated n_factors times, as there) in, d_record_bytes out -- one u32 per tile in flat tile order, the bytes record t
 * occupies in its file: "block" + value + length field + QOI without its magic = 13 + the record's length field.
 * d_file_offsets (n_images + 1 u64, may be NULL) is exactly what pxz_encode_varied_frames_device gives with out_capacity 0.
 * For every image: 26 + 4*rows + the sum of its tiles' record bytes == the length of its file.  No file is written.
 * Asynchronous on the handle's stream; the number of launches does not depend on n_images.  Validation is
 * pxz_encode_varied_frames_device's; on an error nothing is written. */
int pxz_record_bytes_varied_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                   const pxz_params *params, const float *d_block_value, const uint32_t *d_tile_w,
                                   const uint32_t *d_tile_h, const uint8_t *d_slots, uint32_t *d_record_bytes,
                                   uint64_t *d_file_offsets /* may be NULL */);

/* The rule on the device, over a varied ladder's result: d_record_bytes (the call above over the descriptors repeated
 * n_factors times: index r*tiles + t) and d_tile_sse (pxz_distortion_varied_frames_device or
 * pxz_reshrink_distortion_varied_device over the same: index (r*tiles + t)*channels + c).  descs are the n_images images
 * themselves; of params only block_w and block_h are read.  group_first is a HOST array of n_groups + 1 image indices,
 * strictly ascending from 0 to n_images: group g is the images [group_first[g], group_first[g+1]); NULL means every image is
 * its own group (n_groups must be n_images then).  targets is a HOST array of n_groups entries; both travel through handle
 * buffers that pxz_trim gives back.  The fixed bytes of a group are the sum of 26 + 4*rows over its images.
 * d_tile_choice (tiles dwords), d_group_lambda, d_group_bytes, d_group_sse (n_groups u64 each) and d_group_flags (n_groups
 * dwords) equal pxz_fit_tiles_select on the downloaded tables.  A fixed chain of one memset and 37 launches (one per halving of
 * [0, 2^32], 33 of them, the kernel boundary being the only synchronisation), whatever n_images, n_groups, the tiles and n_factors are;
 * nothing is read back in between; integer atomics only, so the result does not depend on the order of arrival.
 * Asynchronous on the handle's stream; none of the state the single-geometry fast paths keep in the handle is touched.
 * Validation runs on the host before anything is launched, as pxz_gather_varied_rungs_device and pxz_fit_select, plus
 * PXZ_ERR_UNSUPPORTED for block_w*block_h*channels > 65536 (the bound on s rests on it) and PXZ_ERR_INVALID_ARG for a bad
 * group_first or n_groups; on an error nothing is written. */
int pxz_fit_varied_tiles_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                const pxz_params *params, const uint32_t *group_first /* may be NULL */, uint32_t n_groups,
                                uint32_t n_factors, uint32_t criterion, const uint64_t *targets, const uint32_t *d_record_bytes,
                                const uint64_t *d_tile_sse, uint32_t *d_tile_choice, uint64_t *d_group_lambda,
                                uint64_t *d_group_bytes, uint64_t *d_group_sse, uint32_t *d_group_flags);

/* pxz_gather_varied_rungs_device with a choice per tile: output tile t is input tile d_tile_choice[t]*tiles + t -- the value's
 * bits, both sizes and exactly the valid bytes of the slot; d_tile_choice has tiles entries in flat tile order.  A choice of
 * n_factors or more is read as n_factors-1 and sets bit 1 of the owning image's entry of d_image_flags (n_images dwords, may
 * be NULL; zeroed by the call).  One kernel launch, no LDS, 64-bit offsets; everything else -- the outputs, d_out_pixels NULL,
 * validation, codes and limits -- is pxz_gather_varied_rungs_device's. */
int pxz_gather_varied_tile_rungs_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                        const pxz_params *params, uint32_t n_factors, const uint32_t *d_tile_choice,
                                        const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                                        const uint8_t *d_slots, float *d_out_value, uint32_t *d_out_w, uint32_t *d_out_h,
                                        uint8_t *d_out_pixels, uint32_t *d_image_flags);

/* pxz_encode_varied_images_fit with a rung per tile: host images in, one .pixlzr file per image out, its tiles taken from the
 * rungs the rule above picks under targets[g] (n_groups entries) for the groups group_first describes (as in
 * pxz_fit_varied_tiles_device; NULL: every image its own group, n_groups == n_images; one group over all images is "one
 * budget for the whole folder").  Composition only: upload, pxz_shrink_varied_ladder_frames_device,
 * pxz_record_bytes_varied_device and pxz_distortion_varied_frames_device (with its per-tile sums) over the n_factors*n_images
 * rung images, pxz_fit_varied_tiles_device, pxz_gather_varied_tile_rungs_device, pxz_encode_varied_frames_device over the
 * n_images gathered images, one download.  File i is what pxz_encode_container makes of image i's gathered tiles; with one
 * factor it is pxz_encode_varied_images' file.  group_bytes[g] is the summed length of the group's files, group_sse[g] the
 * squared error between its images and what pxz_decode_varied_files (filter_up) makes of those files.
 * Always written: file_offsets (n_images + 1), tile_choice (tiles entries in flat tile order, may be NULL) and the groups'
 * lambda, bytes, sse and flags (n_groups each); the files go to out when out_capacity >= file_offsets[n_images], else the call
 * returns PXZ_ERR_BUFFER_TOO_SMALL and writes nothing to out (out may be NULL for that size query).  A tile without a usable
 * candidate or a choice beyond the ladder cannot come from the library's own ladder: PXZ_ERR_INTERNAL.  Errors and limits are
 * those of the calls it composes; on any other error nothing is written. */
int pxz_encode_varied_images_fit_tiles(pxz_handle *h, const uint8_t *const *pixels, const pxz_image_desc *descs, uint32_t n_images,
                                       uint32_t channels, uint32_t block_w, uint32_t block_h, uint32_t mode, uint32_t filter_down,
                                       uint32_t filter_up, const float *factors, uint32_t n_factors, uint32_t criterion,
                                       const uint32_t *group_first /* may be NULL */, uint32_t n_groups, const uint64_t *targets,
                                       uint32_t filter_byte, uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets,
                                       uint32_t *tile_choice /* may be NULL */, uint64_t *group_lambda, uint64_t *group_bytes,
                                       uint64_t *group_sse, uint32_t *group_flags);

/* The same for an archive, as pxz_transcode_varied_files_fit: the error of a candidate is measured against what its file
 * decodes to NOW (pxz_reshrink_distortion_varied_device with its per-tile sums), nothing of image size exists on the device,
 * and a malformed file or a tile that cannot be fails the whole call before anything is written.  group_sse[g] is the squared
 * error between what the group's input files decode to (expand_filter) and what its output files decode to (filter_up). */
int pxz_transcode_varied_files_fit_tiles(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                         const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                         uint32_t n_factors, uint32_t criterion, const uint32_t *group_first /* may be NULL */,
                                         uint32_t n_groups, const uint64_t *targets, uint32_t filter_byte, uint8_t *out,
                                         uint64_t out_capacity, uint64_t *file_offsets, uint32_t *tile_choice /* may be NULL */,
                                         uint64_t *group_lambda, uint64_t *group_bytes, uint64_t *group_sse, uint32_t *group_flags);

/* ---- fit a .pixlzr archive to a budget at a NEW block size: the error of a re-tiled tile without the image ------ */

/* pxz_reshrink_distortion_varied_device for a block size that changes: the sets are tiles of the grid of params->block_w x
 * block_h, the archive's tiles those of src_block_w x src_block_h, both over the same images (pxz_varied_layout order of descs
 * at the respective block; of a descriptor only width, height and reserved are read).  For every tile of the DESTINATION grid,
 * every one of n_sets stored versions of it and every channel, the sum over the tile's full pixels of
 *   (decoded(archive)[pixel] - expand(set's stored tile, params->filter)[pixel])^2,
 * decoded(archive) being what pxz_expand_varied_frames_device writes from the archive's tiles at the source block with
 * expand_filter: the result equals that call into a tightly packed image followed by pxz_distortion_varied_frames_device at the
 * new block for each set (params->filter), bit for bit, and that image is never made -- a destination tile of it is put together
 * in LDS from the parts of the source tiles that cover it, as pxz_retile_varied_frames_device does.  When both blocks are
 * equal the result equals pxz_reshrink_distortion_varied_device.
 * d_ref_w, d_ref_h, d_ref_slots: the archive's tiles in the SOURCE layout (slots of src_block_w*src_block_h*channels bytes) as
 * pxz_decode_varied_frames_device leaves them.  d_tile_w, d_tile_h, d_slots: n_sets*tiles entries of the DESTINATION layout,
 * set-major -- index s*tiles + t, slots of block_w*block_h*channels bytes, exactly what
 * pxz_retile_varied_ladder_frames_device writes.  d_tile_sse (may be NULL), d_image_sse (zeroed by the call) and d_image_flags
 * (may be NULL) have the sizes and index orders of pxz_reshrink_distortion_varied_device, tiles being the destination grid's,
 * so pxz_fit_varied_ladder_device and pxz_fit_varied_tiles_device take them as they are.  Integer sums, 64-bit integer
 * atomics: the result does not depend on the order of arrival.
 *   set tile stored at full size: sums 0, its slot is not read;
 *   a set's stored size of zero or beyond its place: that entry all-ones (UINT64_MAX), the image's flag and
 *   pxz_decode_status bit 0 set, the totals leave it out;
 *   a SOURCE tile whose stored size is zero or beyond its place in the source grid: every set's entry of EVERY destination tile
 *   it covers all-ones, flagged, in no total, and nothing of those tiles is compared.
 * Asynchronous on the handle's stream; one launch, whatever n_images and n_sets are; only the varied scratch of the handle is
 * touched (pxz_trim gives it back), none of the state of the single-geometry fast paths.
 * Validation runs on the host before anything is launched; on an error nothing is written.  Rules, codes and "image i" texts
 * are pxz_retile_varied_ladder_frames_device's for the two geometries (PXZ_ERR_INVALID_ARG for a zero source block or an
 * expand_filter above 4) and pxz_reshrink_distortion_varied_device's for n_sets and the filters; PXZ_ERR_UNSUPPORTED beyond the
 * LDS limit (pxz_retile_distortion_lds_bytes says which pairs) or when n_sets*tiles exceeds 2^32-1.
 * Limit: a block keeps TWO destination tile images (D = block_w*block_h*4 bytes each: the reference and one set's tile) and
 * the re-tile's staging -- for the source side, or for a whole stored tile of the destination block (up to D staged, up to D of
 * intermediate, the windows of both axes), whichever is larger.  D and src_block_w*src_block_h*4 must not exceed 65536 bytes
 * each and the sum not 160 KB.  With Lanczos3 on both sides the largest admitted equal square pair is 99x99 <-> 99x99
 * (160 832 bytes; 100x100 takes 164 000); 64x64 destination blocks take 66.5 KB at most, 32x32 ones at most 22.6 KB from
 * source blocks up to 64x64. */
int pxz_retile_distortion_varied_device(pxz_handle *h, const pxz_image_desc *descs, uint32_t n_images, uint32_t channels,
                                        uint32_t src_block_w, uint32_t src_block_h,
                                        const pxz_params *params /* the NEW block_w, block_h; filter = filter_up */,
                                        uint32_t expand_filter, uint32_t n_sets, const uint32_t *d_ref_w,
                                        const uint32_t *d_ref_h, const uint8_t *d_ref_slots, const uint32_t *d_tile_w,
                                        const uint32_t *d_tile_h, const uint8_t *d_slots, uint64_t *d_tile_sse,
                                        uint64_t *d_image_sse, uint32_t *d_image_flags);

/* LDS bytes of one block of the call above (host only: no handle, no GPU), from the layout function the kernel and its launch
 * use; conventions of pxz_retile_ladder_lds_bytes: a value above 163840 (0xffffffff when a plane of either block exceeds 65536
 * bytes) means PXZ_ERR_UNSUPPORTED.  The footprint depends on both filters (the staged windows) and not on the channel count.
 * PXZ_ERR_INVALID_ARG for a null pointer, a zero side, channels other than 3 or 4 or a filter above 4. */
int pxz_retile_distortion_lds_bytes(uint32_t src_block_w, uint32_t src_block_h, uint32_t block_w, uint32_t block_h,
                                    uint32_t channels, uint32_t expand_filter, uint32_t filter_up, uint32_t *lds_bytes);

/* pxz_rate_distortion_varied_files at a NEW block size: params->block_w x block_h is the block of the files that would be
 * written, the files' own block comes from their headers (all of one block and channel count).  file_bytes[r*n_images + i] is
 * the length of the file pxz_transcode_varied_ladder_files writes for file i at factors[r] with these params (its size query),
 * sse[(r*n_images + i)*channels + c] the squared error of channel c between what file i decodes to (expand_filter) and what
 * that new file decodes to (filter_up).  Composition only: the headers, upload, pxz_decode_varied_frames_device at the files'
 * geometry into a buffer of its own, then the rungs --
 *   another block: pxz_expand_varied_frames_device into a scratch image batch of the handle (on the device: no pixel crosses
 *   the bus), pxz_shrink_varied_ladder_frames_device, the writer for its offsets, pxz_distortion_varied_frames_device against
 *   that image;
 *   equal blocks: the chain of pxz_rate_distortion_varied_files --
 * and one download.  The rule of pxz_transcode_varied_ladder_files would send a pair whose new block divides the files' block
 * through pxz_retile_varied_ladder_frames_device and pxz_retile_distortion_varied_device, with nothing of image size allocated.
 * Files to files that route measured 7-9 % SLOWER than the image batch on strongly shrunk files, in two runs whose samples
 * spread by 1 %, and level on files stored mostly full, so, as for the merging and straddling pairs of
 * pxz_transcode_varied_files, this call takes the images for every other block; a caller to whom the 4 bytes per pixel of
 * scratch matter more than the time composes the device calls.  The numbers are the same on every path.  Synchronous.  A malformed file or a tile that cannot be fails the
 * whole call as in pxz_transcode_varied_files (PXZ_ERR_INVALID_ARG naming the first such image; nothing is written).  Other
 * errors and limits are those of the calls it composes. */
int pxz_rate_distortion_retile_files(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                     const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                     uint32_t n_factors, uint64_t *file_bytes, uint64_t *sse);

/* pxz_transcode_varied_files_fit at a NEW block size: "squeeze this 64x64 archive under N bytes per file at 32x32 tiles".  The
 * chain above, then pxz_fit_varied_ladder_device, pxz_gather_varied_rungs_device, the writer over the gathered images, one
 * download.  Arguments and output protocol are pxz_transcode_varied_files_fit's; params->block_w x block_h is the NEW block.
 * File i of the output is, byte for byte, pxz_transcode_varied_files of file i alone at factors[choice[i]] with the new block,
 * and the whole output equals pxz_decode_varied_files (expand_filter) followed by pxz_encode_varied_images_fit at the new
 * block.  With equal blocks it is pxz_transcode_varied_files_fit. */
int pxz_retile_varied_files_fit(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                uint32_t n_factors, uint32_t criterion, const uint64_t *targets, uint32_t filter_byte,
                                uint8_t *out, uint64_t out_capacity, uint64_t *file_offsets, uint32_t *choice,
                                uint32_t *fit_flags, uint64_t *table_bytes /* may be NULL */, uint64_t *table_sse /* may be NULL */);

/* pxz_transcode_varied_files_fit_tiles at a NEW block size: a rung per tile of the NEW grid under the groups' targets.
 * Arguments and output protocol are pxz_transcode_varied_files_fit_tiles's (tile_choice: the new grid's tiles); the whole
 * output equals pxz_decode_varied_files (expand_filter) followed by pxz_encode_varied_images_fit_tiles at the new block. */
int pxz_retile_varied_files_fit_tiles(pxz_handle *h, const uint8_t *const *files, const size_t *lens, uint32_t n_images,
                                      const pxz_params *params, uint32_t expand_filter, uint32_t filter_up, const float *factors,
                                      uint32_t n_factors, uint32_t criterion, const uint32_t *group_first /* may be NULL */,
                                      uint32_t n_groups, const uint64_t *targets, uint32_t filter_byte, uint8_t *out,
                                      uint64_t out_capacity, uint64_t *file_offsets, uint32_t *tile_choice /* may be NULL */,
                                      uint64_t *group_lambda, uint64_t *group_bytes, uint64_t *group_sse, uint32_t *group_flags);

/* ---- legacy image -> image filter ------------------------ */

/* process_custom (src/process/mod.rs:71-102) with the closures of process() (:107-121: |x - avg| and the
 * identity): per tile get_block_variance -> reduce_image_section((v, v)) with params->filter (the
 * down-scaling filter) -> .resize(w0, h0, filter_upscale) -> copy_from into an RGBA8 image
 * (DynamicImage::new_rgba8, :80-81; RGB input gains alpha 255).  process(image, n) is block_w = block_h = n,
 * params->filter = PXZ_FILTER_LANCZOS3, filter_upscale = PXZ_FILTER_NEAREST.  params->mode and factor are
 * ignored.  Two launches' worth of device work (shrink into the handle's scratch, expand into d_out_rgba);
 * asynchronous on the handle's stream. */
int pxz_process_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                              uint32_t filter_upscale, const uint8_t *d_pixels, uint8_t *d_out_rgba,
                              uint32_t out_pitch_bytes, uint64_t out_frame_stride_bytes);

/* tree::process_custom (src/process/tree.rs:23-83) with the closures of tree::process (:89-109): per tile of the
 * block_w x block_h grid get_block_variance (|x - avg|, identity); a tile with (value >= |threshold|) ^ (threshold >= 0)
 * is pixelised as process() does it (reduce_image_section((v, v)) with params->filter, resized back with
 * filter_upscale); any other tile is handed to the same function with both block sizes halved (|threshold| from
 * there on, so only the outermost level can be inverted) until a block size is no larger than max(min_block_*, 4)
 * (tree.rs:32-36), where the tile keeps its pixels.  tree::process(image, n, k) is block_w = block_h = n, min 4 x 4,
 * PXZ_FILTER_LANCZOS3 down, PXZ_FILTER_NEAREST up, threshold k.  Output RGBA8 (RGB input gains alpha 255; also in the
 * degenerate case of a block size at or below the minimum, where the reference returns the image unchanged in its own
 * colour type).  Any block geometry up to 128 x 128 (what src/bin/tree.rs:6 calls it with): blocks of at most 64 px that
 * halve evenly down to the last level run one detector + shrink + expand pass per level over that level's regular
 * grid; everything else -- 128-px blocks, halvings that go odd (50 -> 25 -> 12 + 12 + 1: every tile is cut from its own
 * corner, tree.rs:70-79) -- goes level by level over lists of rectangles, one block of threads per open tile, with one
 * 8-byte read-back per level: the next level's tile count and a consistency flag (a tile whose axis tables the host
 * did not list -> PXZ_ERR_INTERNAL; so that form is synchronous).  Blocks above 128 px: PXZ_ERR_UNSUPPORTED.  params->mode and factor are ignored. */
int pxz_tree_process_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params,
                                   uint32_t filter_upscale, float threshold, uint32_t min_block_w, uint32_t min_block_h,
                                   const uint8_t *d_pixels, uint8_t *d_out_rgba, uint32_t out_pitch_bytes,
                                   uint64_t out_frame_stride_bytes);

/* Block-stream compaction (device): the valid out_w*out_h*channels bytes of every slot, in tile
 * order, into one contiguous stream -- the payload `encode_block` (src/encoding/mod.rs:168-200)
 * consumes tile after tile, and what one rank ships to the writer rank over RCCL.
 * d_offsets gets n_tiles+1 byte offsets (u64; the last one is the stream length).  Tiles that
 * would exceed packed_capacity are skipped (offsets stay valid, so the caller can detect it).
 * Asynchronous on the handle's stream. */
int pxz_pack_tiles_device(pxz_handle *h, uint32_t n_tiles, uint32_t channels, uint32_t slot_bytes,
                          const uint32_t *d_tile_w, const uint32_t *d_tile_h, const uint8_t *d_slots,
                          uint64_t *d_offsets, uint8_t *d_packed, uint64_t packed_capacity);

/* Pixlzr::encode_to_vec (src/encoding/mod.rs:40-89) + encode_block (:168-200) + the `qoi` crate 0.4.1
 * encoder it calls (:181-189), entirely on the device: the tiles of a batch of frames (as left by
 * pxz_shrink_frames_device: values, dims, slots) become the complete .pixlzr files, back to back in
 * d_out.  d_file_offsets gets n_frames+1 byte offsets (file f = [off[f], off[f+1])).  filter_byte as in
 * pxz_encode_container.  If out_capacity is too small the files are truncated but the offsets are
 * still exact (retry with off[n_frames] bytes).  Asynchronous on the handle's stream. */
int pxz_encode_frames_device(pxz_handle *h, const pxz_frames *frames, const pxz_params *params, uint32_t filter_byte,
                             const float *d_block_value, const uint32_t *d_tile_w, const uint32_t *d_tile_h,
                             const uint8_t *d_slots, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_file_offsets);

/* ---- bitstream: Pixlzr::encode_to_vec, src/encoding/mod.rs:40-89,168-200 ---- */
/* Tiles given as produced by pxz_shrink_image (slots + dims + values).
 * has_value may be NULL (all Some); has_value[t]==0 writes 0.0 (mod.rs:173-178).
 * filter_byte = `self.filter.unwrap_or_default() as u8` (mod.rs:53): 0 after from_image.
 * Returns the number of bytes written into `out`, or a negative pxz_status;
 * call with out==NULL to obtain an upper bound. */
int64_t pxz_encode_container(uint32_t width, uint32_t height, uint32_t block_w, uint32_t block_h,
                             uint32_t channels, uint32_t filter_byte, const float *block_value,
                             const uint8_t *has_value, const uint32_t *tile_w, const uint32_t *tile_h,
                             const uint8_t *slots, uint8_t *out, size_t out_capacity);

/* qoi::Encoder::new(data,w,h).encode_to_vec() as called at mod.rs:181-189
 * (qoi crate 0.4.1 semantics incl. its run-of-one INDEX substitution).
 * Writes the full stream incl. "qoif"; returns its length or a negative status. */
int64_t pxz_qoi_encode(const uint8_t *data, uint32_t w, uint32_t h, uint32_t channels,
                       uint8_t *out, size_t out_capacity);
size_t pxz_qoi_bound(uint32_t w, uint32_t h, uint32_t channels);

/* ---- utilities -------------------------------------------------------- */
/* Deterministic synthetic frames for benchmarks/tests (integer-only generator,
 * DESIGN.md "Synthetic frames"); dist: 0 opaque, 1 alpha, 2 flat, 3 noise.
 * frame f of the batch uses seed 0x5049584C + first_frame_index + f. */
int pxz_synth_frames_device(pxz_handle *h, const pxz_frames *frames, uint8_t *d_pixels,
                            uint32_t first_frame_index, uint32_t dist);

/* Down-scaling tables the kernels use for one axis (for cross-checks):
 * fast_image_resize coefficient windows in i16 fixed point.  coeffs has room for
 * out_size*window entries; any output pointer may be NULL. */
int pxz_axis_table(uint32_t in_size, uint32_t out_size, uint32_t filter,
                   int32_t *starts, int32_t *sizes, int16_t *coeffs, int32_t *window, int32_t *precision);

/* Average device time (milliseconds) of the kernels launched by the last
 * *_device call on this handle, measured with HIP events on the handle's
 * stream; blocks until that work is done.  Enabled by pxz_enable_timing(h, 1); pxz_enable_timing(h, n) with
 * n > 1 brackets every n-th step only (three event records cost a 0.27 ms step about 2 %). */
int pxz_enable_timing(pxz_handle *h, int on);
int pxz_last_kernel_ms(pxz_handle *h, float *ms);
/* The same average for the FIRST kernel of each step alone (shrink32/64/16_kernel; oklab_kernel in shrink_by
 * steps): the figure a per-kernel profile shows for it.  Call before pxz_last_kernel_ms, which resets the record. */
int pxz_last_first_kernel_ms(pxz_handle *h, float *ms);

/* Diagnostics: the handle's kernel-selection state.  Two dwords in pinned memory, written by the worklist kernel of the last
 * FINISHED fast-path launch and read without synchronisation when the next one is set up, pick which kernels run (never what
 * they compute): state[0] = full tiles with transparency that launch saw (>= 2048: the four-plane kernel is launched; >= half
 * the tiles: it goes first), state[1] = tiles it listed for the worklist kernel (sizes that kernel's grid), state[2] = 1 if the
 * LAST launch set up through this handle ran the four-plane kernel, state[3] = 1 if it ran it first.  A timing is only
 * comparable with another taken in the same state; bench.py prints it beside its numbers. */
int pxz_handle_state(pxz_handle *h, uint32_t state[4]);

/* Diagnostics: copies `bytes` bytes at byte `offset` of the handle's worklist buffer to `dst` after waiting for the
 * handle's stream (the in-kernel phase stamps of the -DPXZ_STAMPS build land there; tools/stamps_run.py).  Not part of
 * the path; PXZ_ERR_INVALID_ARG when the range lies outside the buffer. */
int pxz_debug_read_work(pxz_handle *h, void *dst, size_t offset, size_t bytes);
/* The same for the status buffer of the decode side (the -DPXZ_STAMPS build keeps expand_kernel's phase stamps behind the
 * status word; tools/stamps_expand.py). */
int pxz_debug_read_status(pxz_handle *h, void *dst, size_t offset, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* PIXLZR_HIP_H */
