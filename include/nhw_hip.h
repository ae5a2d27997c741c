/*
 * nhw_hip.h -- C ABI of libnhwhip.so: the MI355X (gfx950) NHW encoder hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI; its de-facto C API
 * is encoder/codec.h:184-219 (`read_image_bmp` / `encode_image` / `write_compressed_file`, one
 * 512x512 image per call, errors by exit()).  The entry points below replace that trio for whole
 * batches of images:
 *
 *   reference                                            this library
 *   ---------------------------------------------------  ------------------------------------------
 *   im.setup->quality_setting (nhw_encoder_cli.c:175)     `quality` argument (1..23: every setting the reference has tables for)
 *   read_image_bmp  -> im_buffer4 (nhw_encoder.c:3047)    caller passes n x 786432 BGR24 bytes in BMP
 *                                                         file order (what fread at :3086 delivers)
 *   downsample_YUV420 + encode_image (codec.h:184,189)    nhw_enc_batch / nhw_enc_batch_device
 *   write_compressed_file (nhw_encoder.c:3100)            the .nhw bytes land in the output arena
 *   exit(-1) on code-book overflow (compress_pixel.c:234) per-image status NHW_E_CODEBOOK
 *
 * Plain C types only; device pointers are passed as void*; `stream` is a hipStream_t passed as
 * void* (NULL = the library's own stream).  One nhw_enc handle drives one GPU and is not
 * re-entrant; use one handle per host thread / process (one process per GPU under torchrun).
 */
#ifndef NHW_HIP_H
#define NHW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NHW_IMG_BYTES   786432u      /* 512*512*3, encoder/codec.h:58-61 */
#define NHW_OUT_STRIDE  (512u << 10) /* bytes reserved per image in the device output arena */

enum {
	NHW_OK = 0,
	NHW_E_QUALITY = -1,   /* quality outside the supported set */
	NHW_E_CODEBOOK = -2,  /* reference would exit(-1): compress_pixel.c:234,270,271 */
	NHW_E_SPACE = -3,     /* output arena too small */
	NHW_E_ARG = -4,
	NHW_E_HIP = -5,       /* a HIP call failed; see nhw_last_error() */
	NHW_E_FORMAT = -6,    /* decoder: not a well-formed .nhw file (the reference prints "Not an .nhw file" and exits, or reads out of bounds) */
	NHW_E_BUDGET = -7     /* nhw_enc_fit_batch*, nhw_enc_fit_sse_batch*: no quality of the ladder gives a file within the image's byte or distortion budget */
};

typedef struct nhw_enc nhw_enc;
typedef struct nhw_dec nhw_dec;

/* stage timings of the last nhw_enc_batch_device call, measured with hipEvents on the launch stream */
typedef struct {
	float total_ms;
	float front_ms;       /* colour + pre-filter + level-1 analysis (the HBM-roofline kernels) */
	float color_dwt_ms;   /* quality 1..16: the colour + 4:2:0 kernel, the first of the front group; 0 for 17..23 (the conversion is inside the fused front kernel) */
	float luma_ms;        /* luma tail up to and including the luma quantiser and Y31; the chroma sequence runs next to it on a stream of its own and -- the default since round 5 -- is joined IN FRONT of the luma quantiser, so this figure includes any wait for it (NHW_CHROMA_FORK=0: the chroma sequence follows behind) */
	float chroma_ms;      /* what is left of the chroma sequence once the luma tail is done: about 0 with the default join in front of the quantiser (NHW_QUANT_JOIN=0: the join in front of the packetiser, where this is the exposed rest; NHW_CHROMA_FORK=0: its full time) */
	float entropy_ms;
	int parts;            /* sub-batches the stages behind the front ran as (each on a stream of its own); with more than one, luma/chroma/entropy_ms are those of the first */
	int front_images;     /* images covered by front_ms */
	float prefilter_ms;   /* quality 1..16: the rationed luma pre-filter (k_low_pre, k_low_mapfix, k_low_chain, k_low_apply, k_low_markrows, k_low_marks), second of the front group; 0 for 17..23 */
} nhw_timing;

/* lifecycle: replaces `im.setup=malloc(..)` + per-image mallocs of encode_image (nhw_encoder.c:108-...).  Everything a batch of up to
 * max_batch images needs on the device is allocated here and nowhere else: the workspace (7.4 MB per image) and the staging buffers of the
 * host path nhw_enc_batch / nhw_enc_synth_batch (1.8 MB per image) -- no call behind it allocates, so the first batch costs what the others do */
int  nhw_enc_create(int device, int max_batch, nhw_enc **out);
/* The same with flags.  NHW_CREATE_DEVICE_ONLY: for callers of nhw_enc_batch_device only -- the host path's staging buffers (1.8 MB per image:
 * 7.3 GB at max_batch 4096) are not allocated; a later nhw_enc_batch / nhw_enc_synth_batch on such a handle still works and allocates them
 * then (that one call pays for it).  Unknown flag bits are NHW_E_ARG. */
#define NHW_CREATE_DEVICE_ONLY 1u
int  nhw_enc_create_ex(int device, int max_batch, unsigned flags, nhw_enc **out);
void nhw_enc_destroy(nhw_enc *e);
const char *nhw_last_error(void);
int  nhw_quality_supported(int quality);

/* What the reference's out-of-bounds reads return.  NHW_COMPAT_CANONICAL (default, normative): zeros -- the output equals the reference
 * sources built with a zero-filling guard allocator.  NHW_COMPAT_GLIBC_ONESHOT: the heap neighbours of the stock `gcc -O3` nhw-enc run on
 * one image per process -- the output equals that binary's, except for the bytes it leaves un-initialised itself (the
 * last byte of the res1/res5/res6 word sections and of the two select-word and code-book sections, the last two of res3's). */
enum { NHW_COMPAT_CANONICAL = 0, NHW_COMPAT_GLIBC_ONESHOT = 1 };
int  nhw_enc_set_compat(nhw_enc *e, int mode);

/* Encode n images already resident in HBM.  d_bgr: n*NHW_IMG_BYTES.  d_out: n*NHW_OUT_STRIDE, image i's
 * .nhw starts at i*NHW_OUT_STRIDE.  d_sizes[i] = byte length, d_status[i] = NHW_OK / NHW_E_CODEBOOK.
 * Asynchronous on `stream`. */
int nhw_enc_batch_device(nhw_enc *e, const void *d_bgr, int n, int quality, void *d_out, uint32_t *d_sizes,
                         int32_t *d_status, void *stream);

/* Host convenience: H2D, encode, compact, D2H.  out_off has n+1 entries; image i is
 * out_arena[out_off[i] .. out_off[i+1]).  status has n entries.  Synchronous. */
int nhw_enc_batch(nhw_enc *e, const uint8_t *bgr, int n, int quality, uint8_t *out_arena, size_t arena_cap,
                  uint64_t *out_off, int32_t *status);

/* SURVEY.md section 8d synthetic inputs generated on the device (image i gets seed seed_base+i). */
int nhw_synth_batch_device(nhw_enc *e, void *d_bgr, int n, uint32_t seed_base, void *stream);
/* the same images generated on the device, encoded, and the .nhw files brought to the host like nhw_enc_batch does (`nhw-enc --synthetic`) */
int nhw_enc_synth_batch(nhw_enc *e, int n, uint32_t seed_base, int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status);

/* page-locked host memory for nhw_enc_batch's input (DMA at PCIe speed, overlapped with the encode of the chunk before), and the number
 * of GPUs this process sees (one encoder handle per device, e.g. one host thread each: tools/nhw_enc.c --gpus) */
void *nhw_host_alloc(size_t bytes);
void  nhw_host_free(void *p);
int   nhw_device_count(void);

int nhw_enc_last_timing(nhw_enc *e, nhw_timing *t);

/* ---- encode to a byte budget: a per-image quality search on the device ----
 * ladder: host array of ladder_len (1..23) distinct qualities 1..23, tried in order; NULL (with ladder_len 0) = 23, 22, ..., 1.
 * For every image the result is the .nhw file of the FIRST rung whose encode succeeds (NHW_OK) with a size <= that image's budget,
 * byte-identical to what nhw_enc_batch_device gives for the image at that quality; d_quality[i] = that quality.  A rung where the image
 * reports NHW_E_CODEBOOK does not fit and the search goes on down the ladder.  The search is exact: file size is not monotonic in
 * quality, and no rung is skipped on a guess.  If no rung fits, slot i holds the outputs of the LAST rung (file, size, quality) with
 * status NHW_E_BUDGET -- or NHW_E_CODEBOOK and size 0 if that rung overflowed the code book.
 * Each rung encodes only the images still open, as one batch at that rung's quality; rungs after the first gather those images out of
 * d_bgr (which must be 16-byte aligned) into a staging slab first.  The handle's compat mode applies to every rung.
 * d_max_bytes: n budgets in device memory (indexed like the images); d_out / d_sizes / d_status / d_quality as in nhw_enc_batch_device.
 * Bad arguments are refused before anything is launched: a duplicate or out-of-range ladder entry NHW_E_QUALITY; NULL pointers, n outside
 * 1..max_batch, ladder_len outside 0..23 (0 only with ladder NULL), a handle with nhw_debug_stop_after set, or a stream being captured
 * NHW_E_ARG.
 * NOT asynchronous: after every rung but the last the call waits on `stream` for the number of images still open (the search stops when
 * it reaches 0), so it cannot be captured in a graph.  After it, nhw_enc_last_timing and nhw_stage_chroma_l1 see the last rung's encode.
 * The first fit call on a handle allocates the search's buffers for max_batch images (1.3 MB per image: a staging input and output slot);
 * that one call pays for it, later ones do not allocate. */
int nhw_enc_fit_batch_device(nhw_enc *e, const void *d_bgr, int n, const uint32_t *d_max_bytes, const int *ladder, int ladder_len,
                             void *d_out, uint32_t *d_sizes, int32_t *d_status, int32_t *d_quality, void *stream);
/* host convenience: H2D of the images and budgets (max_bytes: n entries, host), the search, then the files compacted and brought back
 * like nhw_enc_batch does (out_off n+1 entries; status, quality n entries).  Synchronous. */
int nhw_enc_fit_batch(nhw_enc *e, const uint8_t *bgr, int n, const uint32_t *max_bytes, const int *ladder, int ladder_len,
                      uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality);
/* the last fit call: rungs run, the quality and the number of images encoded at each rung (ladder order), and the wall time between
 * its first and its last event on the stream */
typedef struct { int rungs; int quality[23]; int images[23]; float total_ms; } nhw_fit_stats;
int nhw_enc_last_fit_stats(nhw_enc *e, nhw_fit_stats *s);

/* ---- distortion: the sum of squared differences (SSE) over all NHW_IMG_BYTES bytes of a picture, B, G and R together ----
 * d_a, d_b: n pictures each (n*NHW_IMG_BYTES bytes, 16-byte aligned); d_sse[i] = the exact SSE of picture i of d_a against picture i of
 * d_b (at most 786432 * 255^2, beyond 32 bits).  PSNR = 10 log10(255^2 * 786432 / SSE).  No handle: the launch goes to the calling
 * thread's current device; stream NULL is the null stream.  Asynchronous, and may be captured in a graph.  NHW_E_ARG for NULL pointers,
 * n outside 1..65535, unaligned pictures or a d_sse that is not 8-byte aligned. */
int nhw_sse_batch_device(const void *d_a, const void *d_b, int n, uint64_t *d_sse, void *stream);

/* ---- encode to a distortion budget: a per-image quality search on the device, with a decode and an error pass per rung ----
 * The byte-budget search's walk (above) with a different test for "fits".  ladder: as there, but NULL (with ladder_len 0) = 1, 2, ..., 23,
 * so by default the answer is the lowest quality that reaches the target.  d_max_sse: n targets in device memory.  For every image the
 * result is the .nhw file of the FIRST rung whose encode returns NHW_OK and whose decode (by the decoder handle d, the device decoder
 * that is bit-exact against the reference's) returns NHW_OK with an SSE against the input picture <= d_max_sse[i]; the file is
 * byte-identical to what nhw_enc_batch_device gives at that quality, d_quality[i] = that quality and d_sse[i] = that SSE.  Neither the
 * PSNR nor the size is monotonic in quality, so no rung is skipped on a guess.  If no rung meets the target, slot i holds the LAST rung's
 * outputs (file, size, quality, SSE) with status NHW_E_BUDGET -- NHW_E_CODEBOOK, size 0 and SSE UINT64_MAX if that rung overflowed the
 * code book, NHW_E_FORMAT (SSE UINT64_MAX) if the decoder refused the encoder's file.
 * Per rung: the open images are encoded as one batch, the rung's files decoded as one batch by d on `stream` into a buffer of the
 * search, the SSE of every open image computed, and the images that meet their target closed.  Arguments are refused as for
 * nhw_enc_fit_batch_device, with the same codes, and NHW_E_ARG also when d is NULL, d's max_batch is below n, d is on another device than
 * e, or d has a debug stop set.  NOT asynchronous: the call waits on `stream` after every rung but the last, so it cannot be captured in
 * a graph.  After it, nhw_enc_last_fit_stats describes it as for the byte search, nhw_enc_last_timing sees the last rung's encode and
 * nhw_dec_last_timing the last rung's decode.  The first call of this kind on a handle allocates, besides the byte search's buffers, a
 * decoded picture per image for max_batch images (0.75 MB each); byte-budget callers never allocate it. */
int nhw_enc_fit_sse_batch_device(nhw_enc *e, nhw_dec *d, const void *d_bgr, int n, const uint64_t *d_max_sse, const int *ladder, int ladder_len,
                                 void *d_out, uint32_t *d_sizes, int32_t *d_status, int32_t *d_quality, uint64_t *d_sse, void *stream);
/* host convenience: H2D of the images and targets (max_sse: n entries, host), the search, then the files compacted and brought back like
 * nhw_enc_batch does (out_off n+1 entries; status, quality, sse n entries).  Synchronous. */
int nhw_enc_fit_sse_batch(nhw_enc *e, nhw_dec *d, const uint8_t *bgr, int n, const uint64_t *max_sse, const int *ladder, int ladder_len,
                          uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality, uint64_t *sse);

/* ---- pictures of any size as padded 512 x 512 tiles ----
 * A picture is W x H pixels (1 <= W, H <= 65535), 3 bytes a pixel (B, G, R), rows in BMP file order.  It is padded to 512 nx x 512 ny
 * (nx = ceil(W / 512), ny = ceil(H / 512)) by edge replication: padded pixel (r, c) = picture pixel (min(r, H - 1), min(c, W - 1)).
 * Tile (ty, tx) is padded rows 512 ty .. and columns 512 tx .., index ty nx + tx; every tile is encoded as an ordinary 512 x 512 image.
 * Descriptor of a picture in device memory: addr = device address of its first byte (any alignment), pitch = bytes from one row to the
 * next (>= 3 W, any value), first_tile = global number of its first tile (first_tile[k + 1] = first_tile[k] + tiles(k)), reserved 0. */
typedef struct { uint64_t addr, pitch; uint32_t width, height, first_tile, reserved; } nhw_picture;   /* 32 bytes */
/* nx * ny, or NHW_E_ARG for a side outside 1..65535 */
int nhw_picture_tiles(uint32_t width, uint32_t height);
/* The global tiles [tile0, tile0 + m) of the pictures d_pics[0 .. n_pics) (a table in device memory, the caller's responsibility), tile t
 * padded into d_tiles + (t - tile0) * NHW_IMG_BYTES (16-byte aligned); untile: the inverse, from decoded tiles it writes exactly the
 * pictures' bytes (not the bytes between rows, nothing outside the pictures).  No handle: the current device; stream NULL is the null
 * stream.  Asynchronous, and may be captured in a graph.  NHW_E_ARG for NULL pointers, n_pics < 1, m < 1, tile0 < 0, an unaligned d_tiles.
 * A tile of the range that no picture of the table holds -- one below the table's first tile, one past its last, or one of an entry with a
 * zero side (which may share its successor's first_tile) -- is passed over: nothing is written for it, and nhw_sse_pictures_device adds nothing. */
int nhw_tile_pictures_device(const nhw_picture *d_pics, int n_pics, int tile0, int m, void *d_tiles, void *stream);
int nhw_untile_pictures_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, void *stream);
/* The .nhwp container (version 1, little-endian): "NHWP", version 1, 3 zero bytes, W (4 bytes), H (4), T = nx ny tile lengths (4 each,
 * 1 .. NHW_OUT_STRIDE, tile order), then the T .nhw files back to back; exactly 16 + 4 T + the sum of the lengths bytes.  A .nhw file
 * starts with a byte <= 6, so a stock decoder refuses a container ("Not an .nhw file").  nhw_picture_info: NHW_OK and W, H for a
 * well-formed container, else NHW_E_FORMAT. */
int nhw_picture_info(const uint8_t *container, size_t len, uint32_t *width, uint32_t *height);
/* Host convenience, synchronous: n packed pictures (pitch 3 W), picture i at bgr + in_off[i] with width[i] x height[i] pixels, padded and
 * tiled on the device in chunks of at most max_batch tiles, encoded at `quality`; picture i's container is out_arena[out_off[i] ..
 * out_off[i + 1]) (out_off: n + 1 entries; NHW_E_SPACE if arena_cap is short).  status[i] = NHW_OK or the first failing tile's status
 * (NHW_E_CODEBOOK); a failed picture gets an empty container.  NHW_E_ARG for a bad argument or a side outside 1..65535. */
int nhw_enc_pictures(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                     int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status);

/* ---- pictures of any size to a byte budget or a PSNR target ----
 * The error of decoded tiles against the pictures' own bytes: adds to d_sse[k] the SSE between the decoded tiles [tile0, tile0 + m)
 * (d_tiles, tile t at (t - tile0) * NHW_IMG_BYTES, 16-byte aligned) and the bytes of picture k of d_pics that those tiles cover: tile row
 * rr of tile (ty, tx) against picture row 512 ty + rr < H, bytes [1536 tx, min(1536 tx + 1536, 3W)).  Padding never counts.  Accumulates
 * (the caller zeroes d_sse), so chunked calls add up; exact, independent of scheduling; asynchronous and capturable.  NHW_E_ARG as for
 * nhw_untile_pictures_device, and for a d_sse not 8-byte aligned.  PSNR of a picture = 10 log10(65025 * 3 W H / SSE). */
int nhw_sse_pictures_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, void *stream);
/* Host conveniences, synchronous; inputs and outputs as for nhw_enc_pictures, plus the ladder (as for nhw_enc_fit_batch /
 * nhw_enc_fit_sse_batch: NULL with ladder_len 0 = 23, 22, ..., 1 for bytes, 1, 2, ..., 23 for SSE), the limits (host arrays of n) and
 * quality (n), sse (n).  All tiles of a picture get ONE quality.  Picture i's result is the container of the FIRST rung whose test it
 * passes, byte-identical to what nhw_enc_pictures writes for it at that quality:
 *   bytes: every tile encodes NHW_OK and the container (16 + 4 T + the sum of the tile lengths) is at most max_bytes[i] bytes;
 *   SSE:   every tile encodes NHW_OK, every tile decodes NHW_OK by d, and the SSE over the picture's own 3 W H bytes (the decoded tiles
 *          cropped, against the input: what a user measures between nhw_dec_pictures(container) and the input) is at most max_sse[i].
 * Size and PSNR are not monotonic in quality: the walk goes rung by rung and skips none; a picture closes at its first passing rung and
 * later rungs encode only the tiles of the pictures still open.  If no rung passes, the picture gets the last rung's container, quality and
 * SSE with status NHW_E_BUDGET -- NHW_E_CODEBOOK, an empty container and SSE UINT64_MAX if a tile of that rung overflowed the code book,
 * NHW_E_FORMAT (SSE UINT64_MAX) if the decoder refused one of its tiles.
 * Refused before anything is launched: a bad ladder NHW_E_QUALITY; NULL pointers, n < 1, a side outside 1..65535, a debug stop on either
 * handle, a decoder on another device or with a max_batch below min(e's max_batch, the call's tiles) NHW_E_ARG.  NHW_E_SPACE if arena_cap
 * is short.  After a call nhw_enc_last_fit_stats gives rungs and quality[r] as for the image searches, images[r] = the number of TILES
 * encoded at rung r, and total_ms from the upload of the pictures to the end of the last rung.  The SSE search allocates (grow-only) a
 * decoded tile for each of min(max_batch, tiles) tiles, not the image searches' buffers. */
int nhw_enc_fit_pictures(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                         const uint64_t *max_bytes, const int *ladder, int ladder_len,
                         uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality);
int nhw_enc_fit_sse_pictures(nhw_enc *e, nhw_dec *d, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height,
                             int n, const uint64_t *max_sse, const int *ladder, int ladder_len,
                             uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status, int32_t *quality, uint64_t *sse);

/* ---- a rectangle of a picture from only the tiles it touches ----
 * A region of a W x H picture is a rectangle x, y, width, height (width, height >= 1, x + width <= W, y + height <= H) in the coordinates
 * of the array nhw_dec_pictures returns (row 0 = its first row, BMP file order); its result is that array's rows y .. y + height - 1,
 * columns x .. x + width - 1, byte for byte.  It is made from the selected tiles only: columns x / 512 .. (x + width - 1) / 512 times rows
 * y / 512 .. (y + height - 1) / 512 of the picture's tile grid, in row-major order (ty, then tx).
 * Descriptor of a region in device memory: addr = device address of its first destination byte (any alignment), pitch = bytes from one
 * destination row to the next (>= 3 width, any value), first_tile = running number of the region's first selected tile within the call
 * (first_tile[k + 1] = first_tile[k] + nhw_region_tiles(k)), reserved 0. */
typedef struct { uint64_t addr, pitch; uint32_t x, y, width, height, pic_width, pic_height, first_tile, reserved; } nhw_region;   /* 48 bytes */
/* the number of tiles the region selects, or NHW_E_ARG for a picture side outside 1..65535, an empty rectangle or one not inside the picture */
int nhw_region_tiles(uint32_t pic_width, uint32_t pic_height, uint32_t x, uint32_t y, uint32_t width, uint32_t height); /* count, or NHW_E_ARG */
/* d_tiles holds the decoded tiles [tile0, tile0 + m) of the running selection of the regions d_regs[0 .. n_regs) (a table in device memory,
 * the caller's responsibility), NHW_IMG_BYTES each, 16-byte aligned.  Of selected tile (ty, tx), tile row rr is picture row 512 ty + rr;
 * if y <= 512 ty + rr < y + height, its picture columns [max(512 tx, x), min(512 tx + 512, x + width)) go to destination byte 3 (col - x)
 * of row 512 ty + rr - y.  Writes exactly the regions' bytes: never a byte outside [addr + r pitch, addr + r pitch + 3 width) of a row r,
 * never a read-modify-write (two regions may share destination dwords, not bytes).  No handle: the current device; stream NULL is the null
 * stream.  Asynchronous, and may be captured in a graph.  NHW_E_ARG as for nhw_untile_pictures_device. */
int nhw_untile_regions_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, int tile0, int m, void *stream);

/* ---- stage-level entry points (kernel parity tests; same stream rules) ----
 * colour + 4:2:0 (colorspace.c:55-260), any quality 1..23: d_y n*262144 int16, d_u/d_v n*65536 uint8 */
int nhw_stage_color(nhw_enc *e, const void *d_bgr, int n, int quality, void *d_y, void *d_u, void *d_v, void *stream);
/* luma pre-filter (image_processing.c:558-2426) as a stage of its own: quality 1..16 (k_low_pre .. k_low_marks, the kernels the encoder runs, the whole batch in line);
 * for 17..21 it is a step inside the fused front kernel (NHW_E_QUALITY here).  In place on d_y */
int nhw_stage_prefilter(nhw_enc *e, void *d_y, int n, int quality, void *stream);
/* one analysis level (wavelet_filterbank.c:52-302) on planes of `stride` shorts per row, n_img images
 * spaced plane_stride shorts apart; size = transform size; final_level as in the oracle.
 * Size 256 / 128: any `short` input (blocks whose second pass would leave 16 bits take a 32-bit path that follows the reference's `int`
 * accumulators).  Size 512 is the encoder's level-1 kernel, built for luma, and has a DOMAIN: with U = the largest sample of the planes
 * (0 if none is positive) and L = minus the smallest (0 if none is negative),
 *       104 U + 40 L <= NHW_ANA512_BOUND   and   104 L + 40 U <= NHW_ANA512_BOUND
 * (the 2-D low-pass is the outer product of [-1 2 6 2 -1]: positive weights 104, negative 40; 47 below 32767 for the error-diffusion
 * carry and the rounding offset of filters.c:246-276; proof: nhwcodec_amd/csrc/nhw_front_image.h).  E.g. L = 4 allows U <= 313, L = 0
 * U <= 314; the encoder's luma is 0..255 plus at most +-4 of its pre-filters.  Planes outside the domain are refused with NHW_E_ARG
 * (a synchronising check on the stream): the entry point never returns a plane that differs from the reference's wavelet_analysis(). */
#define NHW_ANA512_BOUND 32720
int nhw_stage_analysis(nhw_enc *e, void *d_jpeg, void *d_proc, int n_img, size_t plane_stride, int stride, int size,
                       int final_level, void *stream);
int nhw_stage_synthesis(nhw_enc *e, void *d_jpeg, void *d_proc, int n_img, size_t plane_stride, int stride, int size,
                        void *stream);
/* the two chroma level-1 analyses (nhw_encoder.c:2265, 2576) as the encoder launches them for quality >= 15, on the 4:2:0 planes of the handle's
 * last batch (a measurement hook: bench.py adds their time to the fused front kernel's).  The launches are ordered behind that batch; NHW_E_ARG
 * when the handle's last whole batch had fewer than n images or a quality below 15 (nothing it could work on); it overwrites the chroma
 * work planes, so it belongs between batches */
int nhw_stage_chroma_l1(nhw_enc *e, int n, void *stream);

/* ---- decoder (BASELINE config 5): replaces decode_image + write_image_bmp (decoder/codec.h:184-186,
 * decoder/nhw_decoder.c:54, decoder/nhw_decoder_cli.c:108), one launch sequence per batch of files ----
 * d_nhw: an arena in HBM holding the .nhw files, file i at d_off[i] with d_len[i] bytes (device arrays; the encoder's output
 * arena is such an arena with d_off[i] = i*NHW_OUT_STRIDE and d_len = d_sizes).  d_bgr: n*NHW_IMG_BYTES,
 * the pixel bytes in the order nhw-dec writes them behind its 54-byte header (nhw_dec_bmp_header).  d_status[i] =
 * NHW_OK / NHW_E_FORMAT, d_quality[i] (may be NULL) = the quality setting stored in file i.  Asynchronous on `stream`. */
int  nhw_dec_create(int device, int max_batch, nhw_dec **out);
void nhw_dec_destroy(nhw_dec *d);
const char *nhw_dec_last_error(void);
int nhw_dec_batch_device(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, void *d_bgr, int32_t *d_status,
                         int32_t *d_quality, void *stream);
/* host convenience: H2D of the files (nhw[off[i]..off[i+1])), decode, D2H.  Synchronous.  NHW_E_ARG for n > max_batch and for an off[] that decreases. */
int nhw_dec_batch(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, uint8_t *bgr, int32_t *status, int32_t *quality);
void nhw_dec_bmp_header(uint8_t h[54]);
/* host convenience for .nhwp containers, synchronous: container i is blob[off[i] .. off[i + 1]) (off: n + 1 entries); its tiles are
 * decoded in chunks of max_batch, cropped on the device, and picture i (W x H x 3 bytes, pitch 3 W) lands at bgr + out_off[i] (n entries).
 * status[i] = NHW_OK, or NHW_E_FORMAT for a malformed container or a tile the decoder refuses; that picture's bytes are left untouched. */
int nhw_dec_pictures(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, uint8_t *bgr, const uint64_t *out_off, int32_t *status);
/* ---- regions of .nhwp containers: host conveniences, synchronous ----
 * Containers as for nhw_dec_pictures (container c is blob[off[c] .. off[c + 1]), off: n_containers + 1 entries); rect i is a region of
 * container rects[i].container, and several rects may name one container.  Only the tile files the rects select are uploaded and decoded
 * (in chunks of max_batch, each chunk cropped on the device by k_untile_region); a tile selected by two rects is uploaded and decoded twice.
 * status[i] = NHW_OK; NHW_E_ARG for a container index out of range or a rectangle that is empty or not inside that picture; NHW_E_FORMAT
 * for a malformed container or a selected tile the decoder refuses.  A rect that is not NHW_OK does not disturb the others.
 * nhw_dec_regions: region i (width x height x 3 bytes, pitch 3 width) lands at bgr + out_off[i] (n_rects entries); a rect that is not
 * NHW_OK leaves its bytes untouched.
 * nhw_dec_regions_to_device: region i is cropped straight into device memory at dst_addr[i] with row pitch dst_pitch[i] (any alignment,
 * any pitch >= 3 width: e.g. slot i of an [n, h, w, 3] batch tensor); no pixels are downloaded.  A rect that is NHW_E_ARG or names a
 * malformed container leaves its destination untouched; one that fails on a refused tile may have had bytes of its own rows written by its
 * other tiles, never a byte outside them.
 * The call itself fails (NHW_E_ARG) only for NULL pointers, counts < 1, a decreasing off[], a dst_addr of 0, a dst_pitch below 3 width,
 * or more selected tiles than nhw_dec_pictures accepts. */
typedef struct { uint32_t container, x, y, width, height; } nhw_rect;
int nhw_dec_regions(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                    uint8_t *bgr, const uint64_t *out_off, int32_t *status);
int nhw_dec_regions_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                              const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status);
/* the last region call on the handle: the selected tiles that were handed to the decoder (those of the NHW_OK rects and of the rects that
 * failed on a refused tile) and the tile-file bytes uploaded for them.  After a window call (below): the UNIQUE tiles and the bytes of
 * exactly those files */
int nhw_dec_last_region_stats(nhw_dec *d, uint64_t *tiles_decoded, uint64_t *bytes_uploaded);
/* ---- decode at half or quarter scale straight from the wavelet pyramid ----
 * scale 1, 2 or 4; the tile side is T = 512 / scale and a file decodes to 3 T T bytes, in the byte order of the full decode.  Scale 1 is the
 * full decode.  Scale 2: Y = the level-1 low band of the luma (after its residual lists), U and V = the sharpened 4:2:0 planes, an exact 4:4:4
 * picture with no resampling; scale 4: Y = the level-2 low band, U and V = the chroma planes' level-1 low band after their corrections; both
 * through the file's own colour matrix, neither with the smoothing at the marks or the q > 21 level-1 corrections.  Scale 2 runs neither the
 * level-1 synthesis of the luma nor the mark search, scale 4 in addition none of level 2 of the luma, level 1 of the chroma and the sharpening.
 * nhw_dec_batch_device_scaled: the arguments of nhw_dec_batch_device plus scale; d_out holds n * 3 T T bytes, file after file, 8-byte aligned;
 * d_status and d_quality are exactly those of the full decode, and a refused file's bytes are left untouched.  NHW_E_ARG for any other scale
 * and for a scale of 2 or 4 on a handle with a debug stop set.  Asynchronous on `stream`; nhw_dec_last_timing describes it, recon_ms = the
 * kernel that writes the scaled pictures.  One handle serves full and scaled batches in any order. */
int nhw_dec_batch_device_scaled(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale, void *d_out,
                                int32_t *d_status, int32_t *d_quality, void *stream);
/* host convenience, synchronous: as nhw_dec_batch, for any n >= 1 (decoded in chunks of max_batch); file i lands at out + i * 3 T T */
int nhw_dec_batch_scaled(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality);
/* A W x H picture at scale s is ceil(W / s) x ceil(H / s): output pixel (r, c) is pixel (r % T, c % T) of the scaled decode of tile
 * (r / T, c / T).  The tile count does not change (ceil(ceil(W / s) / T) = ceil(W / 512)); where W or H is no multiple of s the last column or
 * row comes from the edge-replicated padding.  NHW_E_ARG for a side outside 1..65535 or a scale other than 1, 2, 4. */
int nhw_picture_scaled_size(uint32_t width, uint32_t height, int scale, uint32_t *scaled_width, uint32_t *scaled_height);
/* nhw_untile_pictures_device for the tiles of a scaled decode: tile t at d_tiles + (t - tile0) * 3 T T, and the table describes the
 * DESTINATION: the scaled width, height and pitch of every picture.  Same rules otherwise; NHW_E_ARG also for a scale other than 1, 2, 4. */
int nhw_untile_pictures_scaled_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int n_tiles, int scale, void *stream);
/* nhw_dec_pictures at a scale: picture i (ceil(W / scale) x ceil(H / scale) x 3 bytes, packed) lands at out + out_off[i] */
int nhw_dec_pictures_scaled(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, int scale, uint8_t *out, const uint64_t *out_off, int32_t *status);
/* ---- windows: rectangles of .nhwp pictures at scale 1, 2 or 4, every tile decoded once ----
 * A window of a W x H picture at scale s is a rectangle x, y, width, height (width, height >= 1, x + width <= W', y + height <= H') in the
 * coordinates of the scaled picture W' x H' = ceil(W / s) x ceil(H / s), the array nhw_dec_pictures_scaled returns at that scale (scale 1:
 * nhw_dec_pictures); its result is that array's rows y .. y + height - 1, columns x .. x + width - 1, byte for byte.  With T = 512 / s it
 * selects tile columns x / T .. (x + width - 1) / T times tile rows y / T .. (y + height - 1) / T of the picture's ordinary tile grid.
 * nhw_window_tiles: the FULL picture's sides and a window in scaled coordinates -> the window's own tile count, or NHW_E_ARG for a side
 * outside 1..65535, a scale other than 1, 2, 4, an empty rectangle or one not inside the scaled picture.  At scale 1 it is nhw_region_tiles. */
int nhw_window_tiles(uint32_t pic_width, uint32_t pic_height, int scale, uint32_t x, uint32_t y, uint32_t width, uint32_t height);
/* A use: tile (ty, tx) of the picture's grid, decoded into slot `slot` of the call's unique tiles, feeds window `region` of the table. */
typedef struct { uint32_t region, slot, tx, ty; } nhw_window_use;   /* 16 bytes */
/* The crop alone.  d_tiles holds the decoded tiles of the slots [tile0, tile0 + m), 3 T T bytes each (T = 512 / scale), 16-byte aligned;
 * d_regs[0 .. n_regs) are nhw_region descriptors with x, y, width, height in scaled coordinates and pic_width, pic_height the SCALED
 * picture's sides (first_tile is not read); d_uses[0 .. n_uses) the (window, tile) pairs, in any order.  Of a use, tile row rr is
 * scaled-picture row T ty + rr; if y <= T ty + rr < y + height, its columns [max(T tx, x), min(T tx + T, x + width)) go to destination byte
 * 3 (col - x) of row T ty + rr - y.  Writes exactly those bytes: never a byte outside [addr + r pitch, addr + r pitch + 3 width) of a window
 * row r, never a read-modify-write.  A use is passed over, nothing stored, when its region is >= n_regs, its slot outside [tile0, tile0 + m),
 * its (tx, ty) outside the window's selection, or its descriptor no window of a picture (a zero side, a scaled side above ceil(65535 / scale),
 * x + width or y + height beyond the side).  Several uses may share a slot, and a table may hold the uses of other chunks.  No handle: the
 * current device; stream NULL is the null stream.  Asynchronous, and may be captured in a graph.  NHW_E_ARG for NULL pointers, n_regs < 1,
 * n_uses < 1, m < 1, tile0 < 0, an unaligned d_tiles, a scale other than 1, 2, 4. */
int nhw_untile_windows_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses,
                              int tile0, int m, int scale, void *stream);
/* Host conveniences, synchronous: nhw_dec_regions / nhw_dec_regions_to_device for windows, all of one call at one scale.  The tiles of a call
 * are the UNION of its windows' selections: a tile of a container is uploaded and decoded once, however many windows select it, and no other
 * tile file is uploaded, decoded or looked at (but for the well-formedness check of the container).  Containers, rects, bgr / out_off,
 * dst_addr / dst_pitch, the per-rect statuses and the call-level NHW_E_ARG cases are those of the region calls, with the rectangle checked
 * against the scaled picture; NHW_E_ARG also for a scale other than 1, 2, 4, and at scales 2 and 4 for a handle with a debug stop set.  A
 * window's status depends on its selected tiles alone: a tile the decoder refuses fails exactly the windows that select it (NHW_E_FORMAT).
 * After a window call nhw_dec_last_region_stats reports the UNIQUE tiles handed to the decoder and the bytes of exactly those files. */
int nhw_dec_windows(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                    uint8_t *bgr, const uint64_t *out_off, int32_t *status);
int nhw_dec_windows_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                              const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status);
/* ---- decode straight into training tensors ----
 * The form the pixels leave the decoder in.  The byte entry points above write uint8 [S][S][3], B, G, R a pixel, rows in BMP file order; a
 * tensor format names another element type, plane layout, channel order and row direction, and a scale and a bias per output channel.
 *   dtype     NHW_T_U8, NHW_T_F16 (IEEE binary16), NHW_T_BF16 (bfloat16) or NHW_T_F32
 *   layout    NHW_T_HWC: [S][S][3], as the byte path; NHW_T_CHW: [3][S][S]
 *   channels  NHW_T_BGR: output channel 0 is the byte path's byte 0 of a pixel (blue in a BMP file), as the byte path; NHW_T_RGB: channels 0
 *             and 2 change places
 *   rows      NHW_T_ROWS_FILE: as the byte path; NHW_T_ROWS_REVERSED: output row r is row S - 1 - r of the byte path's output.
 *             nhw_dec_bmp_header writes a POSITIVE height (512), and a BMP file with a positive height holds its rows bottom-up: the byte
 *             path's row 0 is the picture's bottom row.  NHW_T_ROWS_REVERSED is therefore the top-down picture, row 0 = its top row, which
 *             is what an image tensor usually is; NHW_T_ROWS_FILE is the bottom-up one.
 *   scale[3], bias[3]   indexed by OUTPUT channel position (with NHW_T_RGB, index 0 belongs to R)
 *   reserved  must be 0
 * The value rule: for NHW_T_F16, NHW_T_BF16 and NHW_T_F32 the element for byte b of output channel c is fmaf((float) b, scale[c], bias[c])
 * in single precision, rounded ONCE, to nearest even, to the output type.  That rounding follows the fma's own, of the exact sum to float32:
 * two roundings in all, and the two-step value is the rule.  Subnormals are kept and what lies beyond the range is an infinity, in float32
 * and in the output type.  A value that is not zero keeps its sign where it rounds to zero; an exact sum of zero is +0, except that a zero
 * product of negative sign (b = 0 or a scale of 0, under a scale below zero or -0) plus a bias of -0 is -0.  For NHW_T_U8 scale must be 1 and
 * bias 0, and the bytes go out unchanged.
 * A format is refused with NHW_E_ARG, before anything is launched, for an unknown enum value, a non-zero reserved word, a scale or bias that is
 * not finite, or NHW_T_U8 with another scale or bias. */
enum { NHW_T_U8 = 0, NHW_T_F16 = 1, NHW_T_BF16 = 2, NHW_T_F32 = 3 };
enum { NHW_T_HWC = 0, NHW_T_CHW = 1 };
enum { NHW_T_BGR = 0, NHW_T_RGB = 1, NHW_T_GREY = 2 };   /* NHW_T_GREY: one channel; taken by the grey decode and the grey calls alone (DESIGN.md sections 22 and 23, below) */
enum { NHW_T_ROWS_FILE = 0, NHW_T_ROWS_REVERSED = 1 };
typedef struct { int32_t dtype, layout, channels, rows; float scale[3], bias[3]; uint32_t reserved; } nhw_tensor_format;   /* 44 bytes */
/* nhw_dec_batch_device_scaled with a format: scale 1, 2 or 4 as there (S = 512 / scale), file i's tensor at d_out + i * 3 * S * S *
 * sizeof(dtype); d_status and d_quality are those of the full decode, and a refused file leaves its slot untouched.  The entropy stages and
 * every kernel up to the last are the byte path's, launched as there; the last kernel (k_dec_final, k_dec_scaled<S>) stores the format
 * straight from the registers that hold R, G and B.  The format NHW_T_U8 / NHW_T_HWC / NHW_T_BGR / NHW_T_ROWS_FILE is the byte path itself.
 * NHW_E_ARG, before anything is launched: a refused format, a d_out that is not 16-byte aligned, a handle with a debug stop set, and the
 * cases of nhw_dec_batch_device_scaled.  Asynchronous on `stream`; one handle serves byte and tensor calls in any order. */
int nhw_dec_batch_device_tensor(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale,
                                const nhw_tensor_format *fmt, void *d_out, int32_t *d_status, int32_t *d_quality, void *stream);
/* The same formats for what is already bytes (the outputs of the picture, region and window calls): picture k of the table d_pics[0 ..
 * n_pics) (as for nhw_tile_pictures_device: any W x H, pitch and alignment; first_tile is not read) goes, under the same rule, to a tensor of
 * its own size -- [H][W][3] or [3][H][W] elements, packed -- at the device address d_out_addr[k] (a device array of n_pics addresses, each a
 * multiple of the element size).  Reads exactly the pictures' bytes, never those between rows or beyond a picture.  An entry with a zero
 * side, a side above 65535 or a misaligned address is passed over: nothing is written for it.  No handle: the current device; stream NULL is
 * the null stream.  Asynchronous, and may be captured in a graph.  NHW_E_ARG for NULL pointers, n_pics outside 1 .. 2^24 and a refused format. */
int nhw_bytes_to_tensor_device(const nhw_picture *d_pics, int n_pics, const nhw_tensor_format *fmt, const uint64_t *d_out_addr, void *stream);
/* ---- crops resized into tensors of one size: crop, resize, flip ----
 * A crop at scale s (1, 2 or 4) is a window of that scale (above) plus an output size out_width x out_height (1 .. 4096 each, one size for all
 * crops of a call) and a flag byte whose bit 0 means "mirror left-right".  With P the window's bytes -- uint8 [h][w][3], B, G, R a pixel, rows
 * in file order -- the result is defined from P alone, in integers:
 *   position of output index o along an axis of source length n and output length m, in 64-bit integers:
 *     t = max((2 o + 1) n - m, 0),  X = min(floor(128 t / m), 256 (n - 1)),  i0 = X >> 8,  f = X & 255,  i1 = min(i0 + 1, n - 1)
 *     (the centre-aligned (o + 1/2) n / m - 1/2, clamped to the axis, in 1/256 pixel);
 *   byte of output pixel (oy, ox), channel c, with (y0, y1, fy) from (oy, h, out_height) and (x0, x1, fx) from (ox, w, out_width):
 *     ((256 - fx)(256 - fy) P[y0][x0][c] + fx (256 - fy) P[y0][x1][c] + (256 - fx) fy P[y1][x0][c] + fx fy P[y1][x1][c] + 32768) >> 16;
 *   the picture R of these bytes, uint8 [out_height][out_width][3], is mirrored left-right (R[oy][out_width - 1 - ox]) when the flag is set;
 *   the tensor is what nhw_bytes_to_tensor_device makes of R under the format: its value rule, channel order, row direction and layout.
 * The filter has two taps a direction: it is meant for reductions below 2, which nhw_crop_scale arranges whenever the crop is at least as
 * large as the output; larger reductions alias as bilinear interpolation does.
 * nhw_crop_scale: the scale to decode a width x height crop at -- the largest s of 4, 2, 1 with s out_width <= width and s out_height <=
 * height, 1 if there is none; NHW_E_ARG for a zero side or an output side above 4096.  A crop x, y, w, h in FULL-resolution coordinates,
 * inside a W x H picture, becomes the window at scale s
 *     x' = floor(x / s),  y' = floor(y / s),  w' = ceil((x + w) / s) - x',  h' = ceil((y + h) / s) - y',
 * the smallest scaled window that covers it; it lies inside ceil(W / s) x ceil(H / s). */
int nhw_crop_scale(uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height);   /* 1, 2 or 4; NHW_E_ARG on a zero or an output side above 4096 */
/* The resize alone, the counterpart of nhw_bytes_to_tensor_device: picture k of the table d_pics[0 .. n) (addr, pitch, width and height are
 * read; any alignment and pitch; bytes outside a row's 3 width are never read) goes, under the rule above with P the picture, to the
 * [out_height][out_width][3] or [3][out_height][out_width] elements at d_out_addr[k]; d_flags: n flag bytes in device memory, or NULL for
 * none.  Writes exactly those 3 out_width out_height elements, element by element.  An entry with a zero side, a side above 65535, a zero
 * address or an address that is no multiple of the element size is passed over: nothing is written for it.  No handle: the current device;
 * stream NULL is the null stream.  Asynchronous, and may be captured in a graph.  NHW_E_ARG, before anything is launched, for NULL d_pics or
 * d_out_addr, n outside 1 .. 2^24, an output side outside 1 .. 4096 and a refused format. */
int nhw_resize_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
/* nhw_dec_windows_to_device with the resize behind it, synchronous: rects are windows at `scale`, flags (host memory, n_rects bytes, or NULL)
 * their flag bytes, dst_addr[i] the device address of crop i's tensor (e.g. slot i of an [n][3][out_height][out_width] batch).  Everything
 * nhw_dec_windows_to_device says holds: the union of tiles, each uploaded and decoded once; the per-rect statuses; nhw_dec_last_region_stats;
 * the call-level NHW_E_ARG cases, among them scale 2 or 4 on a handle with a debug stop -- with, in place of the pitch's, a dst_addr that is 0
 * or no multiple of the element size, an output side outside 1 .. 4096, a refused format and n_rects above 2^24.  The windows are cropped into
 * a staging buffer of the handle and resized from there by one launch behind the last chunk of tiles; nothing is downloaded.  A crop whose
 * status is not NHW_OK leaves its destination untouched. */
int nhw_dec_crops_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                            uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status);
/* ---- the area filter: shrink without aliasing ----
 * The two-tap rule above is right for reductions below 2.  The area rule is the same definition with other taps: P, the output size, the flag,
 * the mirror, the format and the layout are those of the section above, and each axis -- source length n (1 .. 65535), output length m
 * (1 .. 4096) -- gives output index o a list of taps (i, weight) and an axis total A, in integers:
 *   an axis that does not shrink (m >= n): the two taps above, (i0, 256 - f) and (i1, f), A = 256;
 *   an axis that shrinks (m < n): in units of 1 / m source pixel, source pixel i covers [i m, (i + 1) m) and output o covers [o n, (o + 1) n);
 *     the taps are i = floor(o n / m) .. ceil((o + 1) n / m) - 1 with weight min((i + 1) m, (o + 1) n) - max(i m, o n) -- every weight is 1 .. m,
 *     they sum to n, and A = n.  (o + 1) n <= 4096 x 65535 < 2^28;
 *   byte of output pixel (oy, ox), channel c: S = sum over y taps, x taps of wy wx P[y][x][c], D = Ay Ax, byte = floor((2 S + D) / (2 D)) -- the
 *     weighted mean rounded to nearest, halves up.  A row's sum of wx P is at most 255 x 65535 < 2^24; S <= 255 D < 2^40 and D < 2^32, so the sum
 *     over rows and the division are 64 bits wide;
 *   the reduction limit: n <= NHW_AREA_MAX_REDUCTION m on each axis (at most 129 taps an axis; a 65535-pixel side still reaches 512).
 * With out_width >= w and out_height >= h this is the two-tap rule bit for bit (D = 65536); with w = k out_width and h = k out_height it is the
 * k x k box mean floor((2 sum + k k) / (2 k k)).
 * nhw_area_to_tensor_device: nhw_resize_to_tensor_device under the area rule -- the same arguments, reads, writes, passed-over entries and
 * NHW_E_ARG cases, stream-ordered and capturable; an entry beyond the reduction limit on either axis is passed over as well: nothing is written
 * for it.
 * nhw_dec_crops_to_device_filter: nhw_dec_crops_to_device with the filter named.  NHW_FILTER_TWO_TAP is that call itself (the same path, bytes
 * and statistics); NHW_FILTER_AREA resizes the windows under the area rule; any other value is a call-level NHW_E_ARG.  With the area filter a
 * rect whose window is beyond the reduction limit for the call's output size gets status NHW_E_ARG: it selects no tile, its destination is not
 * written, and the other rects go on.
 * nhw_enc_pictures_resized: nhw_enc_pictures with the area rule in front -- n packed pictures of any sizes (as there) to n .nhwp containers of
 * out_width x out_height (1 .. 4096 each); container i is byte for byte what nhw_enc_pictures writes for the rule's picture of picture i (no
 * mirror) at that quality.  The pictures are uploaded, resized by one launch into a buffer of the handle, and tiled and encoded from there.
 * NHW_E_ARG, before anything is uploaded: the cases of nhw_enc_pictures, an output side outside 1 .. 4096 and a picture beyond the reduction
 * limit; NHW_E_QUALITY as there. */
#define NHW_FILTER_TWO_TAP 0
#define NHW_FILTER_AREA 1
#define NHW_AREA_MAX_REDUCTION 128
int nhw_area_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                              const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_to_device_filter(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status,
                                   int filter);
int nhw_enc_pictures_resized(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                             uint32_t out_width, uint32_t out_height, int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status);
/* ---- the cubic filter: a kernel with lobes ----
 * The Keys cubic with a = -1/2 (PIL's BICUBIC, torch's bicubic with antialias), its support widened with the reduction, as one integer rule.
 * P, the output size, the flag, the mirror, the format and the layout are those of the two sections above.  The rule is separable; each axis
 * has source length n (1 .. 65535), output length m (1 .. 4096) and D = max(n, m).  Every division is a floor division, also of a negative
 * numerator; every shift is arithmetic.
 *   the reduction limit: n <= NHW_CUBIC_MAX_REDUCTION m on each axis (at most 129 taps an axis);
 *   distance of source pixel i from output index o: N = (2 i + 1) m - (2 o + 1) n (2 m times the distance of the centres, in source pixels),
 *     U = floor((1024 |N| + D) / (2 D)), in 1/1024 of the kernel's unit: a source pixel when enlarging, n / m source pixels when shrinking;
 *   the taps of o: the i in 0 .. n - 1 with U < 2048, one contiguous run, cut at the picture's edges (not replicated);
 *   raw weight (the cubic times 2^31, exact in 64 bits): r = 3 U^3 - 5120 U^2 + 2^31 for U <= 1024, else r = -U^3 + 5120 U^2 - 8 x 2^20 U + 2^32
 *     (r(0) = 2^31, r(1024) = r(2048) = 0, negative between);
 *   quantised weight: R = sum of r over the run (positive), q_i = floor((2^15 r_i + R) / (2 R)), then 2^14 - sum q is added to the tap with the
 *     largest q, the lowest index among equals: a run's weights sum to exactly 16384;
 *   horizontal pass, source row y, output column ox: H[y][ox][c] = (sum_x qx P[y][x][c] + 128) >> 8 (units of 1/64; it can be negative);
 *   vertical pass and the byte: V = sum_y qy H[y][ox][c], byte = clamp((V + 2^19) >> 20, 0, 255);
 *   widths: sum |q| of a run stays below 2^15 (20 484 at the most on the axes the tests walk), so |sum qx P| < 2^23, |H| < 2^15, |V| < 2^30.
 * With n = m a run is one tap of 16384 (beside two of 0): the picture comes back byte for byte.
 * nhw_resample_to_tensor_device: nhw_resize_to_tensor_device with the filter named -- NHW_FILTER_TWO_TAP and NHW_FILTER_AREA are the two calls
 * above themselves, NHW_FILTER_CUBIC resamples under this rule: the same arguments, reads, writes, passed-over entries and NHW_E_ARG cases,
 * stream-ordered and capturable; an entry beyond the filter's reduction limit on either axis is passed over as well.  Any other filter is
 * NHW_E_ARG and nothing is launched.
 * nhw_dec_crops_to_device_resample: nhw_dec_crops_to_device_filter for the filters 0 .. 2.  Filters 0 and 1 are that call itself (the same
 * path, bytes, statuses and statistics); NHW_FILTER_CUBIC resizes the windows under this rule, and a rect whose window is beyond 32 times the
 * call's output size on a side gets status NHW_E_ARG: it selects no tile, its destination is not written, and the other rects go on.  Any
 * other filter is a call-level NHW_E_ARG.  (nhw_dec_crops_to_device_filter itself keeps refusing everything but 0 and 1.) */
#define NHW_FILTER_CUBIC 2
#define NHW_CUBIC_MAX_REDUCTION 32
int nhw_resample_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                  const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_to_device_resample(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                     uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr,
                                     int *status, int filter);

/* ---- encode straight from training tensors ----
 * The mirror of the section above: the encoder reads its pictures under an nhw_tensor_format -- the same struct, the same enums.  For this
 * direction the format says how the INPUT tensor is laid out, and scale[c], bias[c] are indexed by the TENSOR's channel c.
 *
 * The value rule (the whole specification).  For element x of tensor channel c:
 *   1. x is widened exactly to float32: NHW_T_F16 as IEEE binary16 with its denormals, NHW_T_BF16 as bits << 16, NHW_T_U8 as the integer;
 *   2. y = fmaf(x, scale[c], bias[c]) in single precision, ONE rounding, denormals honoured;
 *   3. the byte is 0 if y is a NaN; otherwise rint(y), ties to even, clamped to 0 .. 255 -- the clamp in float, before the conversion to an
 *      integer: -inf and every negative give 0, +inf and everything from 255.5 on give 255;
 *   4. NHW_T_U8 takes scale 1 and bias 0 only and passes the byte on: a pure permutation.
 * Channels and rows: with NHW_T_RGB tensor channel 0 is R and goes to byte 2 of the pixel; with NHW_T_ROWS_REVERSED tensor row r is row
 * H - 1 - r of the byte picture (S - 1 - r in a batch of 512 x 512 pictures).
 * Everything downstream is defined through those bytes: nhw_enc_batch_device_tensor is nhw_enc_batch_device of them, byte for byte (files,
 * sizes, status), and nhw_tile_tensors_device is nhw_tile_pictures_device of those byte pictures, so the edge replication acts on the
 * converted picture.  A format is refused with NHW_E_ARG, before anything is launched or allocated, for the reasons given above
 * nhw_tensor_format. */

/* n contiguous 512 x 512 pictures, [n][3][512][512] or [n][512][512][3] elements at d_in, to n * NHW_IMG_BYTES bytes at d_bgr as the byte entry
 * points take them.  Both pointers 16-byte aligned.  No handle: the current device; stream NULL is the null stream.  Asynchronous, and may be
 * captured in a graph.  NHW_E_ARG for NULL or misaligned pointers, n outside 1 .. 2^22 and a refused format.  (The byte format U8 / HWC / BGR /
 * ROWS_FILE is a plain copy.) */
int nhw_tensor_to_bytes_device(const void *d_in, int n, const nhw_tensor_format *fmt, void *d_bgr, void *stream);
/* nhw_enc_batch_device with a format in front of it: d_in as for nhw_tensor_to_bytes_device (16-byte aligned), the other arguments as for
 * nhw_enc_batch_device.  The bytes go to a scratch of max_batch * NHW_IMG_BYTES bytes that the handle owns: the FIRST tensor call on a
 * handle allocates it (so make that call before any graph capture) and nhw_enc_destroy frees it.  The conversion and the encode are ordered on
 * `stream`; byte and tensor calls on one handle work in any order.  The format U8 / HWC / BGR / ROWS_FILE routes to nhw_enc_batch_device itself,
 * with no copy and no scratch.  NHW_E_ARG, before anything is launched or allocated: a refused format, a misaligned d_in, and the cases of
 * nhw_enc_batch_device (NULL pointers, n outside 1 .. max_batch); NHW_E_QUALITY as there. */
int nhw_enc_batch_device_tensor(nhw_enc *e, const void *d_in, int n, const nhw_tensor_format *fmt, int quality,
                                void *d_out, int32_t *d_sizes, int32_t *d_status, void *stream);
/* Tensor pictures of any size (sides 1 .. 65535): addr = the device address of element (channel 0, row 0, column 0), pitch = bytes between rows,
 * plane = bytes between channel planes (read for NHW_T_CHW only; an NHW_T_HWC pixel is 3 consecutive elements and consecutive pixels of a row
 * follow each other), first_tile as in nhw_picture.  Crop views therefore work without a copy: x[:, y0:y1, x0:x1] of a larger CHW tensor,
 * x[y0:y1, x0:x1, :] of an HWC one. */
typedef struct { uint64_t addr, pitch, plane; uint32_t width, height, first_tile, reserved; } nhw_tensor_picture;   /* 40 bytes */
/* nhw_tile_pictures_device for tensor pictures: the tiles [tile0, tile0 + m) of the byte pictures the value rule makes of d_pics[0 .. n_pics)
 * (a device table, first_tile ascending) to d_tiles (m * NHW_IMG_BYTES bytes, 16-byte aligned).  Reads only elements of the pictures, never
 * between rows or beyond a view.  An entry with a zero side, a side above 65535, or an address, pitch or (CHW) plane that is no multiple of the
 * element size is passed over: its tiles are not written.  No handle: the current device; stream NULL is the null stream.  Asynchronous, and may
 * be captured in a graph.  NHW_E_ARG as for nhw_tile_pictures_device, and for a refused format. */
int nhw_tile_tensors_device(const nhw_tensor_picture *d_pics, int n_pics, int tile0, int m,
                            const nhw_tensor_format *fmt, void *d_tiles, void *stream);
/* hipEvent timings of the last nhw_dec_batch_device call (events on its launch stream): the whole sequence, the entropy stages
 * (parse, prefix-code walk, un-zig-zag), the two level-1 luma synthesis passes and the colour kernel -- the last three are the kernels
 * SURVEY.md 8(d) prices against the HBM roofline for the decode path */
typedef struct { float total_ms, entropy_ms, recon_ms; } nhw_dec_timing;   /* recon_ms: the final reconstruction kernel (level-1 synthesis both ways + colour) */
int nhw_dec_last_timing(nhw_dec *d, nhw_dec_timing *t);

/* ---- affine warps into tensors of one size: rotate, shear, translate ----
 * The resamplers above sample along an axis-aligned grid; a warp samples along a tilted one.  The source P is uint8 [h][w][3], B, G, R a pixel,
 * rows in file order, sides 1 .. 65535 (what an nhw_picture describes); the output is out_width x out_height, 1 .. 4096 each; an entry
 * carries one nhw_warp, declared below.  All arithmetic is signed 64-bit; every shift is arithmetic and floors.  For output pixel (ox, oy), numbered
 * before the format's row reversal exactly as the resamplers number theirs:
 *   position, in 1/65536 pixel on a grid where source pixel i has its centre at 65536 i:
 *     SX = ((a (2 ox + 1) + b (2 oy + 1)) >> 1) + c,   SY = ((d (2 ox + 1) + e (2 oy + 1)) >> 1) + f
 *     (the host folds the -1/2 of the centre convention into c and f); under the limits |SX|, |SY| < 2^41;
 *   X8 = (SX + 128) >> 8, ix = X8 >> 8, fx = X8 & 255, and iy, fy from SY alike (1/256 pixel; ix and iy fit 32 bits);
 *   the four taps (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1) with the weights (256 - fx)(256 - fy), fx (256 - fy), (256 - fx) fy,
 *     fx fy.  A tap with x outside 0 .. w - 1 or y outside 0 .. h - 1 takes `fill`; with NHW_WARP_REPLICATE it takes the pixel at the
 *     clamped index instead.  A tap is judged outside even where its weight is 0;
 *   byte = (sum of weight x tap + 32768) >> 16, a channel: section 18's blend, which cannot leave 0 .. 255;
 *   the tensor is what nhw_bytes_to_tensor_device makes of these bytes under the format: its value rule, channel order, row direction and
 *     layout.  There is no mirror flag: a mirror is a matrix.
 * The limits: each of |a|, |b|, |d|, |e| <= NHW_WARP_MAX_STEP x 65536 = 2^22, |c|, |f| <= 2^40.  An entry beyond them stores nothing, and so
 * do the entries the resamplers pass over: a zero or oversize side, a zero address, an address that is no multiple of the element size.
 * From a matrix [[A, B, C], [D, E, F]] that takes the centre (ox + 1/2, oy + 1/2) of an output pixel to continuous source coordinates, in
 * which pixel i covers [i, i + 1): a = rint(65536 A), b, d, e alike, c = rint(65536 (C - 1/2)), f = rint(65536 (F - 1/2)).  The matrix
 * [[1, 0, 0], [0, 1, 0]] (a = e = 65536, b = d = 0, c = f = -32768) returns the picture byte for byte, [[-1, 0, w], [0, 1, 0]] its mirror,
 * [[0, 1, 0], [-1, 0, h]] to an h x w output its quarter turn, [[1, 0, 5], [0, 1, -3]] the picture moved with `fill` in the uncovered
 * band: where the entries are multiples of 1/2 nothing is rounded. */
typedef struct nhw_warp {     /* 40 bytes, 8-byte aligned */
	int64_t  c, f;            /* offsets, 1/65536 source pixel; |c|, |f| <= 2^40 */
	int32_t  a, b, d, e;      /* steps, 1/65536 source pixel an output pixel; each |.| <= 2^22 (NHW_WARP_MAX_STEP 64 pixels) */
	uint8_t  fill[3];         /* B, G, R of the border colour */
	uint8_t  flags;           /* bit 0: NHW_WARP_REPLICATE, taps outside take the nearest edge pixel instead of `fill`; other bits are not read */
	uint32_t reserved;        /* 0 */
} nhw_warp;
#define NHW_WARP_REPLICATE 1
#define NHW_WARP_MAX_STEP 64
/* The warp alone, beside nhw_resample_to_tensor_device: picture k of the table d_pics[0 .. n) (addr, pitch, width and height are read; any
 * alignment and pitch; bytes outside a row's 3 width are never read) goes, under the rule above with the warp d_warps[k] (a device table
 * of n entries, 8-byte aligned as nhw_warp is: every device allocation is), to the [out_height][out_width][3] or [3][out_height][out_width]
 * elements at d_out_addr[k].  Writes exactly those elements,
 * element by element, or nothing for an entry that stores nothing.  No handle: the current device; stream NULL is the null stream.
 * Asynchronous, and may be captured in a graph.  NHW_E_ARG, before anything is launched: the cases of nhw_resample_to_tensor_device (NULL
 * d_pics or d_out_addr, n outside 1 .. 2^24, an output side outside 1 .. 4096, a refused format) and a NULL d_warps. */
int nhw_warp_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                              const nhw_warp *d_warps, const uint64_t *d_out_addr, void *stream);
/* nhw_dec_crops_to_device with the warp behind the windows in place of a resize, synchronous: rects are windows at `scale`, warps (host
 * memory, one entry a rect, never NULL: a call-level NHW_E_ARG) are expressed in the coordinates of their rect's window -- window pixel
 * (0, 0) is source pixel (0, 0) --, dst_addr[i] is the device address of warp i's tensor.  A rect whose warp is beyond the limits gets status
 * NHW_E_ARG before it selects a tile: its destination is not written, and the other rects go on.  Everything else is the crop call's: the
 * union of tiles, each uploaded and decoded once, the per-rect statuses, nhw_dec_last_region_stats and the call-level NHW_E_ARG cases. */
int nhw_dec_warps_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                            uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr,
                            int32_t *status);

/* ---- decode grey: the luma alone into one-channel bytes and tensors ----
 * The grey byte of a pixel is what the file's own colour matrix gives for the pixel's luma byte Y at neutral chroma, U = V = 128.  There the
 * matrix gives R = G = B for every quality and every Y, so grey is a table of 256 bytes a quality, G_q[Y]: the identity for quality 20 .. 23,
 * a monotone gain curve below (quality 19: 16 -> 16, 128 -> 131, 235 -> 241).  Y at scale 1 is the decoder's luma plane in front of the colour
 * matrix; at scale 2 and 4 it is the luma of the scaled decode above (the level-1 low band clipped; the level-2 low band turned and clipped).
 * The chroma of the file is not decoded: the chroma planes' kernels are not launched, and the last kernel stores 1 byte a pixel, not 3.
 * nhw_grey_table: G_quality into table[0 .. 256).  Host only: no handle, no GPU call.  NHW_E_ARG for a quality outside 1 .. 23 or a NULL table. */
int nhw_grey_table(int quality, uint8_t table[256]);
/* nhw_dec_batch_device_scaled as grey: scale 1, 2 or 4, S = 512 / scale.  fmt NULL: file i's S S grey bytes at d_out + i * S S, uint8 [S][S],
 * rows in file order (the byte path's).  Otherwise fmt->channels must be NHW_T_GREY, and file i's tensor, S S elements, lies at d_out + i * S *
 * S * sizeof(dtype): dtype, rows, scale[0] and bias[0] are read, under the value rule of the tensor formats; with one channel NHW_T_HWC
 * ([S][S][1]) and NHW_T_CHW ([1][S][S]) are the same memory, and both are accepted; entries 1 and 2 of scale and bias are checked as ever (finite;
 * scale 1 and bias 0 for NHW_T_U8) and not used.  d_status and d_quality are exactly those of the colour decode -- the prefix-code walk of the
 * chroma packet still runs, so a file whose chroma packet alone is damaged is refused here too --, and a refused file leaves its slot untouched.
 * NHW_E_ARG, before anything is launched: a format with NHW_T_BGR or NHW_T_RGB, an otherwise refused format, a d_out that is not 16-byte
 * aligned, a handle with a debug stop set, and the cases of nhw_dec_batch_device_scaled.  Asynchronous on `stream`; nhw_dec_last_timing
 * describes it, recon_ms = the kernel that writes the grey pictures.  One handle serves colour and grey batches in any order.  Every other
 * entry point refuses NHW_T_GREY, but for the grey calls of section 23 below. */
int nhw_dec_batch_device_grey(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale,
                              const nhw_tensor_format *fmt, void *d_out, int32_t *d_status, int32_t *d_quality, void *stream);
/* host convenience, synchronous: as nhw_dec_batch_scaled, for any n >= 1; file i's S S grey bytes land at out + i * S S */
int nhw_dec_batch_grey(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality);

/* ---- grey windows, crops, resamplers and warps at one byte a pixel ----
 * The grey picture of a container at scale s is its tile files' grey decodes at that scale (above), laid on the tile grid and cut to
 * ceil(W / s) x ceil(H / s): uint8 [H'][W'], rows in file order.  A grey window is a rectangle of it, a grey crop or warp a grey window resampled
 * or warped.  The seven calls below are the colour calls named beside them with one byte where those have three and one element where those have
 * three: the same arguments, checks, per-rect statuses (the tiles a call selects, uploads and decodes are the colour call's, and so are the
 * decoder's verdicts on them), statistics and passed-over entries.  What differs:
 *   a picture of a table (nhw_picture) and a packed window have 1 byte a pixel, and a pitch is at least the width;
 *   a tensor format must name NHW_T_GREY: NHW_T_BGR and NHW_T_RGB are refused as nhw_dec_batch_device_grey refuses them.  dtype, rows, scale[0]
 *     and bias[0] are read; NHW_T_HWC and NHW_T_CHW are the same memory, out_height x out_width elements, element (r, c) at index r out_width + c;
 *     entries 1 and 2 of scale and bias are checked as ever and not used;
 *   the rules of the resamplers (sections 18 to 20) and of the warp (section 21) apply to the one channel as they stand: positions, taps, weights,
 *     roundings, reduction limits, the mirror flag; a warp's border byte is fill[0], and fill[1] and fill[2] are not read;
 *   the host calls refuse a handle with a debug stop set at every scale, as the grey decode does.
 * There is no grey nhw_dec_pictures and no grey region call: a whole picture is the window (0, 0, ceil(W / s), ceil(H / s)), a region a window at
 * scale 1.  The colour entry points go on refusing NHW_T_GREY. */
/* nhw_untile_windows_device over the slots of a grey decode, T T bytes each: columns go to destination byte (col - x) of their row */
int nhw_untile_windows_grey_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses,
                                   int tile0, int m, int scale, void *stream);
/* nhw_resample_to_tensor_device and nhw_warp_to_tensor_device for one-byte pictures and one-channel tensors */
int nhw_resample_grey_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                       const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_warp_grey_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                   const nhw_warp *d_warps, const uint64_t *d_out_addr, void *stream);
/* nhw_dec_windows: window i's width x height grey bytes, packed, land at out + out_off[i] */
int nhw_dec_windows_grey(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                         uint8_t *out, const uint64_t *out_off, int32_t *status);
/* nhw_dec_windows_to_device: dst_pitch[i] >= width */
int nhw_dec_windows_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status);
/* nhw_dec_crops_to_device_resample (filter 0 .. 2) and nhw_dec_warps_to_device */
int nhw_dec_crops_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                 uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr,
                                 int32_t *status, int filter);
int nhw_dec_warps_grey_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                 uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr,
                                 int32_t *status);

/* ---- a colour matrix a sample in the crop, resample and warp stores ----
 * The photometric step that differs from sample to sample -- brightness, contrast about a fixed centre, saturation, a linear hue turn, a mix of
 * the channels, an inversion, grey with some probability -- is one affine map of the pixel.  An entry of a mapped call carries one nhw_colour_map.
 * The rule (the whole specification).  x = (x0, x1, x2) are the three bytes B, G, R that a resampler's (sections 18 to 20) or the warp's (section
 * 21) blend has made for an output pixel; a warp's border colour went through that blend and is mapped like any other pixel.  All arithmetic is
 * signed 32-bit:
 *   t_i = m[i][0] x0 + m[i][1] x1 + m[i][2] x2 + o[i];   under the limits |t_i| <= 3 x 255 x 2^20 + 2^28 = 1 070 596 096, so t_i + 32768 fits;
 *   y_i = min(max((t_i + 32768) >> 16, 0), 255);         the shift is arithmetic, floor((t_i + 32768) / 65536): halves go up, towards
 *                                                        +infinity, at either sign.
 * y then takes the place of the bytes in the pixel's store: the format's channel order, value rule, layout and row direction, and the mirror,
 * are what they are without a map.  m = 65536 I, o = 0 is the identity on every byte ((65536 b + 32768) >> 16 = b).
 * The one-channel form (section 23's pictures of one byte a pixel): y = clamp((m[0][0] x + o[0] + 32768) >> 16); the other ten numbers are not
 * used for the value.
 * A map is within the limits when each |m[i][j]| <= NHW_COLOUR_MAX_GAIN x 65536 = 2^20, each |o[i]| <= NHW_COLOUR_MAX_OFFSET x 65536 = 2^28 and
 * the reserved words are 0 -- all twelve numbers, for both families.  An entry whose map is not stores nothing. */
typedef struct nhw_colour_map {   /* 64 bytes, 4-byte aligned */
	int32_t  m[3][3];     /* 1/65536; row i makes output byte i, column j reads input byte j, both in the byte path's order B, G, R; each |.| <= 2^20 */
	int32_t  o[3];        /* 1/65536 of a grey level; each |.| <= 2^28 */
	uint32_t reserved[4]; /* 0 */
} nhw_colour_map;
#define NHW_COLOUR_MAX_GAIN   16     /* 2^20 / 65536 */
#define NHW_COLOUR_MAX_OFFSET 4096   /* 2^28 / 65536 */
/* nhw_resample_to_tensor_device with a device table of n maps, d_maps[k] for picture k: the same arguments, reads, writes, passed-over entries,
 * NHW_E_ARG cases in the same order, stream order and graph capture; a NULL d_maps is a call-level NHW_E_ARG before anything is launched.  The
 * format names the family: with fmt->channels == NHW_T_GREY the call is nhw_resample_grey_to_tensor_device with maps -- pictures of 1 byte a
 * pixel, one-channel tensors, the one-channel form of the rule --, with NHW_T_BGR or NHW_T_RGB the colour call. */
int nhw_resample_mapped_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                         const uint8_t *d_flags, const nhw_colour_map *d_maps, const uint64_t *d_out_addr, void *stream);
/* nhw_warp_to_tensor_device (nhw_warp_grey_to_tensor_device under a grey format) likewise */
int nhw_warp_mapped_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                     const nhw_warp *d_warps, const nhw_colour_map *d_maps, const uint64_t *d_out_addr, void *stream);
/* nhw_dec_crops_to_device_resample (nhw_dec_crops_grey_to_device under a grey format) with one map a rect, host memory, never NULL: a
 * call-level NHW_E_ARG beside dst_addr's.  A rect whose map is beyond the limits gets status NHW_E_ARG before it selects a tile, as a warp
 * beyond its limits does: its destination is not written, and the other rects go on.  Everything else -- the tiles, the statuses, the
 * statistics, the other refusals and their order -- is the unmapped call's; one handle serves mapped and unmapped calls in any order. */
int nhw_dec_crops_mapped_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const nhw_colour_map *maps,
                                   const uint64_t *dst_addr, int32_t *status, int filter);
/* nhw_dec_warps_to_device (nhw_dec_warps_grey_to_device under a grey format) likewise */
int nhw_dec_warps_mapped_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const nhw_colour_map *maps,
                                   const uint64_t *dst_addr, int32_t *status);

/* ---- a tone table a sample in the crop, resample and warp stores; histograms for equalize and autocontrast ----
 * The pointwise operations that are no affine map -- posterize, solarize, gamma, a curve, equalize, autocontrast -- are one table of 256 bytes a
 * channel.  An entry of a toned call carries one nhw_tone_table.
 * The rule (the whole specification).  y = (y0, y1, y2) are the three bytes B, G, R that the blend, and then the colour map if the call has one
 * (section 24), have made for an output pixel:  z_i = t[i][y_i].  z then takes the place of the bytes in the pixel's store.  The order is fixed:
 * blend, map, table, value rule; a warp's border colour goes through all of it.  The one-channel form (section 23) reads t[0] alone: the other 512
 * bytes are ignored, not checked.  Every table is valid: there is no predicate and no refusal for a table. */
typedef struct nhw_tone_table { uint8_t t[3][256]; } nhw_tone_table;   /* 768 bytes, any alignment; rows in the byte path's order B, G, R */
/* what nhw_tone_from_hist_device makes of a sample's histograms, one byte a sample; the rules are nhwcodec_amd/csrc/nhw_tone.h's, in 64-bit sums:
 * equalize -- PIL's ImageOps.equalize, torchvision's _scale_channel: total = sum h, last = the count of the highest non-empty bin, step = (total -
 *   last) / 255; step == 0: the identity; else row[0] = 0, row[x] = min((h[0] + .. + h[x - 1] + step / 2) / step, 255);
 * autocontrast -- lo, hi the lowest and highest non-empty bin; lo >= hi or nothing counted: the identity; else row[x] = clamp(floor(255 (x - lo) /
 *   (hi - lo)), 0, 255), exactly (torchvision computes it in float32 and may differ by one level where the quotient is an integer). */
#define NHW_TONE_KEEP         0      /* the sample's table is left exactly as it is (so is it under any op not named here) */
#define NHW_TONE_EQUALIZE     1
#define NHW_TONE_AUTOCONTRAST 2
/* nhw_resample_mapped_to_tensor_device with a device table of n tone tables, d_tones[k] for picture k.  d_maps may be NULL: no map, the table acts
 * on the blend's bytes.  A NULL d_tones is a call-level NHW_E_ARG among the NULL-pointer checks, before anything is launched.  With a map, an
 * entry whose map is beyond the limits stores nothing.  Every other check, message, order, stream and capture property is the mapped entry's; a
 * format of NHW_T_GREY makes it the one-channel call. */
int nhw_resample_toned_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                        const uint8_t *d_flags, const nhw_colour_map *d_maps, const nhw_tone_table *d_tones, const uint64_t *d_out_addr, void *stream);
/* nhw_warp_mapped_to_tensor_device likewise */
int nhw_warp_toned_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                    const nhw_warp *d_warps, const nhw_colour_map *d_maps, const nhw_tone_table *d_tones, const uint64_t *d_out_addr, void *stream);
/* nhw_dec_crops_mapped_to_device with one table a rect, host memory, never NULL; maps may be NULL.  Everything else is the mapped call's (without
 * maps, the unmapped call's); one handle serves plain, mapped and toned calls in any order. */
int nhw_dec_crops_toned_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                  uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const nhw_colour_map *maps,
                                  const nhw_tone_table *tones, const uint64_t *dst_addr, int32_t *status, int filter);
/* nhw_dec_warps_mapped_to_device likewise */
int nhw_dec_warps_toned_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                  uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const nhw_colour_map *maps,
                                  const nhw_tone_table *tones, const uint64_t *dst_addr, int32_t *status);
/* The histograms of the n pictures of a device table, as the resamplers take it (any address, pitch and sides of 1 .. 65535; `channels` 3 or 1
 * bytes a pixel): d_hist[k][c][v], uint32 [n][channels][256], is the number of pixels of picture k whose byte c is v.  The call overwrites d_hist
 * (it zeroes it on the stream first); a picture with a zero address or a zero or oversize side gives zeroes.  Integer sums: the same words every
 * run.  Reads only the pictures' own bytes.  Asynchronous on `stream`, capturable. */
int nhw_hist_device(const nhw_picture *d_pics, int n, int channels, uint32_t *d_hist, void *stream);
/* Rows of tone tables from histograms: for sample k and channel c, d_ops[k] (NHW_TONE_*) says what d_tones[k].t[c] becomes of d_hist[k][c]; with
 * channels == 1 only t[0] is written.  The histograms need not come from a picture.  Asynchronous on `stream`, capturable. */
int nhw_tone_from_hist_device(const uint32_t *d_hist, int n, int channels, const uint8_t *d_ops, nhw_tone_table *d_tones, void *stream);

/* ---- blur and sharpen a sample: the rule of a separable filter in front of the pixel's store ----
 * The one per-sample step of the common recipes that reads a pixel's neighbours -- GaussianBlur with a random sigma (SimCLR, MoCo v2, BYOL, DINO),
 * RandAugment's Sharpness, a box filter -- is two lists of taps, a mix and a border: one nhw_blur a sample.  This build has the rule (this text and
 * nhwcodec_amd/csrc/nhw_blur.h, for host and device) and the record; it has no device entry that applies it yet (section 26, "Left out").
 * The rule (the whole specification).  A picture is W x H, with C = 3 or 1 bytes a pixel.  Each channel is filtered on its own.  p(y, x) is a byte
 * of the picture.  ix(i, n) depends on the border.  Reflect, without repeating the edge: i < 0 -> -i, and i >= n -> 2 (n - 1) - i; this is torch's
 * `reflect` padding, which torchvision's gaussian_blur uses.  Replicate: min(max(i, 0), n - 1).  The four steps:
 *   1. h(y, x) = (sum_{j = 0 .. 2 rx} wx[j] p(y, ix(x + j - rx, W)) + 64) >> 7.  The result lies in 0 .. 65280, with eight fractional bits, and is
 *      held as 16 bits.
 *   2. b(y, x) = (sum_{j = 0 .. 2 ry} wy[j] h(ix(y + j - ry, H), x) + 2^22) >> 23.  The result lies in 0 .. 255.  The sum plus the rounding term
 *      is at most 32768 x 65280 + 2^22 = 2 143 289 344, below 2^31.
 *   3. z = clamp(p + floor((mix (b - p) + 32768) / 65536), 0, 255).  Halves go up at either sign, as in section 24: an arithmetic shift of a
 *      signed 32-bit value, |mix (b - p)| < 2^28.
 *   4. z takes the place of the byte in the pixel's store: the value rule, channel order, layout and row rule of nhw_tensor_format, exactly as
 *      the resamplers' store applies them.
 * Three consequences: rx = ry = 0 with a tap of 32768 gives b = p and z = p for every mix; mix = 65536 gives z = b; a constant picture stays
 * constant.
 * A blur is within the limits (nhw_blur_within of nhwcodec_amd/csrc/nhw_blur.h) for a W x H picture when rx, ry <= 15; wx[0 .. 2 rx] and
 * wy[0 .. 2 ry] each sum to 32768; |mix| <= 16 x 65536; border <= 1; and, under reflect, rx < W and ry < H.  The reserved fields are not read.
 * Beyond the limits the rule's sums may overflow and an index may leave the picture: nothing applies a record that is not within them. */
#define NHW_BLUR_MAX_RADIUS 15
#define NHW_BLUR_ONE        32768      /* a tap is in 1/32768 */
#define NHW_BLUR_MAX_MIX    16         /* |mix| <= 16 * 65536 */
enum { NHW_BLUR_REFLECT = 0, NHW_BLUR_REPLICATE = 1 };
typedef struct nhw_blur {              /* 144 bytes, 4-byte aligned */
	uint16_t wx[32], wy[32];           /* taps 0 .. 2 rx (2 ry); the entries behind them are not read */
	int32_t  mix;                      /* 1/65536: 65536 the blurred pixel, 0 the picture's own, below 0 sharpens */
	uint8_t  rx, ry, border, reserved8;
	uint32_t reserved[2];
} nhw_blur;

/* ---- encode grey: one-channel bytes and tensors at one byte a pixel ----
 * A grey picture is 512 x 512 bytes, rows in the byte path's order; picture i of a batch lies at i * NHW_GREY_BYTES.  The one contract of every
 * call here: the file is byte for byte the file nhw_enc_batch_device writes for the picture with every grey byte in B, G and R, at the same quality
 * and compatibility mode, with the same size and the same status.  No colour conversion, chroma staging or 4:2:0 filter runs: the luma is a table
 * of the byte and the quality (nhw_grey_luma_table), both 4:2:0 planes are 128.  One handle serves colour and grey batches in any order.
 * Below quality 16 the chroma of such a file does not decode to exactly neutral: the grey decode calls (section 22) are the way to read it.
 * The colour entry points go on refusing NHW_T_GREY. */
#define NHW_GREY_BYTES  262144u      /* 512*512 */
/* L_quality[0 .. 256): the encoder's luma of the pixel B = G = R = g.  Host only: no handle, no GPU call.  NHW_E_ARG for a quality outside 1 .. 23 or a NULL table */
int nhw_grey_luma_table(int quality, int16_t out[256]);
/* nhw_enc_batch_device from n grey pictures at d_grey, which must be 16-byte aligned; every other argument and check as there */
int nhw_enc_batch_device_grey(nhw_enc *e, const void *d_grey, int n, int quality, void *d_out, uint32_t *d_sizes,
                              int32_t *d_status, void *stream);
/* nhw_enc_batch from n grey pictures in host memory, through the staging the handle already has */
int nhw_enc_batch_grey(nhw_enc *e, const uint8_t *grey, int n, int quality, uint8_t *out_arena, size_t arena_cap,
                       uint64_t *out_off, int32_t *status);
/* nhw_tensor_to_bytes_device and nhw_enc_batch_device_tensor for one-channel tensors: fmt->channels must be NHW_T_GREY (NHW_T_BGR and NHW_T_RGB
 * are refused), d_in holds n x 512 x 512 elements -- [n, 1, 512, 512] and [n, 512, 512, 1] are the same memory, so the layout is not read --,
 * the value rule of an encode runs with scale[0] and bias[0]; d_grey: n * NHW_GREY_BYTES, 16-byte aligned */
int nhw_tensor_to_bytes_grey_device(const void *d_in, int n, const nhw_tensor_format *fmt, void *d_grey, void *stream);
int nhw_enc_batch_device_grey_tensor(nhw_enc *e, const void *d_in, int n, const nhw_tensor_format *fmt, int quality,
                                     void *d_out, int32_t *d_sizes, int32_t *d_status, void *stream);
/* nhw_tile_pictures_device at one byte a pixel: a table of [H][W] pictures of any alignment and pitch, tile t into d_tiles + (t - tile0) * NHW_GREY_BYTES */
int nhw_tile_pictures_grey_device(const nhw_picture *d_pics, int n_pics, int tile0, int m, void *d_tiles, void *stream);
/* nhw_enc_pictures from grey pictures, W x H bytes packed at grey + in_off[i]: the container format is unchanged, every tile file an ordinary .nhw */
int nhw_enc_pictures_grey(nhw_enc *e, const uint8_t *grey, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                          int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status);

/* ---- per-sample flip, colour map and tone table in the full-file decode ----
 * The operations of sections 18, 24 and 25 -- the mirror, the 3 x 4 colour map, the 256-entry tone table -- in the last store of
 * nhw_dec_batch_device_tensor and nhw_dec_batch_device_grey: a batch of native .nhw files goes to augmented training tensors without a pass over
 * the bytes.
 * The rule (the whole specification).  Two inputs are defined first.  Colour form: the bytes B, G, R of a pixel of the plain decode at scale s (1, 2
 * or 4; S = 512 / s), as the byte path (nhw_dec_batch_device_scaled) stores them.  Grey form: the grey byte of section 22, the luma after the file's
 * grey table.  File i of a batch has a flag byte d_flags[i], a colour map d_maps[i] and a tone table d_tones[i]; each of the three tables may be
 * absent (NULL) for the whole call, and an absent table's step is skipped.  The output pixel at byte-path row r, column c is made in this order:
 *   1. mirror      take the pixel at column c' = S - 1 - c where bit 0 of d_flags[i] is set, else at column c.  Rows are not touched: the format's
 *                  `rows` keeps its meaning and is independent of the flag.  The other bits of the flag byte are ignored.
 *   2. colour map  nhw_colour_apply<3>(d_maps[i], b), the rule of section 24 on the three bytes; grey: nhw_colour_apply<1>, m[0][0] and o[0] alone.
 *   3. tone table  nhw_tone_apply<3>(d_tones[i].t, b), z_i = t[i][y_i] (section 25); grey: nhw_tone_apply<1>, row 0 alone.
 *   4. the value rule, channel order, layout and row rule of the nhw_tensor_format, as the plain entries apply them.
 * This is section 26's order "resize, flip, colour, tone, blur, value rule" without the resize and the blur.
 * A file whose map is not within the limits of section 24 (a non-zero reserved word included) stores nothing: its slot stays untouched, and its
 * status and quality are those of the plain decode.  A refused file leaves its slot untouched, as in the plain entries.  With all three tables NULL
 * the call is the plain call, byte for byte: it launches exactly what the plain entry launches.
 * d_flags (n bytes), d_maps (n nhw_colour_map, 4-byte aligned) and d_tones (n nhw_tone_table, any alignment) are device tables; they are read by
 * the last kernel, so they must stay valid until the call's work on `stream` is done.
 * NHW_E_ARG, before anything is launched: exactly the cases of the plain entry, in its order; nothing is refused for the tables, which live on the
 * device.  Unlike the plain tensor entry, the byte format (NHW_T_U8 / NHW_T_HWC / NHW_T_BGR / NHW_T_ROWS_FILE) with any table present goes through
 * the operations like every other format.  Asynchronous on `stream`; one handle serves all kinds of call in any order. */
int nhw_dec_batch_device_tensor_ops(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale,
                                    const nhw_tensor_format *fmt, const uint8_t *d_flags, const nhw_colour_map *d_maps,
                                    const nhw_tone_table *d_tones, void *d_out, int32_t *d_status, int32_t *d_quality, void *stream);
/* the same for nhw_dec_batch_device_grey: fmt of NHW_T_GREY as that entry takes it, NULL fmt = uint8 [S][S] in file order */
int nhw_dec_batch_device_grey_ops(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale,
                                  const nhw_tensor_format *fmt, const uint8_t *d_flags, const nhw_colour_map *d_maps,
                                  const nhw_tone_table *d_tones, void *d_out, int32_t *d_status, int32_t *d_quality, void *stream);

#ifdef __cplusplus
}
#endif
#endif
