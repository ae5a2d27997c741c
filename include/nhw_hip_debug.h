/*
 * nhw_hip_debug.h -- the debug / test entry points of libnhwhip.so (C ABI).  Not part of the drop-in boundary (include/nhw_hip.h): the
 * parity tests use them to stop the batch driver after a stage and to read workspace buffers back, so that a mismatch against the
 * checkpoint trace of the reference ("checkpoint" flavour) is located at one stage instead of at the .nhw bytes.
 * tests/test_gpu_parity.py::test_c_abi_exports_every_declared_symbol checks every name declared here against the library, like the
 * boundary's own.
 */
#ifndef NHW_HIP_DEBUG_H
#define NHW_HIP_DEBUG_H

#include "nhw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* encoder: the next batches stop after launch stage `stage` of the batch driver (0: run to the end).  Stage numbers follow the order of
 * the reference's cross-TU calls in encode_image (nhw_encoder.c:103-2878); tools/dev/gpu_low_debug.py lists them per quality. */
int nhw_debug_stop_after(nhw_enc *e, int stage);
/* encoder: every carry segment of the fused front kernel takes its exact replay (the path the look-back falls back to) */
int nhw_debug_front_fallback(nhw_enc *e, int on);
/* encoder: the first `bytes` bytes of workspace buffer `buf` (an index of the B_* list in nhwcodec_amd/csrc/nhw_ws.h) of image `img` -> host */
int nhw_debug_read(nhw_enc *e, int buf, int img, void *dst, size_t bytes);
/* encoder: an order-independent 64-bit digest of the first `bytes` bytes of buffer `buf`, one per image, into device memory (n x uint64) */
int nhw_debug_hash(nhw_enc *e, int buf, size_t bytes, int n, void *d_out, void *stream);

/* encoder: the first `bytes` bytes of buffer `buf` of the first n images set to `byte` (the zero guard behind the buffer is not touched): a test
 * that the production launch sequence -- which leaves out stores nothing reads -- never reads what an earlier batch left in a plane */
int nhw_debug_fill(nhw_enc *e, int buf, int byte, size_t bytes, int n);

/* 0: production launches; 1: every kernel that splits an item runs one slice per launch, slices in ascending order, on the same stream;
 * 2: the same in descending order.  A slice is one value of a kernel's per-item split (a band, a quarter, a window, a row band); each
 * serial launch covers that slice for every item of the batch.  Successive launches on a stream do not overlap, so a slice that reads what
 * another slice of the same item writes sees it written (mode 1: the slices before it; mode 2: the ones behind it).  The kernels in the mode
 * and the ones that cannot have the hazard: DESIGN.md, "Kernels that split an item". */
int nhw_debug_slice_order(nhw_enc *e, int mode);
int nhw_dec_debug_slice_order(nhw_dec *d, int mode);

/* The chroma closed loops of component comp (0: U, 1: V) for the first n images of the handle's last whole batch, at that batch's quality, on the
 * handle's first set of chroma planes (B_CPROC, B_CLL1, B_CL2SAVE; B_CJPEG for the staged forms).  form 0: the head as a production batch
 * launches it, from the 4:2:0 byte planes that batch left (pre-filter / level-1 analysis, then the fused level-2 kernel); form 1: the fused
 * kernel alone on cll1 and cproc as they stand; form 2 .. 8: the first form - 1 of the seven staged kernels alone on the same inputs (8: all
 * of them; 4: up to the first synthesis).  The tests write planes with nhw_debug_write (host bytes into workspace buffer buf of image img,
 * the counterpart of nhw_debug_read) and read them behind the call. */
int nhw_stage_chroma_loops(nhw_enc *e, int n, int comp, int form, void *stream);
int nhw_debug_write(nhw_enc *e, int buf, int img, const void *src, size_t bytes);
/* The chroma tail of component comp (the marks of quality 18 .. 23, the LL2 emission, the quantiser) for the first n images of the handle's last
 * whole batch, at that batch's quality, on B_CPROC, B_CLL1 and B_CL2SAVE as they stand (V on a handle with the chroma fork: B_CPROC_V, B_CLL1_V,
 * B_CL2SAVE_V) and the exception list (B_EXW, its length in B_META).  form 0: the production kernel, which reads each plane row once and
 * does not write the work plane; form 1: the staged body with every plane written and the dense chroma stream in B_SCAN (from byte 4 * 65536
 * on).  Both leave the symbol list (B_CNZQ with the cfbase table of 20 words behind its 2048 maps, B_CVALS: cfbase[F] is where the values of
 * the sixteen plane rows 16 F .. 16 F + 15 start, wherever the kernel put them), U's parked bytes (B_UBYTES), the LL2 bytes, the exception
 * list and the bit-1 bytes.  Run U before V: V merges U's parked bytes. */
int nhw_stage_chroma_tail(nhw_enc *e, int n, int comp, int form, void *stream);
/* The luma plane's first closed loop for the first n images of the handle's last whole batch, at that batch's quality (7 .. 23), on B_JPEG, B_PROC,
 * B_LL1 and B_L2SAVE as they stand.  form 0: the production kernels from the first level-2 analysis to the second; form 1: their last part
 * alone (synthesis, Y8, Y9 and, for q > 12 on the same LDS residency, the second analysis with Y13's copy); form 2: the staged kernels for
 * form 1's part; form 3: the staged kernels for form 0's part; form 4: form 3 stopped behind the synthesis; form 5: the staged synthesis alone.
 * Forms 0 and 1 are the production kernels with every plane stored, so that they can be compared with the staged ones cell by cell.  A batch
 * (outside the compatibility mode and without a debug stop) leaves out the stores of the level-2 block that nothing behind them reads, listed in
 * the transposed first-direction plane of both analyses in B_JPEG, and rows 128 .. 255 of the second analysis' block in B_PROC.
 * forms 6, 7: forms 0, 1 as a batch launches them, without those stores (not in the compatibility mode): the cells keep what stood there. */
int nhw_stage_luma_loop(nhw_enc *e, int n, int form, void *stream);
/* The LL2 bump walk of the luma plane's second closed loop for the first n images of the handle's last whole batch, at that batch's quality
 * (13 .. 23), on B_PROC, B_JPEG and B_L2SAVE as they stand: the LL2 emission, the LL coder and the second dequantiser simulation on one stream.
 * form 0: the forked order's kernels (the emission makes the walk for both, the simulation skips it); form 1: the in-line order's (each makes
 * it); forms 2, 3: the same two with the verbatim samples put back by the level-2 synthesis, which then follows.  These are the kernels of a
 * batch as they are: between them they write every cell of the level-2 block of B_JPEG (which is why a batch does not store the block in front
 * of them, see nhw_stage_luma_loop), and they read of B_PROC only rows 0 .. 127 of the block. */
int nhw_stage_ll2_walk(nhw_enc *e, int n, int form, void *stream);
/* The luma quantiser for the first n images of the handle's last whole batch, at that batch's quality (17 .. 23), on B_L2SAVE, B_PROC and the other
 * planes as they stand.  form 0: the second dequantiser simulation, which leaves the level-2 details behind the quantiser's loops 2 and 3 in
 * B_KMAP, then the quantiser reading them (production); form 1: the quantiser alone with its own loops.  Both leave the symbol list to be read:
 * B_NZQ (the non-zero map, 4096 words, with the fbase table of 33 words behind it) and B_VALS. */
int nhw_stage_quant(nhw_enc *e, int n, int form, void *stream);
/* The luma residual passes Y19 .. Y27 (between the second level-2 synthesis and the quantiser) for the first n images of the handle's last whole
 * batch, at that batch's quality, on B_JPEG (its LL quadrant: the first-order samples Y19 copies above quality 21), B_PROC, B_LL1, B_L2SAVE and
 * B_FIRST as they stand, on one stream.  form 0: the kernels of Y19 .. Y23, of Y24 and Y25 (quality > 12) and of Y26 and Y27 as a production batch
 * launches them -- up to quality 21 without Y26's copy of the level-2 block, HL1's first row looking up into B_L2SAVE; form 1: the same
 * launches as a debug stop makes them, with the copy at every quality; form 2: Y24 and Y25 alone on the code plane B_LL1 as it stands
 * (quality > 12); form 3: Y26 and Y27 alone, as production.  Behind the call: B_PROC's level-1 bands, its level-2 block where the form copies it
 * (quality > 21 or form 1), B_FIRST above quality 21, the position lists B_R1 / R3 / R5 (LIST, BITS, WORD) with their lengths in B_META. */
int nhw_stage_residuals(nhw_enc *e, int n, int form, void *stream);
/* The stream stage (the Y31 symbol rewrites, then the RLE + VLC packetiser and the container) for the first n images of the handle's last whole
 * batch, at that batch's quality, on the workspace as it stands.  form 0: k_y31 and k_final, from the symbol lists as the quantisers leave
 * them (B_NZQ with its fbase table, B_VALS; B_CNZQ with cfbase, B_CVALS); form 1: k_final alone, on B_NZS / B_VOFF / B_VALS as they stand;
 * form 2: k_y31 alone, which leaves its lists to be read (k_final puts the chroma part's map into B_NZS / B_VOFF) and reports nothing.
 * The files go to the handle's own output arena, the per-image status and file size to `status` and `sizes` (n entries each, host memory;
 * sizes may be null); the packet words, the code books, the sign words and the scalars are read from the workspace behind the call
 * (B_PACKET, B_BOOK1/2, B_SEL1/2, B_META). */
int nhw_stage_stream(nhw_enc *e, int n, int form, int32_t *status, uint32_t *sizes, void *stream);

/* decoder: the same two hooks (stage order: decode_image, decoder/nhw_decoder.c:54-1476; `what`: an index of the D_* list in nhw_dec.hip, sized by dec_bytes there) */
void nhw_dec_debug_stop_after(nhw_dec *d, int stage);
int  nhw_dec_debug_read(nhw_dec *d, int what, int img, void *dst, size_t bytes);
/* decoder: the colour matrix of write_image_bmp (nhw_decoder_cli.c:133-283) for quality q on n (Y, U, V) byte triples in device memory (n a
 * multiple of 8) -> n x 3 bytes in the order the reference writes them, through the functions k_dec_final runs: the exhaustive 2^24 test */
int  nhw_dec_debug_colour(int quality, const void *d_yuv, void *d_rgb, int n);
/* the warp kernel's choice of walk, for measurements and tests: every later nhw_warp_to_tensor_device and
 * nhw_dec_warps_to_device of the process walks an entry by rows where |d| <= limit and by 8 x 8 blocks elsewhere (-1: blocks for every entry;
 * 4194304: rows for every entry); a limit below -1 puts the rule's own 16384 back.  The bytes do not depend on the walk. */
void nhw_debug_warp_row_limit(int limit);

#ifdef __cplusplus
}
#endif
#endif
