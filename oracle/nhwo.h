/*
 * nhwo.h -- CPU ORACLE for the NHW encode hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the reference encoder's algorithm (rcanut/nhwcodec,
 * /root/reference/encoder/), written from scratch for this repo.  Every function cites the
 * reference file:line it follows.  It exists to CHECK the HIP product path; nothing under
 * nhwcodec_amd/ or include/ may include, link, load or call it.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may.
 *
 * Parity pin: validated stage by stage (checkpoint trace) and end to end (.nhw bytes) against
 * oracle/_ref = the unmodified reference sources linked with a zero-fill / zero-guard allocator
 * ("canonical" build), and against the committed golden
 * vectors in tests/golden/ that were generated from that build.
 *
 * Out-of-bounds model: ZERO.  The reference reads a few hundred bytes outside several of its
 * heap blocks; here every logical buffer is carved with the reference's own size and has
 * NHWO_GUARD zero bytes on both sides, so those reads return 0 exactly as in the canonical build.
 *
 * Supported quality settings in this revision: 17..23 (see nhwo_quality_supported()).
 */
#ifndef NHWO_H
#define NHWO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NHWO_DIM   512              /* image is NHWO_DIM x NHWO_DIM */
#define NHWO_HALF  256              /* reference IM_DIM  (encoder/codec.h:61) */
#define NHWO_QSIZE 65536            /* reference IM_SIZE (encoder/codec.h:58) */
#define NHWO_IMG_BYTES (NHWO_DIM * NHWO_DIM * 3)
#define NHWO_GUARD 4096
#define NHWO_MAX_OUT (1 << 20)

enum {
	NHWO_OK = 0,
	NHWO_E_QUALITY = -1,      /* quality setting not supported by this revision */
	NHWO_E_CODEBOOK = -2,     /* reference would exit(-1): compress_pixel.c:234,270,271 */
	NHWO_E_SPACE = -3,        /* output buffer too small */
	NHWO_E_ALLOC = -4
};

/* checkpoint trace, same record layout as oracle/ref/ref_shim.c */
typedef struct {
	uint8_t *buf;
	size_t cap, len;
	int count;
} nhwo_trace;

int nhwo_quality_supported(int quality);

/* What out-of-bounds reads of the reference return.  NHWO_OOB_ZERO (default) is the canonical, normative model (every such read
 * is 0).  NHWO_OOB_GLIBC_ONESHOT reproduces the heap adjacency of the stock `gcc -O3` nhw-enc run on one image per process
 * (SURVEY.md App. D): a compatibility mode for comparing against that binary; its output equals the binary's except for the
 * un-initialised padding bytes at the end of the res*_word / select_word sections. */
enum { NHWO_OOB_ZERO = 0, NHWO_OOB_GLIBC_ONESHOT = 1 };
extern int nhwo_oob_mode;

/* Whole encoder: BGR24 (BMP file order, 786432 bytes) -> .nhw bytes.  trace may be NULL. */
int nhwo_encode(const uint8_t *bgr, int quality, uint8_t *out, size_t cap, size_t *out_len, nhwo_trace *trace);

/* SURVEY.md section 8d synthetic image (integer generator), writes 786432 bytes. */
void nhwo_synth_image(uint32_t seed, uint8_t *bgr);

/* ---- stage-level entry points (used by the per-kernel parity tests) ---- */

/* a1: colorspace.c:55-260.  y: short[512*512]; u,v: uint8[256*256]. */
void nhwo_color(const uint8_t *bgr, int quality, int16_t *y, uint8_t *u, uint8_t *v);
/* a2: image_processing.c:558-2426 (q 17..21 branch).  In place on y[512*512]. */
void nhwo_prefilter(int16_t *y, int quality);
/* a3..a6: wavelet_filterbank.c:52-302.  jpeg/proc: planes of stride `stride`, n = transform size.
 * final_level != 0 <=> last_stage == wvlts_order-1 (no LL copy-back).  keep (may be NULL): receives the
 * first 256 rows x 512 of the transposed pass-1 plane (q>=22, level 0; wavelet_filterbank.c:107-112). */
void nhwo_analysis(int16_t *jpeg, int16_t *proc, int stride, int n, int final_level, int16_t *keep);
/* a7: wavelet_filterbank.c:305-496. */
void nhwo_synthesis(int16_t *jpeg, int16_t *proc, int stride, int n);

/* The stream stage: the symbol rewrites of encode_image (nhw_encoder.c:2134-2252) and wavlts2packet (compress_pixel.c:53-469) on a symbol
 * stream the caller made -- luma: 4 * NHWO_QSIZE symbols as the serpentine gather leaves them, chroma: 2 * NHWO_QSIZE as the chroma quantisers
 * leave them.  luma_out: the luma part behind the three rewrites.  select1_pre / select2_pre: the counts the second rewrite leaves
 * (nhw_select1 / nhw_select2 before packing); select1 / select2: the bytes of sel_word1 / sel_word2 (4 * NHWO_QSIZE / 8 + 8 bytes each).
 * The packet is made in a scratch of the worst case's size: `words` is what the stream takes, however many (the encoder's block holds
 * 80000), and `packet` receives the first min(words, packet_cap).  book1 / book2: 708 bytes each.  Returns the status (also in info). */
typedef struct {
	int status;
	int select1_pre, select2_pre, select1, select2;
	int size_data1, size_data2, size_book1, size_book2, tree_end, wavelet_type;
	int words;
} nhwo_stream_info;
int nhwo_stream_stage(const uint8_t *luma, const uint8_t *chroma, uint8_t *luma_out, uint8_t *sel_word1, uint8_t *sel_word2,
                      uint32_t *packet, size_t packet_cap, uint8_t *book1, uint8_t *book2, nhwo_stream_info *info);
/* The residual stage: the luma passes between the second level-2 synthesis and the quantiser (nhw_encoder.c:766-2098, Y19 .. Y27 of SURVEY.md
 * Appendix A) on planes the caller made -- the very function nhwo_luma runs.  The passes come in three parts: 0: Y19 .. Y23 (the copy to the
 * first-order plane, the level-1 thresholds, the +-5..7 runs, the residual classification and codes), 1: Y24 and Y25 (the feedback into the
 * first-order plane, the three position lists), 2: Y26 and Y27 (the detail clean-ups); the call runs parts first .. last.  jpeg, proc: 4 *
 * NHWO_QSIZE shorts each; ll1, l2save, first_order: NHWO_QSIZE each; all in and out.  Inside they live in the guarded arena, so reads past ll1
 * and l2save see zeros.  out: the three position lists (res1, res3, res5) with their lengths and the raw entry count of each pass before pruning
 * (row markers included), and the arm counters of this call. */
#define NHWO_ARM_MAX 128
typedef struct {
	int list_len, bits_len, word_len, raw_count;
	uint8_t list[NHWO_QSIZE + 64], bits[NHWO_QSIZE / 8 + 64], word[NHWO_QSIZE / 4 + 64];
} nhwo_residual_list;
typedef struct {
	nhwo_residual_list pl[3];
	uint32_t arm[NHWO_ARM_MAX];
} nhwo_residual_out;
int nhwo_residual_stage(int quality, int first, int last, int16_t *jpeg, int16_t *proc, int16_t *ll1, const int16_t *l2save,
                        int16_t *first_order, nhwo_residual_out *out);
/* the arm counters: how many there are, a counter's name, whether the arm can be taken at a quality.  The counters themselves are plain
 * increments in the passes, on in every build; nhwo_residual_stage reports what its own call added. */
int nhwo_arm_count(void);
const char *nhwo_arm_name(int arm);
int nhwo_arm_live(int arm, int quality);
/* oracle-only tap: when set (null by default), nhwo_luma copies the five planes in front of the residual passes into `in`, and the planes and
 * lists behind them into `out` and `lists`.  The checkpoint trace does not change. */
typedef struct { int16_t jpeg[4 * NHWO_QSIZE], proc[4 * NHWO_QSIZE], ll1[NHWO_QSIZE], l2save[NHWO_QSIZE], first_order[NHWO_QSIZE]; } nhwo_residual_planes;
typedef struct { nhwo_residual_planes in, out; nhwo_residual_out lists; } nhwo_residual_tap;
extern nhwo_residual_tap *nhwo_residual_tap_ptr;

/* which byte codes can enter a code book (compress_pixel.c:131-160) */
int nhwo_book_symbol_ok(int v);

/* ---- decoder (BASELINE config 5; nhwo_dec.c) ---- */
/* .nhw bytes -> 786432 bytes in the order the reference's nhw-dec writes them behind its 54-byte BMP header */
int nhwo_decode(const uint8_t *nhw, size_t len, uint8_t *bgr, int *quality);
/* checkpoint before the colour matrix: planes = Y, U, V, 262144 bytes each (decode_image's im_bufferY/U/V) */
int nhwo_decode_planes(const uint8_t *nhw, size_t len, uint8_t *planes, int *quality);
void nhwo_dec_color(const uint8_t *y, const uint8_t *u, const uint8_t *v, int q, uint8_t *out);
void nhwo_dec_bmp_header(uint8_t h[54]);

#ifdef __cplusplus
}
#endif
#endif
