/* nhwo_internal.h -- oracle internals.  TEST INFRASTRUCTURE ONLY (see nhwo.h). */
#ifndef NHWO_INTERNAL_H
#define NHWO_INTERNAL_H

#include <stdlib.h>
#include <string.h>
#include "nhwo.h"

#define W  512      /* luma plane row stride = reference 2*IM_DIM */
#define H  256      /* reference IM_DIM; chroma plane row stride */
#define Q  65536    /* reference IM_SIZE */
#define DEADZONE 8  /* reference `ratio` / m1 / m2: nhw_encoder_cli.c:177 select=8 */

static inline int iabs(int v) { return v < 0 ? -v : v; }

/* arena of zero-filled buffers, each between NHWO_GUARD zero bytes ("OOB = ZERO" model) */
typedef struct {
	uint8_t *base;
	size_t cap, used;
} nhwo_arena;

static inline void *arena_get(nhwo_arena *a, size_t bytes)
{
	size_t need = (bytes + 63) & ~(size_t)63;
	uint8_t *p;
	if (a->used + need + 2 * NHWO_GUARD > a->cap) return NULL;
	p = a->base + a->used + NHWO_GUARD;
	a->used += need + NHWO_GUARD; /* the trailing guard of one block is the leading guard of the next */
	return p;
}

/* position-list side stream (nhw_res1/3/5/6: list bytes, low-bit plane, payload words) */
typedef struct {
	uint8_t *list;  int list_len;
	uint8_t *bits;  int bits_len;
	uint8_t *word;  int word_len;
} nhwo_poslist;

typedef struct {
	int q;
	nhwo_arena arena;
	nhwo_trace *trace;

	/* planes (names follow the reference's image_buffer, codec.h:112-123) */
	int16_t *jpeg, *proc;           /* luma: 4*Q shorts each */
	int16_t *cjpeg, *cproc;         /* chroma: Q shorts each */
	uint8_t *pu, *pv;               /* 4:2:0 chroma planes, Q bytes each */
	int16_t *ll1;                   /* reference res256 (luma: Q shorts) */
	int16_t *l2save;                /* reference resIII (luma: Q shorts) */
	int16_t *cll1, *cl2save;        /* chroma res256 / resIII: Q/4 shorts */
	int16_t *keep;                  /* im_quality_setting: 2*Q shorts (q>=22) */
	int16_t *first_order;           /* im_wavelet_first_order: Q shorts (q>=22) */
	int16_t *band;                  /* im_wavelet_band: Q shorts (q>=22) */
	uint8_t *scan;                  /* im_nhw: 6*Q bytes */

	/* encode_state (codec.h:125-181) */
	uint8_t *ll_bytes;              /* first life of enc->tree1: 96*H+1 bytes of LL2 samples */
	uint8_t *ll_full;               /* enc->ch_res during the LL2 emission: Q/4 bytes */
	uint8_t *exw;  int exw_len;     /* exw_Y */
	uint8_t *res4; int res4_len;
	nhwo_poslist res1, res3, res5, res6;
	uint16_t *char_res1; int char_res1_len;
	uint32_t *qsetting3; int qsetting3_len;
	uint8_t *ll_comp;               /* highres_comp: Q/2 bytes */
	int ll_comp_y_len;              /* Y_res_comp */
	uint8_t *ll_word; int ll_word_len;        /* highres_word / highres_comp_len */
	uint16_t *ll_mem; int ll_mem_len;         /* highres_mem */
	uint8_t *ch_res;  int ch_res_len;         /* final ch_res / end_ch_res */
	uint8_t *res_u64, *res_v64;     /* 512 bytes each */
	int res_low, res_high;          /* setup->RES_LOW / RES_HIGH */
	int wavelet_type;               /* setup->wavelet_type after wavlts2packet (0 or 4) */
	int select1, select2;
	uint8_t *sel_word1, *sel_word2;
	uint32_t *packet;               /* enc->encode: 80000 words */
	int size_data1, size_data2;
	uint8_t *book1, *book2;         /* second life of tree1 / tree2: 708 bytes each */
	int size_book1, size_book2, tree_end;
	uint8_t book_tmp[600];          /* wavlts2packet's `codebook` scratch, shared by both parts */
	int res1_count, res3_count, res5_count; /* running nhw_resN_word_len counters of Y22/Y23 */
	int raw_count[3];               /* Y25: entries of each pass's list before pruning, row markers included (reference buffer: 96*H+1 bytes) */
} nhwo_ctx;

/* The arm counters of the residual passes (nhwo.h, nhwo_residual_stage): X(name, first quality, last quality at which the arm can be taken).
 * Arms the reference has and no input reaches are not here: its (-7, -6/-7) and (7, 7) branches of Y21 (nhwo_luma.c, tag_small_runs: 5 .. 7 and
 * -7 .. -5 are consumed by the two tests in front of them), and the ripple's "8 beside -7" (ripple: an 8 is 0 modulo 8 and at least 8, so the chain's
 * first test takes it). */
#define NHWO_ARMS(X) \
	/* Y20, 16 <= q <= 19 */ \
	X(Y20H_HL, 16, 19) X(Y20H_HH, 16, 19) \
	/* Y20, q 14 and 15 */ \
	X(Y20M_HL_ZERO, 14, 15) X(Y20M_HH_LOUD, 14, 15) X(Y20M_HH_ZERO, 14, 15) \
	/* Y20, q <= 13: the loud count's four levels (q <= 12), then by band: thin_by_parent's three arms, the isolated and the small cell */ \
	X(Y20L_LOUD3, 1, 12) X(Y20L_LOUD2, 1, 12) X(Y20L_LOUD1, 1, 12) X(Y20L_LOUD0, 1, 12) \
	X(Y20L_LH_PARENT, 1, 13) X(Y20L_LH_PAIRL, 1, 13) X(Y20L_LH_PAIRR, 1, 13) X(Y20L_LH_ISO, 1, 13) \
	X(Y20L_HL_PARENT, 1, 13) X(Y20L_HL_PAIRL, 1, 13) X(Y20L_HL_PAIRR, 1, 13) X(Y20L_HL_ISO, 1, 13) X(Y20L_HL_SMALL, 1, 13) \
	X(Y20L_HH_PARENT, 1, 13) X(Y20L_HH_PAIRL, 1, 13) X(Y20L_HH_PAIRR, 1, 13) X(Y20L_HH_ISO, 1, 13) X(Y20L_HH_SMALL, 1, 13) \
	X(Y20L_KEEP_P7, 11, 13) X(Y20L_KEEP_N7, 11, 13) X(Y20L_KEEP_0, 1, 13) \
	/* Y21 */ \
	X(Y21_LH_POS, 17, 23) X(Y21_LH_NEG, 17, 23) X(Y21_LH_P8_TEN, 17, 23) X(Y21_LH_P8_PAIR, 17, 23) X(Y21_LH_N8_NINE, 17, 23) X(Y21_LH_N8_PAIR, 17, 23) \
	X(Y21_HL_POS, 17, 23) X(Y21_HL_NEG, 17, 23) X(Y21_HL_P8_TEN, 20, 23) X(Y21_HL_N8_NINE, 20, 23) /* (up to quality 19 Y20 has made HL1's +-8 a +-7) */ \
	/* Y22: the chain's arms in its order */ \
	X(Y22_MARK_22, 13, 23) X(Y22_MARK_23, 13, 23) X(Y22_MARK_33, 13, 23) X(Y22_SNAP_33, 19, 23) \
	X(Y22_INC_AM4, 13, 23) X(Y22_MARK_AM4, 13, 23) X(Y22_MARK_ABOVE_P, 13, 23) \
	X(Y22_SNAP_125, 13, 23) X(Y22_SNAP_121, 19, 23) X(Y22_Q18P_BELOW_A5, 18, 18) X(Y22_Q18P_CELL, 18, 18) X(Y22_Q18P_BELOW_R3, 18, 18) \
	X(Y22_MARK_NB_P, 13, 23) \
	X(Y22_DEC_A4, 13, 23) X(Y22_MARK_A4, 13, 23) \
	X(Y22_SNAP_126, 13, 23) X(Y22_SNAP_122, 19, 23) X(Y22_Q18N_BELOW_A5, 18, 18) X(Y22_Q18N_CELL, 18, 18) X(Y22_Q18N_BELOW_R3, 18, 18) \
	X(Y22_MARK_NEG_D2, 13, 23) X(Y22_CODE_145, 21, 23) X(Y22_MARK_NB_N, 13, 23) X(Y22_SITE_M2_A, 13, 23) X(Y22_SITE_M3_A, 13, 20) \
	X(Y22_MARK_ABOVE_N, 13, 23) X(Y22_MARK_M1_D3, 13, 23) X(Y22_SITE_UP_A, 13, 23) X(Y22_MARK_M4, 13, 23) X(Y22_SITE_LARGE_A, 13, 23) \
	X(Y22_SITE_UP_B, 13, 23) X(Y22_SITE_M2_B, 13, 23) X(Y22_SITE_M3_B, 13, 23) X(Y22_SITE_LARGE_B, 13, 23) \
	/* the nudges of the LH1 partner */ \
	X(NUDGE_UP_7, 13, 23) X(NUDGE_UP_8, 13, 23) X(NUDGE_M2_NEG, 13, 23) X(NUDGE_M2_POS, 13, 23) \
	X(NUDGE_M3_145, 21, 23) X(NUDGE_M3_NEG, 13, 20) X(NUDGE_M3_TEN, 13, 20) X(NUDGE_M3_BIG, 13, 20) \
	X(LARGE_M4, 13, 23) X(LARGE_149, 21, 23) X(LARGE_NEG, 13, 23) X(LARGE_POS, 13, 23) \
	/* Y23 */ \
	X(Y23_R01, 13, 23) X(Y23_R2_DEC, 13, 23) X(Y23_R2_M78, 13, 23) X(Y23_R2_M6, 13, 23) \
	X(Y23_R3_144, 21, 23) X(Y23_R3_DEC, 13, 20) X(Y23_R3_M10, 13, 20) \
	X(Y23_141, 13, 23) X(Y23_R4, 20, 23) X(Y23_148, 21, 23) X(Y23_R7_DEC, 13, 23) X(Y23_R7_M9, 13, 23) \
	/* Y24 */ \
	X(Y24_141, 22, 23) X(Y24_140, 22, 23) X(Y24_144, 22, 23) X(Y24_145, 22, 23) X(Y24_121, 22, 23) X(Y24_122, 22, 23) \
	X(Y24_123, 22, 23) X(Y24_124, 22, 23) X(Y24_126, 22, 23) X(Y24_125, 22, 23) X(Y24_148, 22, 23) X(Y24_149, 22, 23) \
	/* Y27: the ripple, then the three bands (LH1's and HL1's pull to +-7 needs |v| in 6 .. lim2 - 1, and lim2 is 4 at quality 23) */ \
	X(RIPPLE_DEC, 1, 23) X(RIPPLE_M7_8, 1, 23) X(RIPPLE_NEG_7, 1, 23) X(RIPPLE_NEG_AHEAD, 1, 23) \
	X(Y27_LH_TO_M7, 1, 22) X(Y27_LH_TO_7, 1, 22) X(Y27_LH_ZERO, 1, 23) X(Y27_HL_TO_7, 1, 22) X(Y27_HL_ZERO, 1, 23) \
	X(Y27_HH_TO_7, 1, 23) X(Y27_HH_ZERO, 1, 23)
#define NHWO_ARM_ENUM(name, lo, hi) ARM_##name,
enum { NHWO_ARMS(NHWO_ARM_ENUM) ARM_COUNT };
extern uint32_t nhwo_arm[NHWO_ARM_MAX];
#define ARM(name) (nhwo_arm[ARM_##name]++)

/* trace */
void nhwo_trace_put(nhwo_trace *t, const char *name, int nblobs, const void **blobs, const uint32_t *lens);
static inline void trace_planes(nhwo_ctx *c, const char *name, const void *a, uint32_t la, const void *b, uint32_t lb)
{
	const void *bl[2]; uint32_t ln[2]; int n = 0;
	if (!c->trace) return;
	if (a) { bl[n] = a; ln[n++] = la; }
	if (b) { bl[n] = b; ln[n++] = lb; }
	nhwo_trace_put(c->trace, name, n, bl, ln);
}

/* stages */
void nhwo_prefilter_chroma(int16_t *plane, int quality);        /* pre_processing_UV */
void nhwo_dequant_sim_luma(nhwo_ctx *c, int part);              /* offsetY_recons256 */
void nhwo_dequant_sim_chroma(nhwo_ctx *c, int comp);            /* offsetUV_recons256 */
void nhwo_quantise_luma(nhwo_ctx *c);                           /* offsetY */
void nhwo_quantise_chroma(nhwo_ctx *c);                         /* offsetUV */
void nhwo_ll_code_luma(nhwo_ctx *c);                            /* Y_highres_compression */
void nhwo_ll_code_chroma(nhwo_ctx *c);                          /* highres_compression */
int  nhwo_packetise(nhwo_ctx *c);                               /* wavlts2packet */
void nhwo_rewrite_stream(nhwo_ctx *c);                          /* the symbol rewrites in the middle of encode_image */
void nhwo_band_recons(nhwo_ctx *c);                             /* im_recons_wavelet_band */
void nhwo_hq_settings(nhwo_ctx *c);                             /* wavelet_synthesis_high_quality_settings */
void nhwo_poslist_finish(nhwo_ctx *c, nhwo_poslist *pl, uint8_t *raw, int raw_len, const uint8_t *payload,
                         int payload_len, int word_mode);
int  nhwo_luma(nhwo_ctx *c);
int  nhwo_chroma(nhwo_ctx *c, int comp);
size_t nhwo_container(nhwo_ctx *c, uint8_t *out, size_t cap);   /* write_compressed_file */

#endif
