/* nhw_ws.h -- device workspace layout shared by the kernels of libnhwhip.so (gfx950 only). */
#ifndef NHW_WS_H
#define NHW_WS_H

#include <hip/hip_runtime.h>
#include <assert.h>
#include <stdint.h>

#include "nhw_buf.h"   /* the B_* names of the buffers */

#define W  512      /* luma row stride  (reference 2*IM_DIM) */
#define H  256      /* chroma row stride (reference IM_DIM) */
#define Q  65536    /* reference IM_SIZE */
#define DEADZONE 8  /* reference `ratio`: nhw_encoder_cli.c:177 */
#define GUARD 4096  /* zero bytes kept behind every logical buffer: the reference's out-of-bounds reads
                        land here and return 0, the canonical-oracle semantics */

/* Per-image buffers are laid out structure-of-arrays over the batch: buffer b of image i lives at
 * base + off[b] + i * stride[b], stride[b] = size + GUARD rounded to 256 B, and GUARD zero bytes precede
 * image 0.  The guards are never written, so they stay zero between batches. */
/* The buffers' numbers are an interface: nhw_debug_read, nhw_debug_write, nhw_debug_hash and nhw_debug_fill take them, and the stage tests read
 * them out of this list.  It restates the order of nhw_buf.h; a name that moves there without moving here does not compile (a division by zero
 * in a constant expression). */
enum {
	NHW_WS_BUFFER_ORDER = 1 / (int)(
		B_JPEG == 0 && B_PROC == 1 && B_PU == 2 && B_PV == 3 && B_CJPEG == 4 && B_CPROC == 5 && B_LL1 == 6 && B_L2SAVE == 7 && B_CLL1 == 8 &&
		B_CL2SAVE == 9 && B_KEEP == 10 && B_FIRST == 11 && B_BAND == 12 && B_HS == 13 && B_KMAP == 14 && B_ROWMAP == 15 && B_ROWSTATE == 16 &&
		B_SCAN == 17 && B_LLBYTES == 18 && B_LLFULL == 19 && B_EXW == 20 && B_LLCOMP == 21 && B_LLWORD == 22 && B_LLMEM == 23 && B_RES4 == 24 &&
		B_RAW == 25 && B_PAY == 26 && B_CC == 27 && B_HALF == 28 && B_TMP16 == 29 && B_R1LIST == 30 && B_R1BITS == 31 && B_R1WORD == 32 &&
		B_R3LIST == 33 && B_R3BITS == 34 && B_R3WORD == 35 && B_R5LIST == 36 && B_R5BITS == 37 && B_R5WORD == 38 && B_R6LIST == 39 && B_R6BITS == 40 &&
		B_R6WORD == 41 && B_CHARRES == 42 && B_QSET3 == 43 && B_RESU64 == 44 && B_RESV64 == 45 && B_PACKET == 46 && B_BOOK1 == 47 && B_BOOK2 == 48 &&
		B_SEL1 == 49 && B_SEL2 == 50 && B_S1 == 51 && B_S2 == 52 && B_HIST == 53 && B_META == 54 && B_PROF == 55 && B_ROWFLAG == 56 && B_SEGMAP == 57 &&
		B_STALE == 58 && B_NZQ == 59 && B_NZS == 60 && B_VOFF == 61 && B_VALS == 62 && B_CNZQ == 63 && B_CVALS == 64 && B_CJPEG_V == 65 &&
		B_CPROC_V == 66 && B_CLL1_V == 67 && B_CL2SAVE_V == 68 && B_UBYTES == 69 && B_LOWTAB == 70 && B_CPACK == 71 && B_CPACKET == 72 && B_COUNT == 73)
};

/* B_CPACK of an image.  k_pack_chroma runs while the luma tail still owns B_NZS / B_VOFF (Y31) and B_RAW (Y25): everything it writes lies here
 * and in B_CPACKET.  k_final reads the four scalars and the ranked entries. */
struct NhwChromaPack {
	uint64_t nzs[2048];          /* the chroma part's map in stream order (pack_chroma_order) */
	uint32_t voff[2048];
	int gaps[2 * (2048 + 8)];    /* last non-zero symbol before / first at-or-after a slice (pack_words_par) */
	uint16_t sorted[360];        /* book 2's entries by rank */
	int k, rc, nwords, last;     /* entries; the part's status; its packet words; its last word that carries bits (-1: none): the capacity rule's `last` */
};

/* scalar per-image state (reference encode_state / codec_setup scalars), one struct per image in B_META */
struct NhwPosLens { int list_len, bits_len, word_len; };
struct NhwMeta {
	int exw_len, res4_len;
	NhwPosLens r1, r3, r5, r6;
	int char_res1_len, qsetting3_len;
	int ll_comp_y_len, ll_word_len, ll_mem_len, ch_res_len;
	int res_low, res_high, wavelet_type;
	int select1, select2;
	int size_data1, size_data2, size_book1, size_book2, tree_end;
	int status;
	int pad;
};

template <class T> struct Plane;   /* nhw_host.h: how the host's launch layer passes one buffer of every image */
struct NhwWs {
	uint8_t *base;
	size_t off[B_COUNT];
	size_t stride[B_COUNT];
	int n;
	int q;
	int dbg;      /* the batch driver is stopped after a stage (tests): kernels also write the planes that nothing but a test reads */
	int split_chroma;     /* the V sequence works in planes of its own (B_*_V), so that its head -- everything up to the second dequantiser simulation -- runs right behind U's instead of behind U's quantiser, which waits for the luma tail's exception list; the stage checks keep the reference's one set of planes */
	int defer_verbatim;   /* the LL2 coder (Y16) runs beside the second dequantiser simulation: the samples it sent verbatim are put back by the synthesis behind both (k_dwt_syn) */
	int compat;   /* 0: canonical (out-of-bounds reads see zeros); 1: the heap neighbours of the stock one-image-per-process binary (nhw_hip.h) */
	template <typename T> __host__ __device__ T *buf(int b, int img) const { return (T *)(base + off[b] + (size_t)img * stride[b]); }
	template <typename T> Plane<T> plane(int b) const { assert(stride[b] % sizeof(T) == 0); return { (T *)(base + off[b]), stride[b] / sizeof(T) }; }   /* host: buffer b of this view's images */
};


#endif
