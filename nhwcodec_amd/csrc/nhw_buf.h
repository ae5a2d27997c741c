/* nhw_buf.h -- the names of the encoder workspace's per-image buffers.  No HIP header: nhw_ws.h (the device side's layout) and nhw_enc_plan.h
 * (the host-only launch plan and its access table) both include it. */
#ifndef NHW_BUF_H
#define NHW_BUF_H

enum {
	B_JPEG, B_PROC, B_PU, B_PV, B_CJPEG, B_CPROC, B_LL1, B_L2SAVE, B_CLL1, B_CL2SAVE, B_KEEP, B_FIRST, B_BAND,
	B_HS, B_KMAP, B_ROWMAP, B_ROWSTATE, B_SCAN, B_LLBYTES, B_LLFULL, B_EXW, B_LLCOMP, B_LLWORD, B_LLMEM, B_RES4,
	B_RAW, B_PAY, B_CC, B_HALF, B_TMP16,
	B_R1LIST, B_R1BITS, B_R1WORD, B_R3LIST, B_R3BITS, B_R3WORD, B_R5LIST, B_R5BITS, B_R5WORD,
	B_R6LIST, B_R6BITS, B_R6WORD, B_CHARRES, B_QSET3,
	B_RESU64, B_RESV64, B_PACKET, B_BOOK1, B_BOOK2, B_SEL1, B_SEL2, B_S1, B_S2, B_HIST, B_META, B_PROF, B_ROWFLAG, B_SEGMAP, B_STALE,
	B_NZQ, B_NZS, B_VOFF, B_VALS, B_CNZQ, B_CVALS,   /* the luma symbol stream as a list (nhw_tail_wave.h, wave_quantise_luma): non-zero map as the quantiser writes it, the map and the value offsets in stream order (Y31), the values; CNZQ / CVALS: the chroma part's map and values as the chroma quantiser leaves them */
	B_CJPEG_V, B_CPROC_V, B_CLL1_V, B_CL2SAVE_V, B_UBYTES,   /* the V plane's own copies of the four chroma work planes (production: NhwWs::split_chroma); UBYTES: where the chroma quantiser parks U's symbols until V's come (it used the band plane, and above q21 waited for Y29 to be through with it) */
	B_LOWTAB,   /* quality 1..16: the candidate masks pass A of the pre-filter leaves for its order-dependent cells (nhw_low.hip, k_low_pre -> k_low_mapfix): 320 bytes a row */
	B_CPACK, B_CPACKET,   /* the chroma packetiser's own (k_pack_chroma, NhwChromaPack in nhw_ws.h): its map and value offsets in stream order, its scratch and what it leaves for k_final; its packet words from word 0 on (a chroma part alone may hold 80000 words) */
	B_COUNT
};

#endif
