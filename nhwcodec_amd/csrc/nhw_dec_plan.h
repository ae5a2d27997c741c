/*
 * nhw_dec_plan.h -- what one decoder batch enqueues, worked out on the host before anything is launched: the one place where the decoder's
 * launch sequence is stated.  dec_plan() is a pure function from what decides the sequence -- the scale, grey or
 * colour, the debug stop, the NHW_DEC_FORK bits -- to a short list of steps: a kernel, an event operation or a timing stamp, on the caller's
 * stream or the handle's second one.  Whether the last kernel stores bytes or a tensor format changes no step and is no input.  dec_batch
 * (nhw_dec.hip) runs the list; dec_access() below says what every kernel reads and writes, and tests/dec_plan/check.cpp holds every plan of
 * the domain against that table on the CPU: no kernel beside or in front of one that writes what it touches.  No HIP header.
 */
#ifndef NHW_DEC_PLAN_H
#define NHW_DEC_PLAN_H

#include <assert.h>
#include <stdint.h>

/* ------------------------------------------------------------------------------------------------ the steps */
enum DecOp {
	DEC_STAMP,        /* record timing event ev[arg] (arg 0 .. 3) */
	DEC_FORK,         /* record fork_ev on the caller's stream and make the second stream wait for it */
	DEC_JOIN_RECORD,  /* record join_ev on the second stream */
	DEC_JOIN_WAIT,    /* make the caller's stream wait for join_ev */
	DEC_PARSE, DEC_VLC, DEC_VERDICT, DEC_EXPAND,
	DEC_CHROMA,       /* k_dec_chroma, arg = upto: 1 .. 3 the debug stops, 4 everything, 5 the quarter scale's exit */
	DEC_SHARPEN,
	DEC_L2Q,          /* k_dec_luma_l2q<arg>: 1, 2 the debug stops, 3 production */
	DEC_MARKS, DEC_MARKS_FAR,
	DEC_LAST,         /* the last kernel, arg = the scale: k_dec_final (1) or k_dec_scaled<arg> (2, 4), with the call's store */
	DEC_STATUS,
	DEC_OP_COUNT
};
struct DecStep { uint8_t op, side /* 0: the caller's stream, 1: the handle's second one */, arg; };
enum { DEC_PLAN_CAP = 24 };                                       /* the longest plan (scale 1, colour, bits 3) has 21 steps */
struct DecPlan {
	int n;                                                        /* 0: the input lies outside the domain */
	DecStep step[DEC_PLAN_CAP];
	bool timed;                                                   /* the last kernel is in the plan: the four stamps are (nhw_dec_last_timing) */
	bool l1_moved;                                                /* k_dec_luma_l2q is in the plan (nhw_dec_debug_read) */
};

/* The plan of a batch.  The domain is what the entry points admit: scale 1, 2 or 4; stop 0 (run everything) .. 11, and a stop other than 0
 * only at scale 1 and not grey; of bits only the low three count.  Outside the domain the plan is EMPTY (n = 0), and the caller refuses.
 *
 * The bits (NHW_DEC_FORK): 1 the two entropy branches side by side; 2 the chroma sequence beside the luma's whole sequence (scale 1, colour);
 * 4 the chroma sequence behind the luma's level 2, beside the smooth-edge marks only (scale 1, colour, and not with bit 2).  A debug stop
 * keeps everything in line, and so does what a bit does not apply to.  A debug stop k ends the plan behind stage k (tests/dec_stages.py);
 * stops 3, 4 / 5 and 8 / 9 also end a kernel early so that the stage's planes can be read.
 * Grey: no chroma kernel, no sharpen, nothing on the second stream but the prefix-code walk under bit 1. */
inline DecPlan dec_plan(int scale, bool grey, int stop, int bits)
{
	DecPlan p = {};
	if ((scale != 1 && scale != 2 && scale != 4) || stop < 0 || stop > 11 || (stop && (scale != 1 || grey))) return p;
	const bool whole = scale == 1 && !grey && !stop;                /* what bits 2 and 4 apply to */
	const bool fork_e = (bits & 1) && !stop, fork = (bits & 2) && whole, fork_late = (bits & 4) && whole && !fork;
	auto put = [&](int op, int side = 0, int arg = 0) {
		assert(p.n < DEC_PLAN_CAP);
		p.step[p.n++] = { (uint8_t)op, (uint8_t)side, (uint8_t)arg };
		if (op == DEC_LAST) p.timed = true;
		if (op == DEC_L2Q) p.l1_moved = true;
	};
	auto chroma_sequence = [&](int side) { put(DEC_CHROMA, side, 4); put(DEC_SHARPEN, side); };   /* the chroma planes up to the bytes the colour kernels read */
	auto status = [&]() { put(DEC_STATUS); return p; };
	auto last = [&]() { put(DEC_STAMP, 0, 2); put(DEC_LAST, 0, scale); put(DEC_STAMP, 0, 3); return status(); };

	put(DEC_STAMP, 0, 0);
	/* two entropy branches that only meet at the verdict: the side streams (LL2 DPCM, position lists) and the prefix-code walk */
	if (fork_e) put(DEC_FORK);
	put(DEC_PARSE);
	if (stop == 1) return status();
	put(DEC_VLC, fork_e);
	if (fork_e) { put(DEC_JOIN_RECORD, 1); put(DEC_JOIN_WAIT); }
	put(DEC_VERDICT);
	if (fork) put(DEC_FORK);                                       /* behind the verdict: k_dec_chroma reads the status it settles */
	put(DEC_STAMP, 0, 1);
	if (stop == 2) return status();
	put(DEC_EXPAND);
	if (scale == 4) {                                              /* quarter scale: the level-2 LL is in plane A already; the chroma planes up to their corrections */
		if (!grey) put(DEC_CHROMA, 0, 5);
		return last();
	}
	if (fork) { chroma_sequence(1); put(DEC_JOIN_RECORD, 1); }
	if (stop == 3) { put(DEC_CHROMA, 0, 1); return status(); }     /* the chroma planes as the expansion leaves them */
	put(DEC_L2Q, 0, stop == 4 ? 1 : stop == 5 ? 2 : 3);             /* stops 4 (behind the shrink), 5 (behind the synthesis), 6 */
	if (stop >= 4 && stop <= 6) return status();
	if (scale == 2) {                                              /* half scale: the level-1 LL and the chroma sequence in line; no marks, no level 1 of the luma */
		if (!grey) chroma_sequence(0);
		return last();
	}
	if (fork_late) { put(DEC_FORK); chroma_sequence(1); put(DEC_JOIN_RECORD, 1); }
	put(DEC_MARKS);
	put(DEC_MARKS_FAR);                                            /* (ends at once for every file but one whose level-1 LL leaves -5999 .. 10000) */
	if (stop == 7) return status();
	if (fork || fork_late) put(DEC_JOIN_WAIT);
	else if (!grey) {
		put(DEC_CHROMA, 0, stop == 8 ? 2 : stop == 9 ? 3 : 4);      /* stops 8 (behind level 2), 9 (behind the corrections), 10 */
		if (stop >= 8 && stop <= 10) return status();
		put(DEC_SHARPEN);
		if (stop == 11) return status();
	}
	return last();
}

/* ------------------------------------------------------------------------------------------------ what the kernels touch
 * A resource is a workspace buffer (the D_* list of nhw_dec.hip), one of the caller's arrays, or a named part of a buffer where two kernels
 * that some plan runs side by side touch different parts of it.  The rows are read off the kernels' text -- every ws.buf<...>(D_x, ...),
 * plane_a, plane_l1, plane_ca, mark_rows, l1_far_flag, walk_verdict and ws.blob in a kernel and in the device functions it calls -- by hand:
 * nothing holds the table against the kernels, so a kernel that comes to touch another buffer needs its row changed with it.
 * (The prefix code's lookup table, written once when the handle is made, is no resource of a batch.) */
enum DecRes : uint32_t {
	R_BLOB = 1u << 0,          /* the caller's files, offsets and lengths */
	R_OUT = 1u << 1, R_STATUS = 1u << 2, R_QUALITY = 1u << 3,       /* the caller's pixels, status and quality */
	/* D_META in two parts.  HDR: every member of DecMeta but nmarks -- status, q and the header's lengths and offsets, which k_dec_parse writes
	 * (`*gm = sm`), k_dec_verdict updates (`m->status = v`) and every later kernel reads (`if (m->status) return`, `m->q`, `m->o_...`).  NMARKS: the
	 * member nmarks, which k_dec_parse zeroes with the rest, marks_walk writes (`m->nmarks = total`, its last line) and k_dec_final reads (`const
	 * int nmarks = m->nmarks`).  The split is what lets k_dec_marks run beside k_dec_chroma and k_dec_sharpen under bit 4, the default. */
	R_META_HDR = 1u << 4, R_META_NMARKS = 1u << 5,
	R_LL = 1u << 6,
	R_SPARE = 1u << 7,         /* the walk's two verdict words, the far flag, mark_rows */
	R_P1 = 1u << 8, R_P3 = 1u << 9, R_P5 = 1u << 10, R_P6 = 1u << 11,
	R_MARKS = 1u << 12,
	R_A = 1u << 13,
	/* D_B is two things in turn: the luma value list that k_dec_vlc writes and k_dec_expand reads (`ent = ws.buf<uint32_t>(D_B, img)`), and, once
	 * k_dec_expand is through, plane_l1: the level-1 LL that k_dec_luma_l2q writes over it.  One resource under two names, so that the kernel
	 * that writes the second is held behind the readers of the first. */
	R_B_LIST = 1u << 14, R_B_L1 = R_B_LIST,
	R_CA = 1u << 15, R_CB = 1u << 16, R_CU = 1u << 17,
	R_SEG = 1u << 18,          /* the luma strips' index and the chroma list's total */
	R_NZG = 1u << 19,
};
struct DecAccess { uint32_t reads, writes; };

/* what step (op, arg) of a grey or colour plan reads and writes; nothing for the event operations and the stamps */
inline DecAccess dec_access(int op, int arg, bool grey)
{
	switch (op) {
	case DEC_PARSE:      /* the header record, the four side streams */
		return { R_BLOB, R_META_HDR | R_META_NMARKS | R_LL | R_P1 | R_P3 | R_P5 | R_P6 };
	case DEC_VLC:        /* reads the file's header itself, not D_META; its verdict words, the two value lists, their index */
		return { R_BLOB, R_SPARE | R_B_LIST | R_CB | R_SEG };
	case DEC_VERDICT:    /* the verdict words -> the status; clears the far flag */
		return { R_SPARE | R_META_HDR, R_SPARE | R_META_HDR };
	case DEC_EXPAND:     /* the luma list, the LL2 samples, the tags and exception samples of the file -> plane A and its group map */
		return { R_META_HDR | R_BLOB | R_B_LIST | R_SEG | R_LL | R_A, R_A | R_NZG };
	case DEC_CHROMA:     /* every upto: the chroma list, the chroma LL2 samples, the file's exception samples -> the planes */
		return { R_META_HDR | R_BLOB | R_CB | R_SEG | R_LL, R_CA };
	case DEC_SHARPEN:
		return { R_META_HDR | R_CA, R_CU };
	case DEC_L2Q:        /* plane A's block -> plane_l1; UPTO 3: the residual lists (res_list) and the far flag (atomicOr) */
		if (arg < 3) return { R_META_HDR | R_A, R_B_L1 };
		return { R_META_HDR | R_A | R_BLOB | R_P1 | R_P3 | R_P5 | R_SPARE, R_B_L1 | R_SPARE };
	case DEC_MARKS:      /* the far flag, plane_l1 -> the list, mark_rows, nmarks */
		return { R_META_HDR | R_SPARE | R_B_L1, R_MARKS | R_SPARE | R_META_NMARKS };
	case DEC_MARKS_FAR:  /* the same walk, which also writes back the cells it changes */
		return { R_META_HDR | R_SPARE | R_B_L1, R_MARKS | R_SPARE | R_META_NMARKS | R_B_L1 };
	case DEC_LAST:
		if (arg == 1) return { R_META_HDR | R_META_NMARKS | R_A | R_B_L1 | R_NZG | R_BLOB | R_P6 | R_MARKS | R_SPARE | (grey ? 0u : R_CU), R_OUT };
		if (arg == 2) return { R_META_HDR | R_B_L1 | (grey ? 0u : R_CU), R_OUT };
		return { R_META_HDR | R_A | (grey ? 0u : R_CA), R_OUT };
	case DEC_STATUS:
		return { R_META_HDR, R_STATUS | R_QUALITY };
	default:
		return { 0, 0 };
	}
}

#endif
