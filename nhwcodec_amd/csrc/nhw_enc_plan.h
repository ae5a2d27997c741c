/*
 * nhw_enc_plan.h -- what one encoder batch enqueues, worked out on the host before anything is launched: the one place where the encoder's
 * launch sequence is stated.  enc_plan() is a pure function from what decides the sequence -- the quality, the debug
 * stop, the compatibility mode, which part of the sequence is asked for and how it is timed, whether the batch is large, and the schedule
 * switches of the handle -- to a list of steps: a kernel launch, an event record or wait, a timing stamp or a stage boundary, each on one of
 * four streams.  run_batch (nhw_enc.hip) runs the list; enc_access() below says what every kernel step reads and writes, and
 * tests/enc_plan/check.cpp holds every plan of the domain against that table on the CPU: no kernel beside or in front of one that writes what it
 * touches.  The reasons why two kernels may run side by side stand here, next to the step they justify.  No HIP header.
 */
#ifndef NHW_ENC_PLAN_H
#define NHW_ENC_PLAN_H

#include <assert.h>
#include <stdint.h>

#include <bitset>
#include <initializer_list>

#include "nhw_buf.h"

/* ------------------------------------------------------------------------------------------------ the steps */
enum EncStream {
	ES_MAIN,          /* the caller's stream (a sub-batch: its own) */
	ES_CHROMA,        /* the chroma sequence beside the luma tail (part_stream[0]) */
	ES_LISTS,         /* the position lists Y24 / Y25 (part_stream[1]) */
	ES_LL,            /* the LL2 coder Y16; before it Y5, behind it the chroma packetiser (ll_stream) */
	ES_COUNT
};
/* The events a plan records and waits for.  The first seven are the stamps of nhw_timing (the EV_* of nhw_enc.h, same numbers): a stamp is an
 * event like any other, and the chroma fork waits for two of them. */
enum EncEvent {
	EE_START, EE_FRONT, EE_LUMA, EE_CHROMA, EE_END, EE_COLOR, EE_PREFILTER,
	EE_LUMA_LIST,     /* the luma plane's exception list is complete, and the LL2 coder through with the bytes behind the luma samples */
	EE_CHROMA_DONE,   /* the chroma stream is through */
	EE_LISTS_FORK, EE_LISTS,
	EE_LL_FORK, EE_LL_DONE, EE_Y5_FORK, EE_Y5_DONE, EE_PACK_FORK, EE_PACK_DONE,
	EE_LOW_PASS_A,    /* quality 1 .. 16, the pre-filter in sub-batches: the last sub-batch is through its pass A.  Recorded INSIDE the step
	                   * ENC_LOW_PREFILTER (nhw_launch_low_prefilter, on a stream of its own), behind the colour kernel and in front of nothing of that step */
	EE_PART_FRONT,    /* a `what = 2` plan only: the front group of the whole batch is through.  Recorded by the sub-batch loop, not by the plan */
	EE_COUNT
};
enum EncOp {
	ENC_STAMP,          /* record the timing event a (EE_START .. EE_PREFILTER) */
	ENC_RECORD,         /* record event a on the step's stream */
	ENC_WAIT,           /* make the step's stream wait for event a */
	ENC_STAGE,          /* a boundary the debug stop counts (nhw_debug_stop_after); no work */
	/* the front group */
	ENC_COLOR,          /* k_color.  a = 0: luma into B_JPEG (quality 1 .. 16); 1: into B_KMAP (the compatibility mode's replay, quality 17 .. 21) */
	ENC_LOW_PREFILTER,  /* nhw_launch_low_prefilter.  a = its sub-batches (lparts), b = 1: every band takes its exact fallback */
	ENC_LOW_STALE,
	ENC_FRONT,          /* nhw_launch_front_fused, the form the quality selects.  a = 1: every carry segment takes its exact replay (quality 17 .. 23) */
	ENC_FRONT_STALE,
	/* a chroma component.  a = its plane set: 0 U, 1 V in U's planes, 2 V in planes of its own (B_*_V) */
	ENC_C_PREFILTER,    /* quality 1 .. 14 */
	ENC_C_WIDEN,        /* k_phase<PH_C0> */
	ENC_C_ANALYSIS1,    /* level 1 + the copy of LL1.  b = 1: from the byte plane itself */
	ENC_C_THIN,         /* quality 1 .. 16 */
	ENC_C_LOOPS,        /* k_chroma_loops: both closed loops on one residency */
	ENC_C_ANALYSIS2,    /* the staged loops of a debug stop: level 2.  b = 1: + the copy of the block */
	ENC_C_SIM1, ENC_C_SYN, ENC_C_PRECOMP, ENC_C_SIM2,
	ENC_C_TAIL,         /* marks, LL2 emission, quantiser.  b = 1: the one-walk kernel (k_chroma_tail) */
	/* the luma plane */
	ENC_Y4,             /* the first level-2 analysis, from B_LL1.  a = 1: without the transposed first-direction plane */
	ENC_Y5,
	ENC_DQ1,            /* the first dequantiser simulation */
	ENC_L_SYN1, ENC_Y8, /* the staged first loop of a debug stop: synthesis; Y8 + Y9 */
	ENC_L2_RECON,       /* k_l2_recon.  a = 1: + the second analysis and Y13's copy (quality 13 ..), b = 1: its lean form */
	ENC_L_ANALYSIS2,    /* the second level-2 analysis as a kernel of its own.  a = 1: + Y13's copy */
	ENC_LOW_LL2, ENC_COPY_BLOCK,   /* quality 1 .. 12: Y11 / Y12, Y13 */
	ENC_EMIT,           /* Y14, Y15.  a = 1: the LL2 bump walk once, here */
	ENC_LL_CODER,       /* Y16 (+ Y17 where somebody reads it) */
	ENC_DQ0,            /* the second simulation.  a: bit 0 the walk is made (ENC_EMIT a = 1), bit 1 it hands its marks to the quantiser; b = 1: the put-back of verbatim samples is left to ENC_L_SYN2 */
	ENC_L_SYN2,         /* a = 1: without its copy in natural orientation, b = 1: + the put-back of verbatim samples */
	ENC_L4A, ENC_L4B, ENC_L4C,
	ENC_QUANT,          /* Y28 (+ Y30).  a = 1: takes the second simulation's marks */
	ENC_L4C2,           /* Y29, quality 22, 23 */
	ENC_Y31,
	ENC_PACK_CHROMA,    /* Z2's chroma part */
	ENC_LLC,            /* Z1 */
	ENC_FINAL,          /* Z2 + the container.  a = 1: ENC_PACK_CHROMA has run; 0: it is launched here, in front */
	ENC_OP_COUNT
};
inline bool enc_is_kernel(int op) { return op >= ENC_COLOR; }
struct EncStep { uint8_t op, stream, a, b; };
enum { ENC_PLAN_CAP = 160 };                                      /* the longest plan (a debug stop that no boundary reaches, quality 13, the compatibility mode) has 87 steps */

/* what decides the sequence */
struct EncIn {
	int q;                /* 1 .. 23 */
	int stop;             /* the debug stop: 0 = run everything, k = leave behind the k-th stage boundary */
	int compat;           /* 0, 1 */
	int what;             /* bit 0: the front group, bit 1: everything behind it.  1, 2 (a sub-batch's view), 3 */
	int timed;            /* 0: no stage stamp, 1: EE_START .. EE_END, 2: EE_LUMA and EE_CHROMA (the first sub-batch) */
	int big;              /* the batch is large enough for the low pre-filter's sub-batches (n >= 1024) */
	int front_fallback;   /* bit 0 of the debug hook */
	/* the per-batch switches of the handle (nhw_enc_create_ex) */
	int low_chroma, chroma_fork, lists_fork, ll_fork, quant_join, y5_fork, ll2_once, quant_marks, chroma_tail_once, pack_fork, low_parts;
};
struct EncPlan {
	int n;                /* 0: the input lies outside the domain */
	EncStep step[ENC_PLAN_CAP];
	/* what the launches of this plan are made with (NhwWs) and what the driver remembers of it */
	int dbg, split_chroma, defer_verbatim;
	int low_parts_used;   /* the pre-filter's sub-batches: EE_LOW_PASS_A is low_ev_pass_a(low_parts_used - 1) */
	bool timed;           /* a whole batch without a stop: every event nhw_enc_last_timing reads is in the plan */
};

/* a plan under construction: steps are appended until the debug stop or the end of what was asked for closes it */
struct EncBuilder {
	EncPlan p = {};
	int stop = 0, stage = 0;
	bool closed = false;
	void put(int op, int stream = ES_MAIN, int a = 0, int b = 0)
	{
		if (closed) return;
		assert(p.n < ENC_PLAN_CAP);
		p.step[p.n++] = { (uint8_t)op, (uint8_t)stream, (uint8_t)a, (uint8_t)b };
	}
	void record(int ev, int stream) { put(ENC_RECORD, stream, ev); }
	void wait(int ev, int stream) { put(ENC_WAIT, stream, ev); }
	void stamp(int ev) { put(ENC_STAMP, ES_MAIN, ev); }
	void boundary() { put(ENC_STAGE); if (!closed && stop && ++stage == stop) closed = true; }
};

/* A chroma component's launches up to the second dequantiser simulation, on stream cs (enc_plan; nhw_stage_chroma_loops form 0).
 * set: 0 U, 1 V in U's planes, 2 V in planes of its own. */
inline void enc_chroma_head(EncBuilder &b, int q, bool dbg, int set, int cs)
{
	const bool widen_in_analysis = q > 14 && !dbg;                 /* the analysis reads the byte plane itself (the stage checks keep the copy as a stage of its own) */
	if (q <= 14) b.put(ENC_C_PREFILTER, cs, set);                  /* :2263 / :2579 */
	else if (!widen_in_analysis) b.put(ENC_C_WIDEN, cs, set);
	b.boundary();
	b.put(ENC_C_ANALYSIS1, cs, set, widen_in_analysis);            /* + the copy of LL1; production: nor the LL quadrant back into the work plane -- the level-2 analysis reads its copy */
	if (q <= 16) b.put(ENC_C_THIN, cs, set);                       /* :2277-2308 / :2590-2621 */
	b.boundary();
	b.boundary();
	if (!dbg) { b.put(ENC_C_LOOPS, cs, set); return; }             /* both closed loops on one residency of the level-2 block, from the copy of LL1 (k_chroma_loops); the stage checks take the seven kernels */
	b.put(ENC_C_ANALYSIS2, cs, set, 0);
	b.boundary();
	b.put(ENC_C_SIM1, cs, set);
	b.boundary();
	b.put(ENC_C_SYN, cs, set);
	b.boundary();
	b.put(ENC_C_PRECOMP, cs, set);
	b.boundary();
	b.put(ENC_C_ANALYSIS2, cs, set, 1);                            /* + the copy of the level-2 block */
	b.boundary();
	b.boundary();
	b.put(ENC_C_SIM2, cs, set);
	b.boundary();
	b.put(ENC_C_SYN, cs, set);
	b.boundary();
}

/* The luma plane's launches from the first level-2 analysis to the second, on the caller's stream (enc_plan; nhw_stage_luma_loop forms 0, 6;
 * the kernels' comments still call this sequence luma_loop_launches, the function that launched it before the planner).
 * y5_beside: the forked order.  lean: no debug stop, outside the compatibility mode -- the stores of the level-2 block that nothing reads are
 * left out (k_l2_recon). */
inline void enc_luma_loop(EncBuilder &b, int q, bool dbg, bool y5_beside, bool lean)
{
	assert(!lean || !dbg);
	/* Y4: level-2 analysis (:139).  The LL rows come from ll1 (the front's copy of them in natural orientation, res256): outside the stage checks
	 * the front does not write them into the work plane as well, and this analysis fills that quadrant of the work plane itself (its transposed
	 * first-direction plane).  lean, q > 6: the transposed first-direction plane is not stored.  The first dequantiser simulation, the next
	 * kernel that touches the block of jpeg, writes every cell of it (wave_ll2 the LL2 quadrant, wave_dequant_details the rest: the case list
	 * there) in front of its one reader, k_l2_recon; Y5 reads proc and ll1.  (Below q7 there is no simulation and the plane stays.) */
	b.put(ENC_Y4, ES_MAIN, lean && q > 6);
	b.boundary();
	if (q <= 6) return;
	/* first closed loop (:141-283).  Y5 and the first dequantiser simulation need nothing of each other, and the first kernel that needs both
	 * is k_l2_recon (Y8 reads Y5's tags, the synthesis the simulation's plane).  Y5 (luma_p1_par, tag_l2_details_par) reads proc and
	 * read-modify-writes ll1 (compatibility mode: and clears the 512 cells behind ll1); it never touches jpeg.  The simulation
	 * (wave_dequant_sim_luma, part 1) reads proc and writes jpeg; it never touches ll1, and it writes proc only with keep_p, which is the debug
	 * stop's: the forked order has none.  So in the forked order Y5 runs on the LL coder's stream, idle until Y16, beside the simulation. */
	if (y5_beside) {
		assert(!dbg);
		b.record(EE_Y5_FORK, ES_MAIN);
		b.wait(EE_Y5_FORK, ES_LL);
		b.put(ENC_Y5, ES_LL);
		b.record(EE_Y5_DONE, ES_LL);
	} else b.put(ENC_Y5);
	b.put(ENC_DQ1);                                                /* every quality (1..16: rationed low bits, no marking passes) */
	if (y5_beside) b.wait(EE_Y5_DONE, ES_MAIN);                    /* (Y16's later fork onto that stream is behind Y5 by stream order) */
	b.boundary();
	if (dbg) {
		b.put(ENC_L_SYN1);
		b.boundary();
		b.put(ENC_Y8);
		b.boundary();
	} else b.put(ENC_L2_RECON, ES_MAIN, q > 12, lean && q > 12);   /* synthesis + Y8 + Y9 on one residency of the block (the stage checks take the three kernels); q > 12: + the second analysis and Y13 (:623-631), still on that residency */
	if (q <= 12) b.put(ENC_L_ANALYSIS2, ES_MAIN, 0);               /* (Y11 / Y12 follow, and Y13's copy behind them) */
	else if (dbg) b.put(ENC_L_ANALYSIS2, ES_MAIN, 1);              /* + Y13: copy of the coefficient block */
	b.boundary();
}

/* The plan of one call of run_batch.  The domain: q 1 .. 23, any stop (one that no boundary reaches runs everything, with the debug stop's
 * kernels), (what, timed) one of (3, 1) a whole batch, (1, 0) the front group of a
 * batch that runs in sub-batches, (2, 2) and (2, 0) its first and its later sub-batches.  Outside it the plan is EMPTY (n = 0).  The switches
 * are taken as nhw_enc_create_ex leaves them: low_chroma 0 .. 2, pack_fork 0 .. 2, low_parts 1 .. 4, the others 0 or 1. */
inline EncPlan enc_plan(const EncIn &in)
{
	EncBuilder b;
	const int q = in.q, what = in.what, timed = in.timed;
	if (q < 1 || q > 23 || !((what == 3 && timed == 1) || (what == 1 && timed == 0) || (what == 2 && (timed == 0 || timed == 2)))) return b.p;
	const bool dbg = in.stop != 0, compat = in.compat != 0;
	const bool low = q <= 16;      /* integer colour, the rationed pre-filter of image_processing.c:838-2423 and the other quality 1..16 forms (nhw_low.hip) */
	const bool whole = timed == 1 && what == 3 && !in.stop;        /* what every fork applies to: a whole batch on one stream, without a stop */
	b.stop = in.stop;
	b.p.dbg = dbg;
	b.p.timed = what == 3 && !in.stop;
	/* until the pre-filter below runs in sub-batches: the chroma fork never waits on an event of an earlier batch */
	const int lparts = (low && (what & 1) && whole && in.big) ? in.low_parts : 1;   /* (the stage checks and small batches: in line) */
	b.p.low_parts_used = lparts;
	/* The chroma sequence needs nothing of the luma tail except the length of the exception list (its own entries go behind the luma ones,
	 * Y15): it runs on a stream of its own next to the luma tail and fills the issue slots the latency-bound luma kernels leave.  V works in
	 * planes of its own and U's symbols are parked in B_UBYTES until V's quantiser merges them: the sequence waits neither for the band plane
	 * Y29 is done with, nor V's head for U's quantiser. */
	const bool fork = whole && in.chroma_fork;
	/* Y16, the LL2 coder, is a latency-bound parse in front of the vector-bound dequantiser simulation, which only wants its list of verbatim
	 * samples -- at its very end, to put them back into the block.  Production: the coder runs beside the simulation on a stream of its own
	 * and the synthesis behind both does the putting back (defer_verbatim).  Not in the compatibility mode and not below q14, where the coder's
	 * launch also lays out heap neighbours that the passes behind it read (luma_p3_par). */
	const bool fork_ll = fork && q > 13 && !compat && in.ll_fork;
	b.p.defer_verbatim = fork_ll;
	b.p.split_chroma = fork;                                       /* (the stage checks and the in-line order keep the reference's one set of planes) */
	const int cs = fork ? ES_CHROMA : ES_MAIN;
	const int v_set = fork ? 2 : 1;

	if (what & 1) {
		if (timed == 1) b.stamp(EE_START);
		/* a1 + a2 + Y2 + Y3: colour + 4:2:0, pre-filter (q<=21, nhw_encoder.c:116-119), level-1 analysis (:125), LL1 copy (:127-135): ONE kernel
		 * for quality 17..23 (k_front_image with the pre-filter, k_front_plain without: a workgroup walks an image top to bottom).  The luma plane
		 * never reaches HBM.  Quality 1..16: colour kernel -> luma plane, the rationed pre-filter (nhw_low.hip) -> k_front_plain's input plane. */
		if (low) {
			b.put(ENC_COLOR, ES_MAIN, 0);
			b.stamp(EE_COLOR);                                     /* with the front group, whoever brackets it: nhw_timing.color_dwt_ms / prefilter_ms */
			b.boundary();
			/* contrast map -> proc plane, flags -> scan buffer: both free until the band kernel / the quantiser; the pair machine's answers -> the
			 * q >= 22 plane.  lparts > 1: the step records EE_LOW_PASS_A on a stream of its own and joins back into this one */
			b.put(ENC_LOW_PREFILTER, ES_MAIN, lparts, in.front_fallback & 1);
			b.stamp(EE_PREFILTER);
			b.boundary();
			if (compat) b.put(ENC_LOW_STALE);                      /* compatibility mode only: the map cells the stock binary's heap re-uses */
		} else {
			b.stamp(EE_COLOR); b.stamp(EE_PREFILTER);              /* no kernels of their own for colour and pre-filter: both times 0 */
			b.boundary();
			if (q < 22) b.boundary();
		}
		b.put(ENC_FRONT, ES_MAIN, low ? 0 : (in.front_fallback & 1));
		if (!low && compat && q < 22) {   /* compatibility mode only: the kernel-map cells the stock binary's heap re-uses are replayed from a luma plane */
			b.put(ENC_COLOR, ES_MAIN, 1);
			b.put(ENC_FRONT_STALE);
		}
		b.boundary();
		b.boundary();
		if (timed == 1) b.stamp(EE_FRONT);
		if (!(what & 2)) b.closed = true;
	} else b.wait(EE_PART_FRONT, ES_MAIN);                          /* a sub-batch's view: behind the front group of the whole batch */

	if (fork) {
		/* behind the front launch group: that one is bound by vector issue and has nothing to give (and its time is the roofline figure).  Quality
		 * 1..16: behind the colour kernel already (low_chroma 1), or behind the last sub-batch's pass A (2, where the pre-filter runs in
		 * sub-batches) -- the rationed pre-filter's chain (k_low_chain) is one wavefront a picture on the scalar unit and leaves the vector units
		 * and the memory system idle for milliseconds.  The chroma heads read the 4:2:0 byte planes, which the colour kernel has written, and write
		 * the chroma planes, which nothing of the front group touches. */
		b.wait(!low || in.low_chroma == 0 ? EE_FRONT : (in.low_chroma == 2 && lparts > 1) ? EE_LOW_PASS_A : EE_COLOR, cs);
		enc_chroma_head(b, q, dbg, 0, cs);
		enc_chroma_head(b, q, dbg, v_set, cs);                     /* V's head in planes of its own, right behind U's: U's quantiser waits for the luma tail, and this stream stood idle until then */
	}
	enc_luma_loop(b, q, dbg, fork && in.y5_fork, !dbg && !compat);  /* Y4 .. Y10 (+ Y13's copy for q > 12), every order: forked, in line, a sub-batch's view */
	if (q <= 12) {                                                 /* Y11 (q <= 11), Y12, then Y13 */
		b.put(ENC_LOW_LL2);
		b.put(ENC_COPY_BLOCK);
	}
	b.boundary();
	const bool one_walk = fork && q > 12 && in.ll2_once;           /* the LL2 bump walk once, in the emission: the second simulation finds its cells made (wave_emit_ll2) */
	/* The second simulation's two marking blocks are the quantiser's loops 2 and 3 on the same cells (wave_dequant_details): it leaves their
	 * outcome in B_KMAP and the quantiser takes the level-2 details from there.  On wherever the simulation of this very call runs in front of
	 * the quantiser on these planes -- every order above quality 16 (forked, in line, a sub-batch's view: both kernels are on the caller's
	 * stream, and the fit paths come through here) -- and off under a debug stop, whose stage checks read the quantiser's own work plane. */
	const bool marks = q > 16 && !dbg && in.quant_marks;
	b.put(ENC_EMIT, ES_MAIN, one_walk);                            /* Y14, Y15 */
	if (fork_ll) {
		b.record(EE_LL_FORK, ES_MAIN);
		b.wait(EE_LL_FORK, ES_LL);
		b.put(ENC_LL_CODER, ES_LL);
		b.record(EE_LL_DONE, ES_LL);
		b.record(EE_LUMA_LIST, ES_LL);                             /* exception list of the luma plane complete, and the coder through with the bytes behind the luma samples: the chroma emission writes its own there */
	} else {
		b.put(ENC_LL_CODER);
		if (fork) b.record(EE_LUMA_LIST, ES_MAIN);                 /* exception list of the luma plane complete */
	}
	if (q > 12) {                                                  /* second closed loop (:759-779) */
		b.put(ENC_DQ0, ES_MAIN, (one_walk ? 1 : 0) | (marks ? 2 : 0), fork_ll);
		b.boundary();
		if (fork_ll) b.wait(EE_LL_DONE, ES_MAIN);                  /* (the coder is long done: the simulation takes twice its time) */
		b.put(ENC_L_SYN2, ES_MAIN, q <= 21 && !dbg, fork_ll);      /* its copy in natural orientation is only read by Y19 (q > 21, :766-777) */
		b.boundary();
	}
	b.put(ENC_L4A);                                                /* Y19-Y23 */
	/* Y24, Y25: the position lists are read by nothing before the packetiser, and what the pass leaves in the residual-code plane by nobody at
	 * all; below q21 it shares no plane with the passes behind it either (from q21 on its third list and Y27's snapshot both live in the hs
	 * plane, and Y29 needs Y24), so there it runs beside them on a stream of its own.  It does share one scratch buffer with Y31: B_HALF (the
	 * lists' packing, poslist_finish_par; Y31's selected pairs, scan_rewrite_list_par) -- Y31 stands behind the lists' join in either order. */
	const bool fork_lists = fork && q <= 20 && q > 12 && in.lists_fork;
	if (fork_lists) {
		b.record(EE_LISTS_FORK, ES_MAIN);
		b.wait(EE_LISTS_FORK, ES_LISTS);
		b.put(ENC_L4B, ES_LISTS);
		b.record(EE_LISTS, ES_LISTS);
	} else if (q > 12) b.put(ENC_L4B);                             /* Y24, Y25 (:1498) */
	b.put(ENC_L4C);                                                /* Y26, Y27 */
	const bool early_join = fork && in.quant_join;
	const int pack_fork = fork ? in.pack_fork : 0;                 /* every other order: directly in front of k_final (ENC_FINAL a = 0) */
	auto chroma_tail = [&](int set) {                              /* marks, LL2 emission (appends to the exception list), quantiser, stream bytes.  One walk in every unstopped order: nothing in a batch reads cproc behind the chroma tail; the stage checks read the planes */
		b.put(ENC_C_TAIL, cs, set, in.chroma_tail_once && !dbg);
		b.boundary();
	};
	auto chroma_rest = [&]() {
		b.wait(EE_LUMA_LIST, cs);
		chroma_tail(0);
		chroma_tail(v_set);
		/* Z2's chroma part needs V's quantiser and nothing else, and writes only memory of its own (k_pack_chroma): it runs here, while the luma
		 * stream ends its residual passes, instead of inside the packetiser at the very end, where nothing can run beside it.  Beside Z1 on the
		 * LL coder's stream, idle since Y16 (pack_fork 2, the default), or behind Z1 on this stream (1); either way it is through before the
		 * join.  0: in front of k_final, as in every other order. */
		if (pack_fork == 2) {
			b.record(EE_PACK_FORK, cs);
			b.wait(EE_PACK_FORK, ES_LL);
			b.put(ENC_PACK_CHROMA, ES_LL);
			b.record(EE_PACK_DONE, ES_LL);
		}
		b.put(ENC_LLC, cs);                                        /* Z1: the chroma LL2 coder appends to the luma one's output (Y16, long done) */
		if (pack_fork == 1) b.put(ENC_PACK_CHROMA, cs);
		if (pack_fork == 2) b.wait(EE_PACK_DONE, cs);
		b.record(EE_CHROMA_DONE, cs);
	};
	/* The quantiser is a wavefront an image at 119 registers: four wavefronts fill a SIMD's register file, and it is as fast as its slowest
	 * wavefront is late.  A side stream's workgroup that sits on a CU when it starts keeps four of its images waiting for a second round.  So
	 * the side streams are let finish first (they have had the multi-round kernels Y19-Y27 to hide behind), and Y31 and the packetiser then
	 * run alone as well. */
	if (early_join) {
		chroma_rest();
		if (fork_lists) b.wait(EE_LISTS, ES_MAIN);
		b.wait(EE_CHROMA_DONE, ES_MAIN);
	}
	b.put(ENC_QUANT, ES_MAIN, marks);                              /* Y28 (+ Y30: the symbols leave in stream order), every quality */
	if (q > 21) b.put(ENC_L4C2);                                   /* Y29 */
	if (fork && !early_join) chroma_rest();                        /* queued here so that the wait finds its event recorded */
	if (fork_lists && !early_join) b.wait(EE_LISTS, ES_MAIN);      /* in front of Y31, which writes B_HALF as the lists' packing does (until the planner this wait stood behind Y31: DESIGN.md 4.9) */
	b.put(ENC_Y31);                                                /* Y31 (Y30, the stream order, is the quantisers' output order) */
	b.boundary();
	if (timed) b.stamp(EE_LUMA);
	if (fork) { if (!early_join) b.wait(EE_CHROMA_DONE, ES_MAIN); }
	else
		for (int comp = 0; comp < 2; comp++) {                     /* U then V (:2255-2570, :2572-2868) */
			enc_chroma_head(b, q, dbg, comp, cs);
			chroma_tail(comp);
		}
	if (timed) b.stamp(EE_CHROMA);
	if (!fork) b.put(ENC_LLC);                                     /* Z1 */
	b.put(ENC_FINAL, ES_MAIN, pack_fork != 0);                     /* Z2, container */
	if (timed == 1) b.stamp(EE_END);
	return b.p;
}

/* ------------------------------------------------------------------------------------------------ what the kernels touch
 * A resource is a workspace buffer (its B_* number), one of the caller's arrays, or a named part of a buffer where two steps that some plan
 * leaves unordered touch different parts of it.  The rows are read off the kernels' text BY HAND -- the planes a launcher is handed
 * (nhw_enc.hip's executor, nhw_host.h), and every member of Ctx (nhw_tail_dev.h, ctx_load: member -> buffer) that a kernel's body and the
 * device functions it calls name -- and nothing holds the table against the kernels: a kernel that comes to touch another buffer needs its row
 * changed with it.  Where a row could not be narrowed without reading a long body it names MORE than the kernel touches (a buffer read is
 * listed as written, a staged debug kernel is given every plane of its component): that can only make the check report a pair, never hide one.
 * Not resources: B_PROF (developer builds' timers), the guard bytes, the look-up tables in constant memory.
 *
 * B_META is the one buffer in parts, because the streams of the forked order own different scalars of NhwMeta (nhw_ws.h):
 *   R_META_EXW   exw_len, res4_len, pad.  wave_emit_ll2 `c->m->res4_len = ...; c->m->exw_len = e`; chroma_ll2_emit_par `const int e0 =
 *                c->m->exw_len ... c->m->exw_len = e0 + 2 + 3 * (int)total`; chroma_marks_par `c->m->pad = ...`; container_par reads them.
 *   R_META_POS   r1, r3, r5, r6, char_res1_len, qsetting3_len.  poslist_finish_par `pl->len->list_len = ...` (pl->len = &m->r1 ...: ctx_load);
 *                luma_p4c2_par `c->m->qsetting3_len = ...; c->m->char_res1_len = ...`.  What lets Y24 / Y25 on the lists' stream run beside
 *                the chroma tail's `exw_len` on the chroma stream.
 *   R_META_LL    ll_comp_y_len, ll_word_len, ll_mem_len, res_low: Y16's.  ll_code_luma_par `c->m->res_low = mode; c->m->ll_comp_y_len = ...;
 *                c->m->ll_word_len = ...; c->m->ll_mem_len = ...`; wave_ll2_verbatim `const int nm = c->m->ll_mem_len` and k_dwt_syn's verb_len
 *                read ll_mem_len; ll_code_chroma_par reads `c->m->ll_comp_y_len` and `c->m->res_low`.
 *   R_META_CH    res_high, ch_res_len: Z1's.  ll_code_chroma_par `c->m->res_high = c->m->res_low; c->m->ch_res_len = j + 1 + (int)total`.
 *                Apart from R_META_LL because, where Y16 runs in line (quality 13, the compatibility mode, ll_fork off), Z1 on the chroma stream
 *                may run beside the second simulation, which reads ll_mem_len for its put-back of verbatim samples.
 *   R_META_PACK  wavelet_type, select1, select2, size_data1/2, size_book1/2, tree_end, status: the packetiser's (pack_words_par,
 *                pack_book_par, final_phase_par) and, under a debug stop, the dense Y31's (`c->m->select1 = sh_counts[0]`).
 * No other buffer needed a split: the exception list, the LL coder's bytes and its output are each written by the luma and the chroma side,
 * but every plan orders those writers through EE_LUMA_LIST; B_JPEG and B_PROC are read by Y5 beside the first simulation, which writes only
 * B_JPEG -- Y5 does not touch that plane at all. */
enum EncRes {
	R_META_EXW = B_META, R_META_POS = B_COUNT, R_META_LL, R_META_CH, R_META_PACK,
	R_BGR, R_OUT, R_SIZES, R_STATUS,                               /* the caller's pictures, files, sizes and status */
	R_COUNT
};
typedef std::bitset<R_COUNT> EncSet;
inline EncSet enc_set(std::initializer_list<int> l) { EncSet s; for (int r : l) s.set((size_t)r); return s; }
struct EncAccess { EncSet reads, writes; };

/* what kernel step (op, a, b) of a plan at quality q reads and writes; nothing for the event operations, the stamps and the boundaries */
inline EncAccess enc_access(int op, int a, int b, int q, bool compat, bool dbg)
{
	/* a chroma step's planes: work plane, coefficient plane, copy of LL1, copy of the level-2 block, the 4:2:0 bytes */
	const bool own = a == 2;
	const int cj = own ? B_CJPEG_V : B_CJPEG, cp = own ? B_CPROC_V : B_CPROC, cl = own ? B_CLL1_V : B_CLL1, cs = own ? B_CL2SAVE_V : B_CL2SAVE, by = a ? B_PV : B_PU;
	const EncSet staged = enc_set({ cj, cp, cl });                  /* the seven staged kernels of a debug stop: pointwise passes and filterbank calls on the component's planes */
	EncAccess r;
	switch (op) {
	case ENC_COLOR:          /* k_color: bgr -> y, u, v as handed over */
		return { enc_set({ R_BGR }), enc_set({ a ? B_KMAP : B_JPEG, B_PU, B_PV }) };
	case ENC_LOW_PREFILTER:  /* src = jpeg; y = B_KMAP, km = proc, so = B_SCAN, chain = B_KEEP, tab = B_LOWTAB: k_low_pre .. k_low_marks read and write all five */
		r.writes = enc_set({ B_KMAP, B_PROC, B_SCAN, B_KEEP, B_LOWTAB });
		r.reads = r.writes | enc_set({ B_JPEG });
		return r;
	case ENC_LOW_STALE:      /* k_low_stale: km = proc -> B_STALE */
		return { enc_set({ B_PROC }), enc_set({ B_STALE }) };
	case ENC_FRONT:          /* FP_ARGS / FI_ARGS of nhw_launch_front_fused: k_front_plain takes no row state; keep only for q >= 22 */
		if (q <= 16) return { enc_set({ B_KMAP }), enc_set({ B_PROC, B_JPEG, B_LL1 }) };
		if (q <= 21) return { enc_set({ R_BGR }), enc_set({ B_PU, B_PV, B_ROWSTATE, B_PROC, B_JPEG, B_LL1 }) };
		return { enc_set({ R_BGR }), enc_set({ B_PU, B_PV, B_PROC, B_JPEG, B_LL1, B_KEEP }) };
	case ENC_FRONT_STALE:    /* k_front_stale: y = B_KMAP, st = B_ROWSTATE -> B_STALE */
		return { enc_set({ B_KMAP, B_ROWSTATE }), enc_set({ B_STALE }) };
	case ENC_C_PREFILTER:    /* k_low_prefilter_chroma(src = bytes, dst = cjpeg) */
	case ENC_C_WIDEN:        /* chroma_p0_par: `c->pv` / `c->pu` -> `c->cjpeg` */
		return { enc_set({ by }), enc_set({ cj }) };
	case ENC_C_ANALYSIS1:    /* k_dwt_ana<256>: from src8 (b) or the work plane; jpeg, proc, save = cll1 */
		return { enc_set({ b ? by : cj }), enc_set({ cj, cp, cl }) };
	case ENC_C_THIN:         /* k_low_chroma_thin(plane = cproc) */
		return { enc_set({ cp }), enc_set({ cp }) };
	case ENC_C_LOOPS:        /* k_chroma_loops: `side = p[...]`, `ll1_row`, `behind = compat ? pu[32768] ...` (U's byte plane for either component); stores `o[Q >> 2]`, `save`, `p` */
		r.reads = enc_set({ cp, cl });
		if (compat) r.reads.set(B_PU);
		r.writes = enc_set({ cp, cl, cs });
		return r;
	case ENC_C_ANALYSIS2:
		return { staged, b ? staged | enc_set({ cs }) : staged };
	case ENC_C_SIM1:         /* + chroma_ll1_neighbour: `c->pu` (compat), `c->cll1[Q >> 2]` */
		r.reads = staged; r.writes = staged;
		if (compat) r.reads.set(B_PU);
		return r;
	case ENC_C_SYN: case ENC_C_PRECOMP: case ENC_C_SIM2:
		return { staged, staged };
	case ENC_C_TAIL:         /* chroma_tail_once_par / chroma_p5_par: cproc, cll1, cl2save; chroma_ll2_emit_par appends to c->exw, writes c->ll_bytes and res_u64 / res_v64; cq_flush parks U in c->ubytes, V merges it into cnzq (+ cfbase) / cvals; `dense` (debug stop): c->scan + 4 Q */
		r.reads = enc_set({ cp, cl, cs, B_EXW, R_META_EXW, B_UBYTES, B_LLBYTES });
		r.writes = enc_set({ B_EXW, R_META_EXW, B_LLBYTES, a ? B_RESV64 : B_RESU64, B_UBYTES, B_CNZQ, B_CVALS });
		if (!b || dbg) r.writes.set((size_t)cp);
		if (dbg) r.writes.set(B_SCAN);
		return r;
	case ENC_Y4:             /* k_dwt_ana<256> with alt = ll1 */
		return { enc_set({ B_LL1 }), enc_set({ B_PROC, B_JPEG }) };
	case ENC_Y5:             /* luma_p1_par: `c->ll1[Q + k] = 0` (compat), tag_l2_details_par: proc read, ll1 read and written */
		return { enc_set({ B_PROC, B_LL1 }), enc_set({ B_LL1 }) };
	case ENC_DQ1:            /* wave_dequant_sim_luma(part 1): src = c->proc; `jp[at] = ...`; `if (keep_p || !part) p[at] = ...`, keep_p = the debug stop */
		r.reads = enc_set({ B_PROC }); r.writes = enc_set({ B_JPEG });
		if (dbg) r.writes.set(B_PROC);
		return r;
	case ENC_L_SYN1:
		return { enc_set({ B_JPEG, B_PROC }), enc_set({ B_JPEG, B_PROC }) };
	case ENC_Y8:             /* apply_tags_par, precompensate_ll1_par: proc, ll1, jpeg */
		return { enc_set({ B_JPEG, B_PROC, B_LL1 }), enc_set({ B_JPEG, B_PROC, B_LL1 }) };
	case ENC_L2_RECON:       /* k_l2_recon: reads the block of jpeg, `side = p[...]`, the LL1 rows; stores LL1 rows without their tags, `jp` (not LEAN), `p` and `save` (ANA) */
		r.reads = enc_set({ B_JPEG, B_PROC, B_LL1 });
		r.writes = enc_set({ B_LL1 });
		if (!b) r.writes.set(B_JPEG);
		if (a) { r.writes.set(B_PROC); r.writes.set(B_L2SAVE); }
		return r;
	case ENC_L_ANALYSIS2:
		r.reads = enc_set({ B_JPEG, B_PROC }); r.writes = r.reads;
		if (a) r.writes.set(B_L2SAVE);
		return r;
	case ENC_LOW_LL2:        /* k_low_ll2(proc) */
		return { enc_set({ B_PROC }), enc_set({ B_PROC }) };
	case ENC_COPY_BLOCK:     /* proc -> l2save */
		return { enc_set({ B_PROC }), enc_set({ B_L2SAVE }) };
	case ENC_EMIT:           /* wave_emit_ll2: ll2_load_row(p ...); stores p, jp, c->exw, c->ll_bytes, c->ll_full, c->res4, res4_len, exw_len */
		return { enc_set({ B_PROC }), enc_set({ B_PROC, B_JPEG, B_EXW, B_LLBYTES, B_LLFULL, B_RES4, R_META_EXW }) };
	case ENC_LL_CODER:       /* luma_p3_par: clears c->ll_bytes behind the luma samples, ll_code_luma_par: ll_bytes, ll_full -> ll_comp, ll_word, ll_mem, the four scalars.
		                      * compat: reads c->stale, c->l2save, writes the cells behind ll1 and (q <= 13) behind l2save.  Y17 (q <= 12, a debug stop): l2save -> proc */
		r.reads = enc_set({ B_LLBYTES, B_LLFULL });
		r.writes = enc_set({ B_LLBYTES, B_LLFULL, B_LLCOMP, B_LLWORD, B_LLMEM, R_META_LL });
		if (compat) { r.reads |= enc_set({ B_STALE, B_L2SAVE }); r.writes |= enc_set({ B_LL1, B_L2SAVE }); }
		if (q <= 12 || dbg) { r.reads.set(B_L2SAVE); r.writes.set(B_PROC); }
		return r;
	case ENC_DQ0:            /* wave_dequant_sim_luma(part 0): src = l2save (a debug stop: proc); wave_ll2 / wave_dequant_details / wave_shrink store p and jp; `hand` = B_KMAP;
		                      * wave_ll2_verbatim, unless deferred: `c->m->ll_mem_len`, `c->ll_mem[i]` */
		r.reads = enc_set({ B_L2SAVE, B_PROC, B_JPEG });
		r.writes = enc_set({ B_PROC, B_JPEG });
		if (a & 2) r.writes.set(B_KMAP);
		if (!b) r.reads |= enc_set({ B_LLMEM, R_META_LL });
		return r;
	case ENC_L_SYN2:         /* k_dwt_syn<256>(jpeg, proc); verb_list = B_LLMEM, verb_len = ll_mem_len */
		r.reads = enc_set({ B_JPEG, B_PROC }); r.writes = r.reads;
		if (b) r.reads |= enc_set({ B_LLMEM, R_META_LL });
		return r;
	case ENC_L4A:            /* luma_p4a_par: Y19 jpeg -> first_order; Y20 proc; Y21 .. Y23 (tag_small_runs_par, residuals_fused_par): proc, l2save, the code plane ll1 */
		return { enc_set({ B_JPEG, B_PROC, B_L2SAVE, B_LL1, B_FIRST }), enc_set({ B_PROC, B_LL1, B_FIRST }) };
	case ENC_L4B:            /* luma_p4b_par: adjust_first_order_par (q > 21), build_poslists_par: ll1, first_order -> raw, pay, hs; poslist_finish_par: `P = c->cc`, `F = c->half`, the lists and their lengths */
		r.reads = enc_set({ B_LL1, B_FIRST });
		r.writes = enc_set({ B_FIRST, B_RAW, B_PAY, B_HS, B_CC, B_HALF, B_R1LIST, B_R1BITS, B_R1WORD, B_R3LIST, B_R3BITS, B_R3WORD, B_R5LIST, B_R5BITS, B_R5WORD, R_META_POS });
		return r;
	case ENC_L4C:            /* luma_p4c_par: Y26 l2save -> proc, clean_details_seq: proc, l2save */
		return { enc_set({ B_L2SAVE, B_PROC }), enc_set({ B_PROC }) };
	case ENC_QUANT:          /* wave_quantise_luma: proc, llsrc = l2save, hand = B_KMAP -> nzq (+ fbase), vals; write_plane (q > 21, a debug stop): proc; dense (a debug stop): c->scan */
		r.reads = enc_set({ B_PROC, B_L2SAVE });
		if (a) r.reads.set(B_KMAP);
		r.writes = enc_set({ B_NZQ, B_VALS });
		if (q > 21 || dbg) r.writes.set(B_PROC);
		if (dbg) r.writes.set(B_SCAN);
		return r;
	case ENC_L4C2:           /* luma_p4c2_par: proc, first_order, keep -> band, hs, raw, pay, qsetting3, char_res1, res6, cc, half, the three lengths */
		r.reads = enc_set({ B_PROC, B_FIRST, B_KEEP });
		r.writes = enc_set({ B_BAND, B_HS, B_RAW, B_PAY, B_QSET3, B_CHARRES, B_R6LIST, B_R6BITS, B_R6WORD, B_CC, B_HALF, R_META_POS });
		r.reads |= r.writes;
		return r;
	case ENC_Y31:            /* scan_rewrite_list_par: nzq, fbase -> nzs, voff; rewrites c->vals; `sel = c->half`.  A debug stop (luma_p4d_par, dense): + proc, c->scan, select1 / select2 */
		r.reads = enc_set({ B_NZQ, B_VALS });
		r.writes = enc_set({ B_NZS, B_VOFF, B_VALS, B_HALF });
		if (dbg) { r.reads |= enc_set({ B_PROC, B_SCAN }); r.writes |= enc_set({ B_SCAN, R_META_PACK }); }
		return r;
	case ENC_PACK_CHROMA:    /* pack_chroma_par points nzs, voff, raw and packet at B_CPACK / B_CPACKET; pack_words_par<1> reads cnzq, cfbase, cvals and writes neither s1 / s2 nor a scalar of NhwMeta */
		return { enc_set({ B_CNZQ, B_CVALS }), enc_set({ B_CPACK, B_CPACKET }) };
	case ENC_LLC:            /* ll_code_chroma_par: ll_bytes, ll_comp_y_len, res_low -> ll_comp behind the luma part, res_high, ch_res_len */
		return { enc_set({ B_LLBYTES, B_LLCOMP, R_META_LL }), enc_set({ B_LLCOMP, R_META_CH }) };
	case ENC_FINAL:          /* final_phase_par: pack_words_par<0>, both books, container_par */
		r.reads = enc_set({ B_NZS, B_VOFF, B_VALS, B_CPACK, B_CPACKET, B_CNZQ, B_EXW, B_RES4, B_CHARRES, B_QSET3, B_RESU64, B_RESV64, B_LLWORD, B_LLCOMP,
		                    B_R1LIST, B_R1BITS, B_R1WORD, B_R3LIST, B_R3BITS, B_R3WORD, B_R5LIST, B_R5BITS, B_R5WORD, B_R6LIST, B_R6BITS, B_R6WORD,
		                    R_META_EXW, R_META_POS, R_META_LL, R_META_CH, R_META_PACK });
		r.writes = enc_set({ B_PACKET, B_S1, B_S2, B_SEL1, B_SEL2, B_BOOK1, B_BOOK2, B_CC, B_RAW, R_META_PACK, R_OUT, R_SIZES, R_STATUS });
		if (!a) { r.reads |= enc_set({ B_CNZQ, B_CVALS }); r.writes |= enc_set({ B_CPACK, B_CPACKET }); }
		r.reads |= r.writes & ~enc_set({ R_OUT, R_SIZES, R_STATUS });
		return r;
	default:
		return r;
	}
}

#endif
