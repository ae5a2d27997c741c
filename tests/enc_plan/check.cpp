/* The encoder's batch plans (nhwcodec_amd/csrc/nhw_enc_plan.h) held against the header's own resource table and against the sequences the
 * batch driver issued before it had a planner, on the CPU (tests/test_enc_plan.py builds and runs this, plain and under the sanitizers).
 * Over the whole domain -- 23 qualities x compat 0, 1 x the four (what, timed) pairs of the driver x small and large n x low_parts 1, 2 x every
 * combination of the ten other switches at stop 0; stops 1 .. STOPS x 23 qualities x compat 0, 1 x 13 switch settings:
 *   a. order: in the happens-before relation of a plan (program order on each stream, record -> wait) every two kernel steps of which one
 *      writes what the other reads or writes are ordered;
 *   b. events: every wait names an event recorded earlier in the plan (but EE_PART_FRONT of a `what = 2` plan, the sub-batch loop's); no event
 *      is recorded twice without a wait between; every step of a side stream happens before the plan's last step: a batch ends joined;
 *   c. shape: the stamps, what a `what = 1` / `what = 2` / stopped plan holds, the values the plan carries, the stage count;
 *   d. what a switch must not change;
 *   e. the pin: the literal sequences below, transcribed from the driver as it was.
 * Prints "plans <n> pinned <m> mismatches <k>"; k = 0 is success. */
#include <stdio.h>
#include <string.h>

#include <unordered_map>
#include <string>
#include <vector>

#include "../../nhwcodec_amd/csrc/nhw_enc_plan.h"

enum { STOPS = 48 };                                              /* more than the stage boundaries of any plan (37): the last stops run to the end */

static int mismatches = 0;
static void fail(const std::string &where, const std::string &what)
{
	mismatches++;
	if (mismatches <= 200) printf("%s: %s\n", where.c_str(), what.c_str());
}

typedef std::vector<EncStep> Steps;
static const char *const op_name[ENC_OP_COUNT] = { "stamp", "record", "wait", "stage", "color", "low-prefilter", "low-stale", "front", "front-stale",
	"c-prefilter", "c-widen", "c-analysis1", "c-thin", "c-loops", "c-analysis2", "c-sim1", "c-syn", "c-precomp", "c-sim2", "c-tail",
	"y4", "y5", "dq1", "l-syn1", "y8", "l2-recon", "l-analysis2", "low-ll2", "copy-block", "emit", "ll-coder", "dq0", "l-syn2", "l4a", "l4b", "l4c",
	"quant", "l4c2", "y31", "pack-chroma", "llc", "final" };
static const char *const stream_name[ES_COUNT] = { "", "@chroma", "@lists", "@ll" };
static std::string show(const EncStep &s) { return std::string(op_name[s.op]) + stream_name[s.stream] + "(" + std::to_string(s.a) + "," + std::to_string(s.b) + ")"; }
static std::string show(const Steps &v) { std::string r; for (const EncStep &s : v) r += show(s) + " "; return r; }
static bool same(const Steps &a, const Steps &b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(EncStep))); }
static Steps steps_of(const EncPlan &p) { return Steps(p.step, p.step + p.n); }

static EncIn defaults(int q)
{
	EncIn in = {};
	in.q = q; in.what = 3; in.timed = 1; in.big = 1;
	in.low_chroma = 2; in.chroma_fork = in.lists_fork = in.ll_fork = in.quant_join = in.y5_fork = in.ll2_once = in.quant_marks = in.chroma_tail_once = 1;
	in.pack_fork = 2; in.low_parts = 2;
	return in;
}
static std::string where_of(const EncIn &i)
{
	char b[256];
	snprintf(b, sizeof b, "q %d stop %d compat %d what %d timed %d big %d fb %d | low_chroma %d chroma_fork %d lists %d ll %d join %d y5 %d ll2 %d marks %d once %d pack %d low_parts %d",
	         i.q, i.stop, i.compat, i.what, i.timed, i.big, i.front_fallback, i.low_chroma, i.chroma_fork, i.lists_fork, i.ll_fork, i.quant_join, i.y5_fork, i.ll2_once, i.quant_marks,
	         i.chroma_tail_once, i.pack_fork, i.low_parts);
	return b;
}

/* ------------------------------------------------------------------------------------------------ a. order, b. events */
typedef std::bitset<ENC_PLAN_CAP> Row;
/* reach[i]: the steps that happen after step i.  Every edge runs forward in enqueue order, so one pass from the back closes the relation.
 * The record of EE_LOW_PASS_A lies inside its step, behind nothing of it: its edge starts at the step in front of the pre-filter. */
static std::vector<Row> happens_before(const Steps &v)
{
	const int n = (int)v.size();
	std::vector<std::vector<int>> succ((size_t)n);
	for (int i = 0; i < n; i++) {
		for (int j = i + 1; j < n; j++) if (v[j].stream == v[i].stream) { succ[(size_t)i].push_back(j); break; }
		if (v[i].op != ENC_WAIT) continue;
		for (int r = i - 1; r >= 0; r--) {
			const bool rec = (v[r].op == ENC_RECORD || v[r].op == ENC_STAMP) && v[r].a == v[i].a;
			const bool in_step = v[r].op == ENC_LOW_PREFILTER && v[r].a > 1 && v[i].a == EE_LOW_PASS_A;
			if (!rec && !in_step) continue;
			if (rec) succ[(size_t)r].push_back(i);
			else for (int f = r - 1; f >= 0; f--) if (v[f].stream == v[r].stream) { succ[(size_t)f].push_back(i); break; }
			break;
		}
	}
	std::vector<Row> reach((size_t)n);
	for (int i = n - 1; i >= 0; i--) for (int j : succ[(size_t)i]) { reach[(size_t)i] |= reach[(size_t)j]; reach[(size_t)i].set((size_t)j); }
	return reach;
}
/* the conflicts of `v` that its happens-before relation leaves unordered */
static int unordered_conflicts(const Steps &v, int q, bool compat, bool dbg, const std::string &where, bool report, std::string *pairs = nullptr)
{
	const int n = (int)v.size();
	const std::vector<Row> reach = happens_before(v);
	std::vector<EncAccess> acc((size_t)n);
	for (int i = 0; i < n; i++) acc[(size_t)i] = enc_access(v[i].op, v[i].a, v[i].b, q, compat, dbg);
	int found = 0;
	for (int i = 0; i < n; i++) {
		if (!enc_is_kernel(v[i].op)) continue;
		for (int j = i + 1; j < n; j++) {
			if (!enc_is_kernel(v[j].op) || reach[(size_t)i].test((size_t)j)) continue;
			const EncAccess &a = acc[(size_t)i], &b = acc[(size_t)j];
			const EncSet clash = (a.writes & (b.reads | b.writes)) | (b.writes & a.reads);
			if (clash.none()) continue;
			found++;
			std::string res;
			for (int r = 0; r < R_COUNT; r++) if (clash.test((size_t)r)) res += " " + std::to_string(r);
			if (pairs) *pairs += show(v[i]) + "/" + show(v[j]) + ":" + res + ";";
			if (report) fail(where, "steps " + std::to_string(i) + " " + show(v[i]) + " and " + std::to_string(j) + " " + show(v[j]) + " are not ordered and share resources" + res);
		}
	}
	return found;
}
static void check_events(const Steps &v, const EncIn &in, const std::string &where)
{
	const int n = (int)v.size();
	int state[EE_COUNT] = {};                                     /* 0: not recorded, 1: recorded and not yet waited for, 2: recorded and waited for */
	for (int i = 0; i < n; i++) {
		const EncStep &s = v[i];
		int rec = -1;
		if (s.op == ENC_RECORD || s.op == ENC_STAMP) rec = s.a;
		if (s.op == ENC_LOW_PREFILTER && s.a > 1) rec = EE_LOW_PASS_A;
		if (rec >= EE_COUNT) { fail(where, show(s) + " names no event"); continue; }
		if (rec >= 0) {
			if (rec == EE_PART_FRONT) fail(where, "the plan records the sub-batch loop's event");
			if (state[rec] == 1 && s.op != ENC_STAMP) fail(where, show(s) + " records an event a second time with no wait between");
			if (s.op == ENC_STAMP && state[rec]) fail(where, show(s) + " stamps twice");
			state[rec] = 1;
		}
		if (s.op == ENC_WAIT) {
			if (s.a >= EE_COUNT) { fail(where, show(s) + " names no event"); continue; }
			if (s.a == EE_PART_FRONT) { if (in.what != 2 || i != 0) fail(where, "the wait for the front group's event is not the first step of a what = 2 plan"); continue; }
			if (!state[s.a]) fail(where, show(s) + " waits for an event that no earlier step records");
			else state[s.a] = 2;
		}
	}
	for (int ev = EE_LUMA_LIST; ev < EE_PART_FRONT; ev++) if (state[ev] == 1 && ev != EE_LOW_PASS_A) fail(where, "event " + std::to_string(ev) + " is recorded and never waited for");
	/* ends joined: behind the last step of the caller's stream lies everything a side stream was given */
	int last = n - 1;
	while (last >= 0 && v[(size_t)last].stream != ES_MAIN) last--;
	if (last != n - 1) fail(where, "the plan does not end on the caller's stream");
	const std::vector<Row> reach = happens_before(v);
	for (int i = 0; i < n; i++) if (v[i].stream != ES_MAIN && i != last && !reach[(size_t)i].test((size_t)last)) fail(where, show(v[i]) + " on a side stream is not joined before the plan ends");
}

/* ------------------------------------------------------------------------------------------------ c. shape */
static int stage_count(const Steps &v) { int k = 0; for (const EncStep &s : v) k += s.op == ENC_STAGE; return k; }
static bool front_step(int op) { return op >= ENC_COLOR && op <= ENC_FRONT_STALE; }
static void check_shape(const EncPlan &p, const EncIn &in, const std::string &where)
{
	const Steps v = steps_of(p);
	static const int order[7] = { EE_START, EE_COLOR, EE_PREFILTER, EE_FRONT, EE_LUMA, EE_CHROMA, EE_END };   /* nhw_timing order */
	int at = -1;
	bool seen[7] = {};
	bool side = false, marks = false, once = false, lean = false, front = false, behind = false;
	for (const EncStep &s : v) {
		if (s.op >= ENC_OP_COUNT || s.stream >= ES_COUNT) { fail(where, "a step that is none"); continue; }
		if (s.stream != ES_MAIN) side = true;
		if (s.op == ENC_STAMP) {
			int k = 0;
			while (k < 7 && order[k] != s.a) k++;
			if (k == 7 || s.stream != ES_MAIN) { fail(where, show(s) + " is no stamp of nhw_timing on the caller's stream"); continue; }
			if (k <= at) fail(where, show(s) + " out of nhw_timing order");
			at = k; seen[k] = true;
		}
		if ((s.op == ENC_DQ0 && (s.a & 2)) || (s.op == ENC_QUANT && s.a)) marks = true;
		if (s.op == ENC_C_TAIL && s.b) once = true;
		if ((s.op == ENC_Y4 && s.a) || (s.op == ENC_L2_RECON && s.b)) lean = true;
		if (front_step(s.op)) front = true; else if (enc_is_kernel(s.op)) behind = true;
		if (s.op == ENC_LOW_PREFILTER && s.a != p.low_parts_used) fail(where, "low_parts_used is not the pre-filter's");
		if (s.op == ENC_DQ0 && s.b != p.defer_verbatim) fail(where, "defer_verbatim is not the second simulation's");
		if (s.op >= ENC_C_PREFILTER && s.op <= ENC_C_TAIL && (s.a > 2 || (s.a == 2) != (p.split_chroma != 0 && s.a != 0))) fail(where, show(s) + ": plane set against split_chroma");
	}
	/* the stamps: EV_COLOR and EV_PREFILTER belong to the front group whoever brackets it (the sub-batch loop stamps EV_START and EV_FRONT around a
	 * `what = 1` plan itself); the five stage stamps follow `timed` */
	const bool complete = !in.stop;
	if (in.timed == 1) { if (v.empty() || v[0].op != ENC_STAMP || v[0].a != EE_START) fail(where, "EV_START is not first"); if (complete && (v.back().op != ENC_STAMP || v.back().a != EE_END)) fail(where, "EV_END is not last"); }
	else if (seen[0] || seen[3] || seen[6]) fail(where, "EV_START, EV_FRONT or EV_END without timed = 1");
	if (in.timed == 0 && (seen[4] || seen[5])) fail(where, "a stage stamp with timed = 0");
	if (in.timed == 2 && !(seen[4] && seen[5])) fail(where, "timed = 2 without EV_LUMA and EV_CHROMA");
	if ((seen[1] || seen[2]) && !(in.what & 1)) fail(where, "the front group's stamps without the front group");
	if (complete && (in.what & 1) && !(seen[1] && seen[2])) fail(where, "the front group without its stamps");
	if (in.what == 1 && (behind || !front || v.back().op != ENC_STAGE)) fail(where, "a what = 1 plan does not end behind the front group");
	if (in.what == 2 && front) fail(where, "a what = 2 plan holds a front step");
	if (in.stop) {
		if (side) fail(where, "a stopped plan uses a side stream");
		if (!p.dbg || marks || once || lean || p.split_chroma || p.defer_verbatim || p.timed) fail(where, "a stopped plan with marks, once, lean, a fork's value, or without dbg");
		const int k = stage_count(v);
		if (k > in.stop || (k < in.stop && (v.empty() || v.back().op != ENC_STAMP)) || (k == in.stop && v.back().op != ENC_STAGE)) fail(where, "a stop at k does not end behind the k-th boundary");
	} else if (p.dbg) fail(where, "dbg without a stop");
	if (p.timed != (in.what == 3 && !in.stop)) fail(where, "`timed` is not `a whole batch without a stop`");
	if (p.low_parts_used < 1 || (p.low_parts_used > 1 && !(in.q <= 16 && in.big && in.what == 3 && !in.stop))) fail(where, "low_parts_used");
}

/* ------------------------------------------------------------------------------------------------ e. the pin
 * The sequences of run_batch, chroma_head_launches and luma_loop_launches as they stood before the planner, read off their text: (operation,
 * stream, a, b) in the order enqueued.  The pieces that recur are named once; each pin is written out of them by hand, not by a rule.
 * ONE OF THEM IS NOT WHAT THE DRIVER ISSUED: with NHW_QUANT_JOIN=0 and the lists' fork on (quality 13 .. 20) it waited for the lists' event behind
 * Y31 -- "... y31 stage stamp(luma) wait(lists) wait(chroma) ..." -- so that Y24 / Y25 on the lists' stream ran beside Y31, and both use B_HALF as
 * scratch, which check (a) reports (old_late_join below keeps that sequence to show it).  The wait now stands in front of Y31. */
#define K(OP, S, A, B) EncStep{ ENC_##OP, ES_##S, A, B }
#define ST K(STAGE, MAIN, 0, 0)
#define T(E) K(STAMP, MAIN, EE_##E, 0)
#define REC(E, S) K(RECORD, S, EE_##E, 0)
#define WAIT(E, S) K(WAIT, S, EE_##E, 0)
static Steps cat(std::initializer_list<Steps> l) { Steps r; for (const Steps &s : l) r.insert(r.end(), s.begin(), s.end()); return r; }

/* the front group, timed == 1 */
static Steps front_low(int lparts, bool compat) { Steps r = { T(START), K(COLOR, MAIN, 0, 0), T(COLOR), ST, K(LOW_PREFILTER, MAIN, (uint8_t)lparts, 0), T(PREFILTER), ST }; if (compat) r.push_back(K(LOW_STALE, MAIN, 0, 0)); return cat({ r, { K(FRONT, MAIN, 0, 0), ST, ST, T(FRONT) } }); }
static const Steps front_17 = { T(START), T(COLOR), T(PREFILTER), ST, ST, K(FRONT, MAIN, 0, 0), ST, ST, T(FRONT) };
static const Steps front_17_compat = { T(START), T(COLOR), T(PREFILTER), ST, ST, K(FRONT, MAIN, 0, 0), K(COLOR, MAIN, 1, 0), K(FRONT_STALE, MAIN, 0, 0), ST, ST, T(FRONT) };
static const Steps front_22 = { T(START), T(COLOR), T(PREFILTER), ST, K(FRONT, MAIN, 0, 0), ST, ST, T(FRONT) };
/* a chroma head of a production batch on stream S, plane set A: quality <= 14, 15 / 16, 17 .. */
#define HEAD_14(S, A) Steps{ K(C_PREFILTER, S, A, 0), ST, K(C_ANALYSIS1, S, A, 0), K(C_THIN, S, A, 0), ST, ST, K(C_LOOPS, S, A, 0) }
#define HEAD_16(S, A) Steps{ ST, K(C_ANALYSIS1, S, A, 1), K(C_THIN, S, A, 0), ST, ST, K(C_LOOPS, S, A, 0) }
#define HEAD_17(S, A) Steps{ ST, K(C_ANALYSIS1, S, A, 1), ST, ST, K(C_LOOPS, S, A, 0) }
/* ... and under a debug stop (the caller's stream): the seven staged kernels */
#define HEAD_DBG_LOOPS(A) K(C_ANALYSIS2, MAIN, A, 0), ST, K(C_SIM1, MAIN, A, 0), ST, K(C_SYN, MAIN, A, 0), ST, K(C_PRECOMP, MAIN, A, 0), ST, K(C_ANALYSIS2, MAIN, A, 1), ST, ST, K(C_SIM2, MAIN, A, 0), ST, K(C_SYN, MAIN, A, 0), ST
#define HEAD_DBG_14(A) Steps{ K(C_PREFILTER, MAIN, A, 0), ST, K(C_ANALYSIS1, MAIN, A, 0), K(C_THIN, MAIN, A, 0), ST, ST, HEAD_DBG_LOOPS(A) }
#define HEAD_DBG_17(A) Steps{ K(C_WIDEN, MAIN, A, 0), ST, K(C_ANALYSIS1, MAIN, A, 0), ST, ST, HEAD_DBG_LOOPS(A) }
/* the luma loop with Y5 beside the first simulation (LEAN: 1 outside the compatibility mode), and in line */
#define Y5_BESIDE REC(Y5_FORK, MAIN), WAIT(Y5_FORK, LL), K(Y5, LL, 0, 0), REC(Y5_DONE, LL), K(DQ1, MAIN, 0, 0), WAIT(Y5_DONE, MAIN), ST
#define Y5_INLINE K(Y5, MAIN, 0, 0), K(DQ1, MAIN, 0, 0), ST
static const Steps loop_6 = { K(Y4, MAIN, 0, 0), ST };
#define LOOP_12(LEAN, Y5) Steps{ K(Y4, MAIN, LEAN, 0), ST, Y5, K(L2_RECON, MAIN, 0, 0), K(L_ANALYSIS2, MAIN, 0, 0), ST }
#define LOOP_13(LEAN, Y5) Steps{ K(Y4, MAIN, LEAN, 0), ST, Y5, K(L2_RECON, MAIN, 1, LEAN), ST }
#define LOOP_DBG(SAVE) Steps{ K(Y4, MAIN, 0, 0), ST, Y5_INLINE, K(L_SYN1, MAIN, 0, 0), ST, K(Y8, MAIN, 0, 0), ST, K(L_ANALYSIS2, MAIN, SAVE, 0), ST }
static const Steps low_ll2 = { K(LOW_LL2, MAIN, 0, 0), K(COPY_BLOCK, MAIN, 0, 0), ST };
/* the LL2 coder beside the second simulation; in line with the fork's record; in line */
#define CODER_BESIDE REC(LL_FORK, MAIN), WAIT(LL_FORK, LL), K(LL_CODER, LL, 0, 0), REC(LL_DONE, LL), REC(LUMA_LIST, LL)
#define CODER_FORK K(LL_CODER, MAIN, 0, 0), REC(LUMA_LIST, MAIN)
#define LISTS_BESIDE REC(LISTS_FORK, MAIN), WAIT(LISTS_FORK, LISTS), K(L4B, LISTS, 0, 0), REC(LISTS, LISTS)
/* the rest of the chroma stream: both tails, the packetiser's chroma part (pack_fork 2, 1, 0), Z1 */
#define TAILS(ONCE) WAIT(LUMA_LIST, CHROMA), K(C_TAIL, CHROMA, 0, ONCE), ST, K(C_TAIL, CHROMA, 2, ONCE), ST
static const Steps rest_2 = { TAILS(1), REC(PACK_FORK, CHROMA), WAIT(PACK_FORK, LL), K(PACK_CHROMA, LL, 0, 0), REC(PACK_DONE, LL), K(LLC, CHROMA, 0, 0), WAIT(PACK_DONE, CHROMA), REC(CHROMA_DONE, CHROMA) };
static const Steps rest_2_staged = { TAILS(0), REC(PACK_FORK, CHROMA), WAIT(PACK_FORK, LL), K(PACK_CHROMA, LL, 0, 0), REC(PACK_DONE, LL), K(LLC, CHROMA, 0, 0), WAIT(PACK_DONE, CHROMA), REC(CHROMA_DONE, CHROMA) };
static const Steps rest_1 = { TAILS(1), K(LLC, CHROMA, 0, 0), K(PACK_CHROMA, CHROMA, 0, 0), REC(CHROMA_DONE, CHROMA) };
static const Steps rest_0 = { TAILS(1), K(LLC, CHROMA, 0, 0), REC(CHROMA_DONE, CHROMA) };
static const Steps end_fork = { K(Y31, MAIN, 0, 0), ST, T(LUMA), T(CHROMA), K(FINAL, MAIN, 1, 0), T(END) };
/* the in-line order's chroma sequence behind the luma tail */
#define INLINE_CHROMA(HEAD, ONCE) HEAD(MAIN, 0), Steps{ K(C_TAIL, MAIN, 0, ONCE), ST }, HEAD(MAIN, 1), Steps{ K(C_TAIL, MAIN, 1, ONCE), ST }
static const Steps end_inline = { T(CHROMA), K(LLC, MAIN, 0, 0), K(FINAL, MAIN, 0, 0), T(END) };

/* the default forked order at quality 20, piece by piece; the single-switch pins below replace one piece */
static const Steps q20_heads = cat({ { WAIT(FRONT, CHROMA) }, HEAD_17(CHROMA, 0), HEAD_17(CHROMA, 2) });
static const Steps q20_second = { K(EMIT, MAIN, 1, 0), CODER_BESIDE, K(DQ0, MAIN, 3, 1), ST, WAIT(LL_DONE, MAIN), K(L_SYN2, MAIN, 1, 1), ST };
static const Steps q20_resid = { K(L4A, MAIN, 0, 0), LISTS_BESIDE, K(L4C, MAIN, 0, 0) };
static const Steps q20_join = { WAIT(LISTS, MAIN), WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 1, 0) };
static Steps q20_default() { return cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, q20_resid, rest_2, q20_join, end_fork }); }
static Steps q20_inline_tail(int marks)
{
	return cat({ LOOP_13(1, Y5_INLINE), { ST, K(EMIT, MAIN, 0, 0), K(LL_CODER, MAIN, 0, 0), K(DQ0, MAIN, (uint8_t)(marks ? 2 : 0), 0), ST, K(L_SYN2, MAIN, 1, 0), ST, K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0),
	             K(QUANT, MAIN, (uint8_t)marks, 0), K(Y31, MAIN, 0, 0), ST } });
}

struct Pin { const char *name; EncIn in; Steps want; };
static EncIn with(EncIn in, int EncIn::*m, int v) { in.*m = v; return in; }
static EncIn inline_of(int q) { return with(defaults(q), &EncIn::chroma_fork, 0); }
static EncIn compat_of(int q) { return with(defaults(q), &EncIn::compat, 1); }
static EncIn low10(int low_chroma, int lparts) { return with(with(defaults(10), &EncIn::low_chroma, low_chroma), &EncIn::low_parts, lparts); }
static Steps q10_forked(int lparts, int ev)                          /* the forked order at quality 10; ev: what the chroma stream waits for */
{
	return cat({ front_low(lparts, false), { K(WAIT, CHROMA, (uint8_t)ev, 0) }, HEAD_14(CHROMA, 0), HEAD_14(CHROMA, 2), LOOP_12(1, Y5_BESIDE), low_ll2, { K(EMIT, MAIN, 0, 0), CODER_FORK, K(L4A, MAIN, 0, 0), K(L4C, MAIN, 0, 0) },
	             rest_2, { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork });
}
static std::vector<Pin> pins()
{
	std::vector<Pin> p;
	/* the default forked order (n >= 1024: the low pre-filter in two sub-batches) */
	p.push_back({ "default q6", defaults(6), cat({ front_low(2, false), { WAIT(LOW_PASS_A, CHROMA) }, HEAD_14(CHROMA, 0), HEAD_14(CHROMA, 2), loop_6, low_ll2, { K(EMIT, MAIN, 0, 0), CODER_FORK, K(L4A, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2,
	                                          { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "default q7", defaults(7), cat({ front_low(2, false), { WAIT(LOW_PASS_A, CHROMA) }, HEAD_14(CHROMA, 0), HEAD_14(CHROMA, 2), LOOP_12(1, Y5_BESIDE), low_ll2, { K(EMIT, MAIN, 0, 0), CODER_FORK, K(L4A, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2,
	                                          { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "default q12", defaults(12), q10_forked(2, EE_LOW_PASS_A) });
	p.push_back({ "default q13", defaults(13), cat({ front_low(2, false), { WAIT(LOW_PASS_A, CHROMA) }, HEAD_14(CHROMA, 0), HEAD_14(CHROMA, 2), LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_FORK, K(DQ0, MAIN, 1, 0), ST, K(L_SYN2, MAIN, 1, 0), ST },
	                                            q20_resid, rest_2, { WAIT(LISTS, MAIN), WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "default q14", defaults(14), cat({ front_low(2, false), { WAIT(LOW_PASS_A, CHROMA) }, HEAD_14(CHROMA, 0), HEAD_14(CHROMA, 2), LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_BESIDE, K(DQ0, MAIN, 1, 1), ST, WAIT(LL_DONE, MAIN), K(L_SYN2, MAIN, 1, 1), ST },
	                                            q20_resid, rest_2, { WAIT(LISTS, MAIN), WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "default q16", defaults(16), cat({ front_low(2, false), { WAIT(LOW_PASS_A, CHROMA) }, HEAD_16(CHROMA, 0), HEAD_16(CHROMA, 2), LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_BESIDE, K(DQ0, MAIN, 1, 1), ST, WAIT(LL_DONE, MAIN), K(L_SYN2, MAIN, 1, 1), ST },
	                                            q20_resid, rest_2, { WAIT(LISTS, MAIN), WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "default q17", defaults(17), q20_default() });
	p.push_back({ "default q20", defaults(20), q20_default() });
	p.push_back({ "default q21", defaults(21), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, { K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2, { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 1, 0) }, end_fork }) });
	for (int q = 22; q <= 23; q++)
		p.push_back({ q == 22 ? "default q22" : "default q23", defaults(q), cat({ front_22, q20_heads, LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_BESIDE, K(DQ0, MAIN, 3, 1), ST, WAIT(LL_DONE, MAIN), K(L_SYN2, MAIN, 0, 1), ST },
		              { K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2, { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 1, 0), K(L4C2, MAIN, 0, 0) }, end_fork }) });
	/* each switch off, one at a time, at quality 20 */
	p.push_back({ "q20 chroma_fork 0", inline_of(20), cat({ front_17, q20_inline_tail(1), { T(LUMA) }, INLINE_CHROMA(HEAD_17, 1), end_inline }) });
	p.push_back({ "q20 lists_fork 0", with(defaults(20), &EncIn::lists_fork, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, { K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2, { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 1, 0) }, end_fork }) });
	p.push_back({ "q20 ll_fork 0", with(defaults(20), &EncIn::ll_fork, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_FORK, K(DQ0, MAIN, 3, 0), ST, K(L_SYN2, MAIN, 1, 0), ST }, q20_resid, rest_2, q20_join, end_fork }) });
	/* quant_join 0: the join in front of the packetiser.  NOT the old driver's sequence: the wait for the lists stands in front of Y31 (B_HALF) */
	p.push_back({ "q20 quant_join 0", with(defaults(20), &EncIn::quant_join, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, q20_resid, { K(QUANT, MAIN, 1, 0) }, rest_2,
	                                                                                  { WAIT(LISTS, MAIN), K(Y31, MAIN, 0, 0), ST, T(LUMA), WAIT(CHROMA_DONE, MAIN), T(CHROMA), K(FINAL, MAIN, 1, 0), T(END) } }) });
	p.push_back({ "q20 y5_fork 0", with(defaults(20), &EncIn::y5_fork, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_INLINE), { ST }, q20_second, q20_resid, rest_2, q20_join, end_fork }) });
	p.push_back({ "q20 ll2_once 0", with(defaults(20), &EncIn::ll2_once, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 0, 0), CODER_BESIDE, K(DQ0, MAIN, 2, 1), ST, WAIT(LL_DONE, MAIN), K(L_SYN2, MAIN, 1, 1), ST }, q20_resid, rest_2, q20_join, end_fork }) });
	p.push_back({ "q20 quant_marks 0", with(defaults(20), &EncIn::quant_marks, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_BESIDE, K(DQ0, MAIN, 1, 1), ST, WAIT(LL_DONE, MAIN), K(L_SYN2, MAIN, 1, 1), ST }, q20_resid, rest_2,
	                                                                                    { WAIT(LISTS, MAIN), WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "q20 chroma_tail_once 0", with(defaults(20), &EncIn::chroma_tail_once, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, q20_resid, rest_2_staged, q20_join, end_fork }) });
	p.push_back({ "q20 pack_fork 1", with(defaults(20), &EncIn::pack_fork, 1), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, q20_resid, rest_1, q20_join, end_fork }) });
	p.push_back({ "q20 pack_fork 0", with(defaults(20), &EncIn::pack_fork, 0), cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, q20_resid, rest_0, q20_join, { K(Y31, MAIN, 0, 0), ST, T(LUMA), T(CHROMA), K(FINAL, MAIN, 0, 0), T(END) } }) });
	/* low_chroma 0, 1, 2 with the pre-filter in one and in two sub-batches, at quality 10 */
	p.push_back({ "q10 low_chroma 0 lparts 1", low10(0, 1), q10_forked(1, EE_FRONT) });
	p.push_back({ "q10 low_chroma 0 lparts 2", low10(0, 2), q10_forked(2, EE_FRONT) });
	p.push_back({ "q10 low_chroma 1 lparts 1", low10(1, 1), q10_forked(1, EE_COLOR) });
	p.push_back({ "q10 low_chroma 1 lparts 2", low10(1, 2), q10_forked(2, EE_COLOR) });
	p.push_back({ "q10 low_chroma 2 lparts 1", low10(2, 1), q10_forked(1, EE_COLOR) });
	p.push_back({ "q10 low_chroma 2 lparts 2", low10(2, 2), q10_forked(2, EE_LOW_PASS_A) });
	/* the in-line order */
	const Steps inline_low_tail = { K(EMIT, MAIN, 0, 0), K(LL_CODER, MAIN, 0, 0), K(L4A, MAIN, 0, 0), K(L4C, MAIN, 0, 0), K(QUANT, MAIN, 0, 0), K(Y31, MAIN, 0, 0), ST, T(LUMA) };
	p.push_back({ "in line q5", inline_of(5), cat({ front_low(2, false), loop_6, low_ll2, inline_low_tail, INLINE_CHROMA(HEAD_14, 1), end_inline }) });
	p.push_back({ "in line q10", inline_of(10), cat({ front_low(2, false), LOOP_12(1, Y5_INLINE), low_ll2, inline_low_tail, INLINE_CHROMA(HEAD_14, 1), end_inline }) });
	p.push_back({ "in line q23", inline_of(23), cat({ front_22, LOOP_13(1, Y5_INLINE), { ST, K(EMIT, MAIN, 0, 0), K(LL_CODER, MAIN, 0, 0), K(DQ0, MAIN, 2, 0), ST, K(L_SYN2, MAIN, 0, 0), ST, K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0),
	                                               K(QUANT, MAIN, 1, 0), K(L4C2, MAIN, 0, 0), K(Y31, MAIN, 0, 0), ST, T(LUMA) }, INLINE_CHROMA(HEAD_17, 1), end_inline }) });
	/* the compatibility mode (forked: no lean stores, the LL2 coder in line) */
	p.push_back({ "compat q10", compat_of(10), cat({ front_low(2, true), { WAIT(LOW_PASS_A, CHROMA) }, HEAD_14(CHROMA, 0), HEAD_14(CHROMA, 2), LOOP_12(0, Y5_BESIDE), low_ll2, { K(EMIT, MAIN, 0, 0), CODER_FORK, K(L4A, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2,
	                                              { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 0, 0) }, end_fork }) });
	p.push_back({ "compat q20", compat_of(20), cat({ front_17_compat, q20_heads, LOOP_13(0, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_FORK, K(DQ0, MAIN, 3, 0), ST, K(L_SYN2, MAIN, 1, 0), ST }, q20_resid, rest_2, q20_join, end_fork }) });
	p.push_back({ "compat q23", compat_of(23), cat({ front_22, q20_heads, LOOP_13(0, Y5_BESIDE), { ST, K(EMIT, MAIN, 1, 0), CODER_FORK, K(DQ0, MAIN, 3, 0), ST, K(L_SYN2, MAIN, 0, 0), ST, K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0) }, rest_2,
	                                              { WAIT(CHROMA_DONE, MAIN), K(QUANT, MAIN, 1, 0), K(L4C2, MAIN, 0, 0) }, end_fork }) });
	/* a batch in sub-batches at quality 20: the front group for all of it, then a view (the first one carries the two stage stamps) */
	{ EncIn in = defaults(20); in.what = 1; in.timed = 0; p.push_back({ "what 1 q20", in, { T(COLOR), T(PREFILTER), ST, ST, K(FRONT, MAIN, 0, 0), ST, ST } }); }
	{ EncIn in = defaults(20); in.what = 2; in.timed = 2; p.push_back({ "what 2 q20", in, cat({ { WAIT(PART_FRONT, MAIN) }, q20_inline_tail(1), { T(LUMA) }, INLINE_CHROMA(HEAD_17, 1), { T(CHROMA), K(LLC, MAIN, 0, 0), K(FINAL, MAIN, 0, 0) } }) }); }
	return p;
}
/* The whole sequence of a batch under a debug stop that lies behind its last boundary, at quality 10, 20 and 23: stop k is its part up to the
 * k-th boundary.  One set of chroma planes, the staged kernels, every plane stored, no marks. */
static Steps stopped(int q)
{
	if (q == 10) return cat({ front_low(1, false), LOOP_DBG(0), low_ll2, { K(EMIT, MAIN, 0, 0), K(LL_CODER, MAIN, 0, 0), K(L4A, MAIN, 0, 0), K(L4C, MAIN, 0, 0), K(QUANT, MAIN, 0, 0), K(Y31, MAIN, 0, 0), ST, T(LUMA) },
	                          HEAD_DBG_14(0), { K(C_TAIL, MAIN, 0, 0), ST }, HEAD_DBG_14(1), { K(C_TAIL, MAIN, 1, 0), ST }, end_inline });
	const Steps tail20 = { ST, K(EMIT, MAIN, 0, 0), K(LL_CODER, MAIN, 0, 0), K(DQ0, MAIN, 0, 0), ST, K(L_SYN2, MAIN, 0, 0), ST, K(L4A, MAIN, 0, 0), K(L4B, MAIN, 0, 0), K(L4C, MAIN, 0, 0), K(QUANT, MAIN, 0, 0) };
	const Steps chroma = cat({ HEAD_DBG_17(0), { K(C_TAIL, MAIN, 0, 0), ST }, HEAD_DBG_17(1), { K(C_TAIL, MAIN, 1, 0), ST }, end_inline });
	if (q == 20) return cat({ front_17, LOOP_DBG(1), tail20, { K(Y31, MAIN, 0, 0), ST, T(LUMA) }, chroma });
	return cat({ front_22, LOOP_DBG(1), tail20, { K(L4C2, MAIN, 0, 0), K(Y31, MAIN, 0, 0), ST, T(LUMA) }, chroma });
}
static Steps upto_boundary(const Steps &v, int k)
{
	int seen = 0;
	for (size_t i = 0; i < v.size(); i++) if (v[i].op == ENC_STAGE && ++seen == k) return Steps(v.begin(), v.begin() + (long)i + 1);
	return v;
}
/* quant_join 0 as the driver issued it before: the wait for the lists' event behind Y31 */
static Steps old_late_join()
{
	return cat({ front_17, q20_heads, LOOP_13(1, Y5_BESIDE), { ST }, q20_second, q20_resid, { K(QUANT, MAIN, 1, 0) }, rest_2,
	             { K(Y31, MAIN, 0, 0), ST, T(LUMA), WAIT(LISTS, MAIN), WAIT(CHROMA_DONE, MAIN), T(CHROMA), K(FINAL, MAIN, 1, 0), T(END) } });
}

/* ------------------------------------------------------------------------------------------------ the walk */
/* the ten switches other than low_parts as one number: low_chroma (3) x pack_fork (3) x eight flags */
enum { COMBOS = 3 * 3 * 256 };
enum { F_CHROMA = 1, F_LISTS = 2, F_LL = 4, F_JOIN = 8, F_Y5 = 16, F_LL2 = 32, F_MARKS = 64, F_ONCE = 128 };
static void set_combo(EncIn &in, int c)
{
	const int f = c & 255;
	in.chroma_fork = !!(f & F_CHROMA); in.lists_fork = !!(f & F_LISTS); in.ll_fork = !!(f & F_LL); in.quant_join = !!(f & F_JOIN); in.y5_fork = !!(f & F_Y5);
	in.ll2_once = !!(f & F_LL2); in.quant_marks = !!(f & F_MARKS); in.chroma_tail_once = !!(f & F_ONCE);
	in.low_chroma = (c >> 8) % 3; in.pack_fork = (c >> 8) / 3;
}
static int combo(int flags, int low_chroma, int pack_fork) { return flags | ((low_chroma + 3 * pack_fork) << 8); }

int main()
{
	long plans = 0;
	std::unordered_map<std::string, int> ids;                               /* a plan with what its checks depend on -> its number: (a), (b) and (c) run once a distinct plan */
	auto check_plan = [&](const EncIn &in) -> int {
		const EncPlan p = enc_plan(in);
		plans++;
		if (!p.n) { fail(where_of(in), "an empty plan inside the domain"); return -1; }
		std::string key((const char *)p.step, (size_t)p.n * sizeof(EncStep));
		const char tail[10] = { (char)in.q, (char)in.compat, (char)in.stop, (char)in.what, (char)in.timed, (char)p.dbg, (char)p.split_chroma, (char)p.defer_verbatim, (char)p.low_parts_used, (char)(p.timed + 2 * in.big) };
		key.append(tail, sizeof tail);
		const auto it = ids.find(key);
		if (it != ids.end()) return it->second;
		const int id = (int)ids.size();
		ids.emplace(key, id);
		const std::string where = where_of(in);
		const Steps v = steps_of(p);
		check_shape(p, in, where);
		check_events(v, in, where);
		unordered_conflicts(v, in.q, in.compat != 0, p.dbg != 0, where, true);
		return id;
	};
	static const int pairs[4][2] = { { 3, 1 }, { 1, 0 }, { 2, 2 }, { 2, 0 } };
	std::vector<int> id((size_t)COMBOS);
	for (int q = 1; q <= 23; q++)
		for (int compat = 0; compat < 2; compat++) {
			int stages = -1;
			for (const auto &pr : pairs)
				for (int big = 0; big < 2; big++)
					for (int lp = 1; lp <= 2; lp++) {
						EncIn in = defaults(q);
						in.compat = compat; in.what = pr[0]; in.timed = pr[1]; in.big = big; in.low_parts = lp;
						for (int c = 0; c < COMBOS; c++) { set_combo(in, c); id[(size_t)c] = check_plan(in); }
						/* d. what a switch must not change: combination c against the one with the switches in question cleared */
						const bool whole = pr[0] == 3;
						for (int c = 0; c < COMBOS; c++) {
							const int f = c & 255, lc = (c >> 8) % 3, pf = (c >> 8) / 3;
							set_combo(in, c);
							auto must_equal = [&](int other, const char *why) { if (id[(size_t)c] != id[(size_t)other]) fail(where_of(in), why); };
							if (!whole) must_equal(combo(f & (F_ONCE | F_MARKS), 0, 0), "outside a whole batch a switch other than chroma_tail_once and quant_marks changes the plan");
							if (!(f & F_CHROMA)) must_equal(combo(f & (F_ONCE | F_MARKS), 0, 0), "with chroma_fork off, lists_fork, ll_fork, quant_join, y5_fork, ll2_once, pack_fork or low_chroma changes the plan");
							if (!(q > 13 && !compat)) must_equal(combo(f & ~F_LL, lc, pf), "ll_fork changes a plan of q <= 13 or of the compatibility mode");
							if (!(q >= 13 && q <= 20)) must_equal(combo(f & ~F_LISTS, lc, pf), "lists_fork changes a plan outside q 13 .. 20");
							if (!(q > 12)) must_equal(combo(f & ~F_LL2, lc, pf), "ll2_once changes a plan of q <= 12");
							if (!(q > 6)) must_equal(combo(f & ~F_Y5, lc, pf), "y5_fork changes a plan of q <= 6");
							if (!(q > 16)) must_equal(combo(f & ~F_MARKS, lc, pf), "quant_marks changes a plan of q <= 16");
							if (!(q <= 16)) must_equal(combo(f, 0, pf), "low_chroma changes a plan of q > 16");
						}
						if (!(q <= 16) || !whole || !big) {                  /* low_parts: only where the pre-filter runs in sub-batches */
							EncIn other = in;
							other.low_parts = 3 - lp;
							for (int c = 0; c < COMBOS; c += 37) { set_combo(in, c); set_combo(other, c); if (!same(steps_of(enc_plan(in)), steps_of(enc_plan(other)))) fail(where_of(in), "low_parts changes a plan of q > 16, of a small batch or of a part"); }
						}
						/* c. the stage count of an unstopped in-line plan is the same at every switch setting (and whatever n is) */
						if (whole) for (int c = 0; c < COMBOS; c++) if (!(c & F_CHROMA)) {
							set_combo(in, c);
							const int k = stage_count(steps_of(enc_plan(in)));
							if (stages < 0) stages = k; else if (k != stages) fail(where_of(in), "the stage count of the in-line plan depends on a switch");
						}
					}
			/* every stop: the default switches, all of them off, each one changed alone -- under a stop no switch changes the plan */
			for (int stop = 1; stop <= STOPS; stop++) {
				EncIn in = defaults(q);
				in.compat = compat; in.stop = stop;
				const int want = check_plan(in);
				for (int v = 0; v < 12; v++) {                       /* 0: all off; 1 .. 11: one switch changed */
					EncIn o = in;
					if (v == 0) { set_combo(o, 0); o.low_parts = 1; }
					int *const sw[11] = { &o.low_chroma, &o.chroma_fork, &o.lists_fork, &o.ll_fork, &o.quant_join, &o.y5_fork, &o.ll2_once, &o.quant_marks, &o.chroma_tail_once, &o.pack_fork, &o.low_parts };
					if (v > 0) *sw[v - 1] = v == 11 ? 1 : !*sw[v - 1];
					if (check_plan(o) != want) fail(where_of(o), "a switch changes a plan with a debug stop");
				}
				if (stages >= 0 && stop <= stages && stage_count(steps_of(enc_plan(in))) != stop) fail(where_of(in), "the stop does not count the in-line plan's boundaries");
			}
		}
	/* front_fallback reaches the front group's two kernels and nothing else */
	for (int q = 1; q <= 23; q++) {
		EncIn a = defaults(q), b = a;
		b.front_fallback = 1;
		Steps x = steps_of(enc_plan(a)), y = steps_of(enc_plan(b));
		for (EncStep &s : y) { if (s.op == ENC_LOW_PREFILTER) s.b = 0; if (s.op == ENC_FRONT) s.a = 0; }
		if (!same(x, y) || same(x, steps_of(enc_plan(b)))) fail(where_of(b), "front_fallback changes more, or less, than the front kernels' argument");
	}
	/* outside the domain: an empty plan */
	{
		EncIn o = defaults(20);
		o.q = 0; if (enc_plan(o).n) fail("q 0", "a plan outside the domain");
		o.q = 24; if (enc_plan(o).n) fail("q 24", "a plan outside the domain");
		o = defaults(20); o.what = 1; if (enc_plan(o).n) fail("what 1 timed 1", "a plan outside the domain");
		o = defaults(20); o.what = 3; o.timed = 2; if (enc_plan(o).n) fail("what 3 timed 2", "a plan outside the domain");
	}
	/* e. */
	int pinned = 0;
	for (const Pin &pin : pins()) {
		const Steps got = steps_of(enc_plan(pin.in));
		pinned++;
		if (!same(got, pin.want)) fail(pin.name, "the plan is\n  " + show(got) + "\nand the pinned sequence\n  " + show(pin.want));
	}
	for (int q : { 10, 20, 23 }) {
		const Steps whole = stopped(q);
		for (int stop = 1; stop <= STOPS; stop++) {
			EncIn in = defaults(q);
			in.stop = stop;
			const Steps got = steps_of(enc_plan(in)), want = upto_boundary(whole, stop);
			pinned++;
			if (!same(got, want)) fail("q " + std::to_string(q) + " stop " + std::to_string(stop), "the plan is\n  " + show(got) + "\nand the pinned sequence\n  " + show(want));
		}
	}
	/* the check itself: it must see what was wrong with the old order of quant_join 0, and only that -- Y24 / Y25 beside Y31, on B_HALF */
	{
		std::string pairs_found;
		const int k = unordered_conflicts(old_late_join(), 20, false, false, "the old order of quant_join 0", false, &pairs_found);
		if (k != 1 || pairs_found != "l4b@lists(0,0)/y31(0,0): " + std::to_string(B_HALF) + ";") fail("the old order of quant_join 0", "the order check does not report exactly the l4b / y31 pair on B_HALF, but: " + pairs_found);
	}
	printf("plans %ld pinned %d mismatches %d\n", plans, pinned, mismatches);
	return mismatches ? 1 : 0;
}
