/* The decoder's batch plans (nhwcodec_amd/csrc/nhw_dec_plan.h) held against the header's own resource table and against the sequences the
 * batch driver issued before it had a planner, on the CPU (tests/test_dec_plan.py builds and runs this, plain and under the sanitizers).
 * Over the whole domain -- 3 scales x colour or grey x fork bits 0 .. 7 at stop 0, stops 1 .. 11 x bits 0 .. 7 at scale 1 colour:
 *   a. order: in the happens-before relation of a plan (program order on either stream, the fork and join edges) every two steps of which one
 *      writes what the other reads or writes are ordered;
 *   b. shape: stamp 0 first, status last, the second stream only between a fork and a join that is waited for, stamps 2 and 3 around the last
 *      kernel and nothing else, `timed` and `l1_moved` as the steps say;
 *   c. grey plans: no chroma, no sharpen, nothing of D_CA, D_CU, and of D_CB nothing behind the verdict; the second stream only under bit 0;
 *   d. what the bits do not change;
 *   e. the pin: the literal sequences below, transcribed from the driver as it was.
 * "Bit k" here is the bit of value 1 << k of NHW_DEC_FORK (the header names the bits by their values 1, 2, 4).
 * Prints "plans <n> pinned <m> mismatches <k>"; k = 0 is success. */
#include <stdio.h>

#include <string>
#include <vector>

#include "../../nhwcodec_amd/csrc/nhw_dec_plan.h"

static int mismatches = 0;
static void fail(const std::string &where, const std::string &what)
{
	mismatches++;
	printf("%s: %s\n", where.c_str(), what.c_str());
}

typedef std::vector<DecStep> Steps;
static const char *const op_name[DEC_OP_COUNT] = { "stamp", "fork", "join-record", "join-wait", "parse", "vlc", "verdict", "expand", "chroma", "sharpen",
	"l2q", "marks", "marks-far", "last", "status" };
static std::string show(const DecStep &s) { return std::string(op_name[s.op]) + (s.side ? "@side" : "") + "(" + std::to_string(s.arg) + ")"; }
static std::string show(const Steps &v) { std::string r; for (const DecStep &s : v) r += show(s) + " "; return r; }
static bool same(const Steps &a, const Steps &b)
{
	if (a.size() != b.size()) return false;
	for (size_t i = 0; i < a.size(); i++) if (a[i].op != b[i].op || a[i].side != b[i].side || a[i].arg != b[i].arg) return false;
	return true;
}
static Steps steps_of(const DecPlan &p) { return Steps(p.step, p.step + p.n); }
static Steps plan(int scale, bool grey, int stop, int bits) { return steps_of(dec_plan(scale, grey, stop, bits)); }

/* ------------------------------------------------------------------------------------------------ a. order */
/* the conflicts of `v` that its happens-before relation leaves unordered; a join-wait without a record in front of it counts as one */
static int unordered_conflicts(const Steps &v, bool grey, const std::string &where, bool report)
{
	const int n = (int)v.size();
	std::vector<std::vector<char>> hb((size_t)n, std::vector<char>((size_t)n, 0));
	for (int i = 0; i < n; i++) {
		for (int j = i + 1; j < n; j++) if (v[j].side == v[i].side) { hb[i][j] = 1; break; }       /* program order: the next step of the stream */
		if (v[i].op == DEC_FORK) for (int j = i + 1; j < n; j++) if (v[j].side == 1) { hb[i][j] = 1; break; }   /* the second stream waits from here on */
		if (v[i].op == DEC_JOIN_WAIT) {                               /* ... for the record last enqueued */
			int r = i - 1;
			while (r >= 0 && v[r].op != DEC_JOIN_RECORD) r--;
			if (r >= 0) hb[r][i] = 1;
		}
	}
	for (int k = 0; k < n; k++) for (int i = 0; i < n; i++) if (hb[i][k]) for (int j = 0; j < n; j++) if (hb[k][j]) hb[i][j] = 1;
	int found = 0;
	for (int i = 0; i < n; i++)
		for (int j = i + 1; j < n; j++) {
			const DecAccess a = dec_access(v[i].op, v[i].arg, grey), b = dec_access(v[j].op, v[j].arg, grey);
			const uint32_t clash = (a.writes & (b.reads | b.writes)) | (b.writes & a.reads);
			if (!clash || hb[i][j]) continue;
			found++;
			if (report) fail(where, "steps " + std::to_string(i) + " " + show(v[i]) + " and " + std::to_string(j) + " " + show(v[j]) + " are not ordered and share resources " + std::to_string(clash));
		}
	return found;
}

/* ------------------------------------------------------------------------------------------------ b. shape */
static void check_shape(const DecPlan &p, const std::string &where)
{
	const Steps v = steps_of(p);
	const int n = (int)v.size();
	if (n < 3) return fail(where, "a plan of fewer than three steps");
	if (v[0].op != DEC_STAMP || v[0].side || v[0].arg != 0) fail(where, "does not begin with stamp 0 on the main stream");
	if (v[n - 1].op != DEC_STATUS || v[n - 1].side) fail(where, "does not end with status on the main stream");
	bool open = false, pending = false, last = false, l2q = false;
	for (int i = 0; i < n; i++) {
		const DecStep &s = v[i];
		const bool on_side = s.side != 0;
		if (s.side > 1 || s.op >= DEC_OP_COUNT) fail(where, "step " + std::to_string(i) + " is no step");
		if ((s.op == DEC_STAMP || s.op == DEC_FORK || s.op == DEC_JOIN_WAIT || s.op == DEC_STATUS || s.op == DEC_LAST) && on_side) fail(where, show(s) + " on the side stream");
		if (s.op == DEC_JOIN_RECORD && !on_side) fail(where, "a join record on the main stream");
		if (on_side && !open) fail(where, show(s) + " on the side stream outside a fork");
		if (s.op == DEC_FORK) { if (open || pending) fail(where, "a fork inside a fork"); open = true; }
		if (s.op == DEC_JOIN_RECORD) { open = false; pending = true; }
		if (s.op == DEC_JOIN_WAIT) { if (!pending || open) fail(where, "a wait without a record"); pending = false; }
		if (s.op == DEC_STATUS && (open || pending || i != n - 1)) fail(where, "status in front of a join, or not last");
		if (s.op == DEC_STAMP && s.arg > 3) fail(where, "a stamp that is none of 0 .. 3");
		if (s.op == DEC_CHROMA && (s.arg < 1 || s.arg > 5)) fail(where, "chroma upto outside 1 .. 5");
		if (s.op == DEC_L2Q && (s.arg < 1 || s.arg > 3)) fail(where, "l2q UPTO outside 1 .. 3");
		if (s.op == DEC_LAST) {
			if (last) fail(where, "two last kernels");
			last = true;
			if (i < 1 || i + 1 >= n || v[i - 1].op != DEC_STAMP || v[i - 1].arg != 2 || v[i + 1].op != DEC_STAMP || v[i + 1].arg != 3) fail(where, "the last kernel is not between stamps 2 and 3");
		}
		if (s.op == DEC_STAMP && s.arg == 2 && (i + 1 >= n || v[i + 1].op != DEC_LAST)) fail(where, "stamp 2 not in front of the last kernel");
		if (s.op == DEC_STAMP && s.arg == 3 && (i < 1 || v[i - 1].op != DEC_LAST)) fail(where, "stamp 3 not behind the last kernel");
		if (s.op == DEC_L2Q) l2q = true;
	}
	if (p.timed != last) fail(where, "`timed` does not say whether the last kernel is in the plan");
	if (p.l1_moved != l2q) fail(where, "`l1_moved` does not say whether k_dec_luma_l2q is in the plan");
}

/* ------------------------------------------------------------------------------------------------ c. grey */
static void check_grey(const Steps &v, int bits, const std::string &where)
{
	bool verdict = false;
	for (const DecStep &s : v) {
		const DecAccess a = dec_access(s.op, s.arg, true);
		const uint32_t touched = a.reads | a.writes;
		if (s.op == DEC_CHROMA || s.op == DEC_SHARPEN) fail(where, "a grey plan with " + show(s));
		if (s.side && !(bits & 1)) fail(where, show(s) + " on the side stream of a grey plan without bit 0");
		if (touched & (R_CA | R_CU)) fail(where, show(s) + " touches D_CA or D_CU");
		if (verdict && (touched & R_CB)) fail(where, show(s) + " touches D_CB behind the verdict");
		if (s.op == DEC_VERDICT) verdict = true;
	}
}

/* ------------------------------------------------------------------------------------------------ e. the pin */
#define M(OP, ARG) { DEC_##OP, 0, ARG }
#define S(OP, ARG) { DEC_##OP, 1, ARG }
#define T0 M(STAMP, 0)
#define T1 M(STAMP, 1)
#define T2 M(STAMP, 2)
#define T3 M(STAMP, 3)
#define FK M(FORK, 0)
#define JR S(JOIN_RECORD, 0)
#define JW M(JOIN_WAIT, 0)
#define PA M(PARSE, 0)
#define VL M(VLC, 0)
#define VLs S(VLC, 0)
#define VE M(VERDICT, 0)
#define EX M(EXPAND, 0)
#define C(K) M(CHROMA, K)
#define C4s S(CHROMA, 4)
#define SH M(SHARPEN, 0)
#define SHs S(SHARPEN, 0)
#define Q(K) M(L2Q, K)
#define MK M(MARKS, 0)
#define MF M(MARKS_FAR, 0)
#define F(K) M(LAST, K)
#define ST M(STATUS, 0)
struct Pin { int scale; bool grey; int stop, bits; Steps want; };
/* The sequences of dec_batch as it stood before the planner, read off its text: (operation, stream, argument) in the order enqueued.
 * TWO OF THEM ARE NOT WHAT IT ISSUED: with bit 1 (values 2, 3, and 6, 7, which equal them) it recorded the fork event in front of k_dec_verdict
 * -- "... VL FK VE T1 EX C4s ..." -- so that k_dec_chroma on the second stream read DecMeta's status beside the kernel that settles it, which
 * check (a) reports (old_fork_order below keeps that sequence to show it).  The record now stands behind the verdict: "... VL VE FK T1 ...". */
static const Pin pins[] = {
	/* the debug stops, bits 0 */
	{ 1, false, 0, 0, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, C(4), SH, T2, F(1), T3, ST } },
	{ 1, false, 1, 0, { T0, PA, ST } },
	{ 1, false, 2, 0, { T0, PA, VL, VE, T1, ST } },
	{ 1, false, 3, 0, { T0, PA, VL, VE, T1, EX, C(1), ST } },
	{ 1, false, 4, 0, { T0, PA, VL, VE, T1, EX, Q(1), ST } },
	{ 1, false, 5, 0, { T0, PA, VL, VE, T1, EX, Q(2), ST } },
	{ 1, false, 6, 0, { T0, PA, VL, VE, T1, EX, Q(3), ST } },
	{ 1, false, 7, 0, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, ST } },
	{ 1, false, 8, 0, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, C(2), ST } },
	{ 1, false, 9, 0, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, C(3), ST } },
	{ 1, false, 10, 0, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, C(4), ST } },
	{ 1, false, 11, 0, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, C(4), SH, ST } },
	/* the fork bits, stop 0, scale 1, colour */
	{ 1, false, 0, 1, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, Q(3), MK, MF, C(4), SH, T2, F(1), T3, ST } },
	{ 1, false, 0, 2, { T0, PA, VL, VE, FK, T1, EX, C4s, SHs, JR, Q(3), MK, MF, JW, T2, F(1), T3, ST } },
	{ 1, false, 0, 3, { T0, FK, PA, VLs, JR, JW, VE, FK, T1, EX, C4s, SHs, JR, Q(3), MK, MF, JW, T2, F(1), T3, ST } },
	{ 1, false, 0, 4, { T0, PA, VL, VE, T1, EX, Q(3), FK, C4s, SHs, JR, MK, MF, JW, T2, F(1), T3, ST } },
	{ 1, false, 0, 5, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, Q(3), FK, C4s, SHs, JR, MK, MF, JW, T2, F(1), T3, ST } },
	{ 1, false, 0, 6, { T0, PA, VL, VE, FK, T1, EX, C4s, SHs, JR, Q(3), MK, MF, JW, T2, F(1), T3, ST } },
	{ 1, false, 0, 7, { T0, FK, PA, VLs, JR, JW, VE, FK, T1, EX, C4s, SHs, JR, Q(3), MK, MF, JW, T2, F(1), T3, ST } },
	/* the scaled plans under the default bits and under bits 0 and 1 */
	{ 2, false, 0, 4, { T0, PA, VL, VE, T1, EX, Q(3), C(4), SH, T2, F(2), T3, ST } },
	{ 2, false, 0, 3, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, Q(3), C(4), SH, T2, F(2), T3, ST } },
	{ 2, true, 0, 4, { T0, PA, VL, VE, T1, EX, Q(3), T2, F(2), T3, ST } },
	{ 2, true, 0, 3, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, Q(3), T2, F(2), T3, ST } },
	{ 4, false, 0, 4, { T0, PA, VL, VE, T1, EX, C(5), T2, F(4), T3, ST } },
	{ 4, false, 0, 3, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, C(5), T2, F(4), T3, ST } },
	{ 4, true, 0, 4, { T0, PA, VL, VE, T1, EX, T2, F(4), T3, ST } },
	{ 4, true, 0, 3, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, T2, F(4), T3, ST } },
	/* grey at scale 1 */
	{ 1, true, 0, 4, { T0, PA, VL, VE, T1, EX, Q(3), MK, MF, T2, F(1), T3, ST } },
	{ 1, true, 0, 3, { T0, FK, PA, VLs, JR, JW, VE, T1, EX, Q(3), MK, MF, T2, F(1), T3, ST } },
};
/* bit 1 as the driver issued it before: the fork recorded in front of the verdict */
static const Steps old_fork_order = { T0, PA, VL, FK, VE, T1, EX, C4s, SHs, JR, Q(3), MK, MF, JW, T2, F(1), T3, ST };

int main()
{
	int plans = 0;
	auto where_of = [](int scale, bool grey, int stop, int bits) {
		return "scale " + std::to_string(scale) + (grey ? " grey" : " colour") + " stop " + std::to_string(stop) + " bits " + std::to_string(bits);
	};
	auto check_plan = [&](int scale, bool grey, int stop, int bits) {
		const std::string where = where_of(scale, grey, stop, bits);
		const DecPlan p = dec_plan(scale, grey, stop, bits);
		plans++;
		if (!p.n) return fail(where, "an empty plan inside the domain");
		check_shape(p, where);
		unordered_conflicts(steps_of(p), grey, where, true);
		if (grey) check_grey(steps_of(p), bits, where);
	};
	for (int scale = 1; scale <= 4; scale *= 2)
		for (int grey = 0; grey < 2; grey++)
			for (int bits = 0; bits < 8; bits++) {
				check_plan(scale, grey != 0, 0, bits);
				/* d. bits 1 and 2 change no scaled and no grey plan; bit 1 set makes bit 2 irrelevant; bits above the third do not count */
				if ((scale != 1 || grey) && !same(plan(scale, grey != 0, 0, bits), plan(scale, grey != 0, 0, bits & 1))) fail(where_of(scale, grey != 0, 0, bits), "bits 1 or 2 change a scaled or grey plan");
				if ((bits & 2) && !same(plan(scale, grey != 0, 0, bits), plan(scale, grey != 0, 0, bits & ~4))) fail(where_of(scale, grey != 0, 0, bits), "bit 2 changes a plan that has bit 1");
				if (!same(plan(scale, grey != 0, 0, bits), plan(scale, grey != 0, 0, bits | 8))) fail(where_of(scale, grey != 0, 0, bits), "a bit above the third changes the plan");
			}
	for (int stop = 1; stop <= 11; stop++)
		for (int bits = 0; bits < 8; bits++) {
			check_plan(1, false, stop, bits);
			if (!same(plan(1, false, stop, bits), plan(1, false, stop, 0))) fail(where_of(1, false, stop, bits), "the bits change a plan with a debug stop");   /* d. */
		}
	/* outside the domain: an empty plan */
	const int outside[][4] = { { 3, 0, 0, 0 }, { 0, 0, 0, 4 }, { 8, 0, 0, 4 }, { 1, 0, 12, 0 }, { 1, 0, -1, 0 }, { 2, 0, 3, 0 }, { 4, 0, 1, 4 }, { 1, 1, 4, 0 }, { 2, 1, 4, 4 } };
	for (const auto &o : outside) if (dec_plan(o[0], o[1] != 0, o[2], o[3]).n) fail(where_of(o[0], o[1] != 0, o[2], o[3]), "a plan outside the domain");
	/* e. */
	int pinned = 0;
	for (const Pin &pin : pins) {
		const Steps got = plan(pin.scale, pin.grey, pin.stop, pin.bits);
		pinned++;
		if (!same(got, pin.want)) fail(where_of(pin.scale, pin.grey, pin.stop, pin.bits), "the plan is\n  " + show(got) + "\nand the pinned sequence\n  " + show(pin.want));
	}
	/* the check itself: it must see what was wrong with the old order of bit 1, and only that -- the verdict beside the chroma kernel and beside the
	 * sharpen kernel, all three on DecMeta's header part */
	if (unordered_conflicts(old_fork_order, false, "the old order of bit 1", false) != 2) fail("the old order of bit 1", "the order check does not report exactly the verdict / chroma and verdict / sharpen pairs");
	printf("plans %d pinned %d mismatches %d\n", plans, pinned, mismatches);
	return mismatches ? 1 : 0;
}
