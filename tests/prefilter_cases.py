"""Pictures for the carry paths of pass A of the quality 1..16 pre-filter (nhwcodec_amd/csrc/nhw_low.hip, k_low_pre), shared by
test_prefilter_census.py and test_prefilter_carry.py: the pictures themselves, the inverse of the colour stage that turns a luma plane into
a grey BGR picture, a numpy restatement of pass A's look-back that says which of k_low_pre's paths a picture takes (the CENSUS), and the
oracle's planes.

The restatement QUALIFIES INPUTS ONLY.  No expected value of any test comes from it: those come from the oracle (oracle/nhwo_prelow.c through
tests/low_machine/oracle_side.c), and the restated map is itself checked against the oracle's pass A on every picture that is used.

What it restates (k_low_pre's comments, oracle contrast_map_low):
  vb = sign(sm) (15 |sm| + mg)        sm: the sum of the eight differences centre - neighbour, mg: the sum of their magnitudes
  vb == 0 sets the state to 0; otherwise acc = |vb| + ((cr + 2) >> 2), the map cell is sign(vb) (acc >> 4) and the state becomes acc & 15
  lane l of a row holds cells 8 l .. 8 l + 7.  A lane with 8 l > 16 is FAR: it starts from the five candidates (|vb| + 0..4) & 15 of the first of
  the sixteen cells in front of it (the one state 0 where that cell's vb is 0), follows them through the other fifteen, and is MERGED when one
  state is left, OPEN otherwise.  An open lane takes its entry state from the lane on its left (the hand-over loop).
  A band of 32 rows starts at row r0 = 1 + 32 b.  Its entry state is the exit state of row r0 - 1 where that row's last lane is merged; otherwise
  the band goes back row by row to a row whose last lane is merged, or to row 0.  DEPTH: the rows it goes back, r0 - (the row it stops at).
The marker rule of pass A (+-20000, 7000 and the three bumped cells) rewrites map cells but never the state: the restated map is the map in front
of that rule, and map_agrees says what the rule may have done to a cell.
"""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from tests.support import ROOT

S = 512
RB = 32                       # PRE_RB
NB = 16                       # PRE_NB
FAR0 = 3                      # the first far lane: 8 l > PF_LOOK = 16
SUITE_Q = 10                  # the quality the record of the suite's own pictures is taken at (test_prefilter_matches_oracle and the encodes around it)
SHARP_BY_Q = (0, 48, 45, 36, 24, 24, 0, 0, 0, 1, 17, 35, 41, 44, 49, 54, 59)      # oracle params_for
P2_DEPTHS = {2: 33, 4: 32, 6: 31, 8: 2, 10: 3, 12: 4}                              # band -> the depth P2 gives it


def sharp2(q):
    return max(10, SHARP_BY_Q[q])


# ---------------------------------------------------------------------------------------------------------------- colour, inverted
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oraclepy import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def luma_levels(q):
    """grey[l]: the grey level (R = G = B) whose luma at quality q is l, -1 where none is; taken from oracle.color on a picture that holds
    all 256 levels.  Every level between the smallest and the largest is reached (asserted)."""
    g = (np.arange(S * S) % 256).astype(np.uint8).reshape(S, S)
    y = _oracle().color(np.repeat(g[:, :, None], 3, 2), q)[0].reshape(S, S)
    assert all(np.array_equal(y[r], y[0]) for r in (1, 255, 511)), "the luma of a grey pixel depends on where it stands"
    lum = y[0, :256].astype(int)
    assert np.all(np.diff(lum) >= 0)
    grey = np.full(int(lum.max()) + 1, -1)
    grey[lum[::-1]] = np.arange(255, -1, -1)
    lo, hi = int(lum.min()), int(lum.max())
    assert np.all(grey[lo:] >= 0), f"q{q}: luma levels between {lo} and {hi} that no grey level gives"
    return lo, hi, grey


def bgr_of(luma, q):
    """luma plane (512 x 512 ints inside quality q's range) -> the grey BGR picture whose colour stage gives it"""
    lo, hi, grey = luma_levels(q)
    luma = np.asarray(luma)
    assert luma.shape == (S, S) and luma.min() >= lo and luma.max() <= hi, (q, lo, hi, int(luma.min()), int(luma.max()))
    return np.repeat(grey[luma].astype(np.uint8)[:, :, None], 3, 2)


# ---------------------------------------------------------------------------------------------------------------- the pictures
def _ramp(n):
    """n columns that rise by 2, 3, 2, 3 ..: constant down the picture every cell has |vb| = 60, and the state cycles 0 -> 12 -> 15 -> 0"""
    return np.concatenate([[0], np.cumsum(np.tile([2, 3], n)[:n - 1])])


def _noise(seed, lo, hi):
    from oracle.harness import _hash_u32
    return lo + (_hash_u32(np.arange(S * S, dtype=np.uint64), seed) >> 8).astype(np.int64).reshape(S, S) % (hi - lo + 1)


def _saw(width, period, lo):
    return lo + _ramp(period)[np.arange(width) % period]


def saw_period(q):
    """48 columns of slope 2.5 where quality q's luma range holds them, fewer below"""
    lo, hi, _ = luma_levels(q)
    return min(48, int((hi - lo) / 2.5))


def _stretches(lo):
    """flat at the range's low end, a never-merging ramp over the row's first 42 columns and one over its last 42 (102 levels: quality 1 has
    106).  Row r steps onto the last one at column 470 + (3 r) % 7, so that the state a row ends in is not the same in every row; from column
    478 on the cells see columns that are constant down the picture (the last lane looks back over 488 .. 503)."""
    y = np.full((S, S), lo, np.int64)
    y[:, :42] = lo + _ramp(42)
    for r in range(S):
        c = 470 + (3 * r) % 7
        y[r, c:] = lo + _ramp(42)[c - 470:]
    return y


def p1(q):
    """P1: the last lane of no row merges, every band b = 1 .. 15 goes back 32 b + 1 rows to row 0"""
    return _stretches(luma_levels(q)[0])


def p2(q):
    """P2: P1 with one merging row placed for each of six bands (P2_DEPTHS): pixel row m - 1 flat from column 460 on makes map row m merge and
    leaves map row m + 1 alone (a map cell sees three pixel rows)"""
    lo = luma_levels(q)[0]
    y = _stretches(lo)
    for b, d in P2_DEPTHS.items():
        m = 1 + RB * b - d
        y[m - 1, 460:] = lo
    return y


def p3(q):
    """P3: the 2, 3 ramp as a sawtooth over the whole width: most far lanes of every row are open, in runs of several lanes"""
    return np.tile(_saw(S, saw_period(q), luma_levels(q)[0]), (S, 1))


def p4(q):
    """P4: half P3's sawtooth (the first 130 and the last 128 columns), half noise (markers, hits, a dense code stream) between them: a row starts
    in a stretch where its entry state shows, the noise is entered from open lanes, and the row's end never merges, so the bands go back to
    row 0 through rows of noise"""
    lo, hi, _ = luma_levels(q)
    y = _noise(4, lo, hi)
    y[:, :130] = lo + _ramp(saw_period(q))[(np.arange(130) - 130) % saw_period(q)]      # (a whole tooth ends at column 129: lane 16 looks back over a ramp, cells 112 .. 127, and walks into the noise)
    y[:, 384:] = _saw(128, saw_period(q), lo)
    return y


CRAFTED = (("P1", p1), ("P2", p2), ("P3", p3), ("P4", p4))


def crafted_lumas(q):
    return [f(q) for _, f in CRAFTED]


def crafted_pictures(q):
    """P1 .. P4 as 512 x 512 x 3 grey pictures at quality q (any quality the colour stage knows)"""
    return np.stack([bgr_of(y, q) for y in crafted_lumas(q)])


def suite_pictures():
    """the pictures the suite's pre-filter and fallback tests run on, by name"""
    from oracle.harness import class_image
    o = _oracle()
    return ([(f"synth({s})", o.synth(s)) for s in (0, 3, 40, 41)] +
            [(f"{k}({s})", class_image(k, s)) for k, s in (("noise", 1), ("blocks", 2), ("tiles", 0), ("gradient", 0), ("flat", 0))])


# ---------------------------------------------------------------------------------------------------------------- the restatement
_STEP = np.array([[(a + ((c + 2) >> 2)) & 15 for c in range(16)] for a in range(16)] + [[0] * 16], np.uint8)   # [|vb| & 15, or 16 for vb == 0][state]


class Census:
    """what pass A does with a luma plane (512 x 512), restated.  Arrays are indexed [row, column] with rows and columns 0 .. 511; only
    1 .. 510 are cells."""

    def __init__(self, luma, q):
        y = np.asarray(luma).reshape(S, S).astype(np.int64)
        self.q = q
        ctr = y[1:-1, 1:-1]
        sm = np.zeros((S, S), np.int64); mg = np.zeros((S, S), np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    d = ctr - y[1 + dy:S - 1 + dy, 1 + dx:S - 1 + dx]
                    sm[1:-1, 1:-1] += d; mg[1:-1, 1:-1] += np.abs(d)
        self.sm = sm
        self.avb = 15 * np.abs(sm) + mg                                  # |vb|; 0 exactly where sm is 0
        self.kind = np.where(sm == 0, 16, self.avb & 15)                 # which row of _STEP a cell applies
        # pre[r, c, s]: the state behind cell c of row r for a row entered in state s (pre[r, 0] is the identity)
        pre = np.empty((S, S - 1, 16), np.uint8)
        pre[:, 0] = np.arange(16, dtype=np.uint8)
        for c in range(1, S - 1):
            pre[:, c] = np.take_along_axis(_STEP[self.kind[:, c]], pre[:, c - 1].astype(np.int64), 1)
        self.pre = pre
        self.entry = np.zeros(S, np.int64)                               # the exact state row r starts from
        for r in range(2, S - 1):
            self.entry[r] = pre[r - 1, S - 2, self.entry[r - 1]]
        self.map = self.row_maps(self.entry)
        # the far lanes' look-back
        lanes = np.arange(FAR0, 64)
        first = 8 * lanes - 16
        cand = np.where((self.kind[:, first] == 16)[:, :, None], 0, (self.kind[:, first][:, :, None] + np.arange(5)) & 15)
        for i in range(1, 16):
            cand = _STEP[self.kind[:, first + i][:, :, None], cand]
        self.merged = np.ones((S, 64), bool)
        self.merged[:, FAR0:] = np.all(cand == cand[:, :, :1], 2)
        self.merged[[0, S - 1]] = True
        self.open = ~self.merged                                         # [row, lane]

    def state_before(self, entry):
        """[row, column]: the state in front of every cell when row r is entered in state entry[r]"""
        st = np.zeros((S, S), np.int64)
        st[:, 1:] = np.take_along_axis(self.pre, np.asarray(entry).reshape(S, 1, 1).astype(np.int64), 2)[:, :, 0]
        return st

    def cells(self, st):
        """map cells from the state in front of each"""
        v = (self.avb + ((st + 2) >> 2)) >> 4
        v = np.where(self.sm == 0, 0, np.where(self.sm < 0, -v, v))
        v[[0, S - 1]] = 0; v[:, [0, S - 1]] = 0
        return v

    def row_maps(self, entry):
        return self.cells(self.state_before(entry))

    # ---- the paths
    def depth(self, b):
        r0 = 1 + RB * b
        rr = r0 - 1
        while rr > 0 and not self.merged[rr, 63]:
            rr -= 1
        return r0 - rr

    def depths(self):
        return [self.depth(b) for b in range(1, NB)]

    def open_rows(self):
        """per row 1 .. 510: (open lanes, separate runs of them, the longest run)"""
        out = []
        for r in range(1, S - 1):
            o = self.open[r].astype(np.int8)
            starts = np.flatnonzero(np.diff(np.concatenate([[0], o])) == 1)
            ends = np.flatnonzero(np.diff(np.concatenate([o, [0]])) == -1)
            out.append((int(o.sum()), len(starts), int((ends - starts + 1).max()) if len(starts) else 0))
        return out

    def marker_rows(self, oracle_map):
        return int(np.count_nonzero(np.any(np.abs(oracle_map.reshape(S, S)) > 6000, 1)))

    # ---- the sensitivity
    def band_entry_changes(self, b):
        """for each of the 15 states a band's first row does NOT start from: the cells of that row that change"""
        r0 = 1 + RB * b
        out = {}
        for s in range(16):
            if s != self.entry[r0]:
                e = self.entry.copy(); e[r0] = s
                out[s] = int(np.count_nonzero(self.row_maps(e)[r0] != self.map[r0]))
        return out

    def far_entry_changes(self, state, only_open=False):
        """every far lane (only_open: every open lane) entered in `state` (an int, or a function of the exact state) instead of its exact state: the
        map cells that change, as a mask"""
        st = self.state_before(self.entry)
        wrong = st.copy()
        lanes = np.arange(FAR0, 64)
        cur = st[:, 8 * lanes]
        cur = np.full_like(cur, state) if np.isscalar(state) else state(cur)
        if only_open:
            cur = np.where(self.open[:, FAR0:], cur, st[:, 8 * lanes])
        for e in range(8):
            c = 8 * lanes + e
            wrong[:, c] = cur
            cur = _STEP[self.kind[:, c], cur]
        ch = self.cells(wrong) != self.map
        ch[:, S - 1] = False
        return ch

    def summary(self):
        rows = self.open_rows()
        return dict(depths=self.depths(), open_min=min(r[0] for r in rows), open_max=max(r[0] for r in rows), runs_min=min(r[1] for r in rows),
                    longest_min=min(r[2] for r in rows), longest_max=max(r[2] for r in rows),
                    far0=int(self.far_entry_changes(0).sum()), far_other=int(self.far_entry_changes(lambda s: (s + 8) & 15).sum()),
                    open0=int(self.far_entry_changes(0, True).sum()), open_other=int(self.far_entry_changes(lambda s: (s + 8) & 15, True).sum()))


def map_agrees(census, oracle_map):
    """the restated map against the oracle's pass A, cell for cell: equal, or what the marker rule makes of that value (+-20000 for a value just
    above the threshold, 7000 for threshold + 21 or, written by the cell on its right, + 22, and the bump of - threshold by one, three times
    a picture at the most).  -> the number of cells the rule rewrote"""
    o = np.asarray(oracle_map).reshape(S, S).astype(np.int64)
    v, s2 = census.map, sharp2(census.q)
    diff = o != v
    diff[[0, S - 1]] = False; diff[:, [0, S - 1]] = False
    ok = (((o == 20000) & (v > s2) & (v <= s2 + 20)) | ((o == -20000) & (-v > s2) & (-v <= s2 + 20)) |
          ((o == 7000) & ((v == s2 + 21) | (v == s2 + 22))))
    bump = ((o == -s2 - 1) | (o == -20000)) & (v == -s2)                 # (a bumped cell is just above the threshold: the rule may mark it too)
    bad = diff & ~ok & ~bump
    assert not bad.any(), f"q{census.q}: {int(bad.sum())} cells of the restated map differ from the oracle's pass A, first {np.argwhere(bad)[:4].tolist()}"
    assert int((diff & bump).sum()) <= 3
    return int(diff.sum())


# ---------------------------------------------------------------------------------------------------------------- the oracle's planes
@functools.lru_cache(maxsize=None)
def oracle_side():
    """tests/low_machine/oracle_side.c as a shared library of this process's own (it opens up oracle/nhwo_prelow.c)"""
    odir = os.path.join(ROOT, "oracle")
    if not os.path.exists(os.path.join(odir, "liboracle.so")):
        subprocess.check_call(["make", "-s", "-C", odir])
    so = os.path.join(tempfile.mkdtemp(prefix="nhw_oracle_side"), "oracle_side.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "low_machine", "oracle_side.c"),
                           "-L" + odir, "-l:liboracle.so", "-Wl,-rpath," + odir])
    L = ctypes.CDLL(so)
    L.lm_contrast_map.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.lm_prefilter_planes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return L


def oracle_pass_a(luma, q):
    """the oracle's contrast map behind pass A alone (int16, flat)"""
    src = np.ascontiguousarray(np.asarray(luma).reshape(-1), np.int16)
    km = np.zeros(S * S, np.int16)
    oracle_side().lm_contrast_map(src.ctypes.data, km.ctypes.data, q)
    return km


def oracle_planes(luma, q):
    """the oracle's pre-filter on a luma plane -> (filtered picture, contrast map, flag plane) behind its last pass, flat"""
    y = np.ascontiguousarray(np.asarray(luma).reshape(-1), np.int16).copy()
    km = np.zeros(S * S, np.int16); so = np.zeros(S * S, np.uint8)
    oracle_side().lm_prefilter_planes(y.ctypes.data, km.ctypes.data, so.ctypes.data, q)
    return y, km, so
