"""Crafted planes for the luma residual passes Y19 .. Y27 (tests/test_residual_stage.py): the inputs of nhw_stage_residuals
(include/nhw_hip_debug.h) and of the oracle's nhwo_residual_stage (oracle/nhwo.h).  A support module: seeded builders, no tests.

The value domain is what an 8-bit picture can put into the planes at this point of the encode; outside it the kernels make no promise
(residuals_fused_par keeps the cells of the code plane as bytes because |LL1| < 500, nhwcodec_amd/csrc/nhw_tail_par.h):

  * LL1 cells (B_LL1) and the first-order samples (B_JPEG's LL quadrant, B_FIRST) lie in -480 .. 480;
  * the reconstruction (B_PROC's LL quadrant) is LL1 plus a residual in -16 .. 16;
  * the level-1 details (the other three quadrants of B_PROC) lie in -520 .. 520;
  * the level-2 block (B_L2SAVE): LL2 samples 0 .. 8000 untagged or 16000 .. 16255 tagged, level-2 details in -1040 .. 1040;
  * a code plane (the input of Y24 and Y25 alone) holds 0 or a code that the quality's Y23 can leave (codes_of).

check_domain asserts all of it on every plane a builder returns.

Coordinates: a residual cell (r, j) of the 256 x 256 LL quadrant is walked by Y22 down its column j; its LH1 partner is the coefficient
(j, 256 + r) of the work plane, i.e. lh[j, r] of the band here, and "the one before" is lh[j, r - 1] (for r = 0: the reconstruction
sample (j, 255)).  Bands are 256 x 256 arrays in band-local coordinates: lh = plane[:256, 256:], hl = plane[256:, :256], hh = plane[256:, 256:].
"""
import numpy as np

Q = 65536
H = 256
N_PLANES = 8
# the LH1 partner values on both sides of every nudge's test (nudge_up_small .. mark_m_large, code_residuals: oracle/nhwo_luma.c) and the
# values of the coefficient before it
PARTNERS = np.array([-24, -23, -16, -15, -10, -9, -8, -7, -6, 0, 6, 7, 8, 9, 10, 15, 16, 23, 24, 32], np.int16)
BEFORE = np.arange(-9, 10, dtype=np.int16)
# the rows on either side of a wavefront's 64-row range in Y27 (clean_details_seq): LH1 rows, and rows of the lower half (band-local: - 256)
WAVE_ROWS_LH = (64, 65, 128, 129, 192, 193)
WAVE_ROWS_LOW = (319, 320, 383, 384, 447, 448)


def codes_of(q):
    """the codes Y23 can leave in the code plane at quality q (code_residuals and the marks of classify_residuals)"""
    c = [140, 141, 123, 124, 125, 126]
    if q >= 19: c += [121, 122]
    if q >= 21: c += [144, 145, 148, 149]
    return sorted(c)


class Planes:
    """the five planes of one image in front of Y19"""

    def __init__(self, seed):
        self.rng = rng = np.random.default_rng(seed)
        self.ll1 = rng.integers(-480, 481, (H, H)).astype(np.int16)
        self.res = np.zeros((H, H), np.int16)
        self.lh = np.zeros((H, H), np.int16); self.hl = np.zeros((H, H), np.int16); self.hh = np.zeros((H, H), np.int16)
        self.l2 = level2_block(rng)
        self.first = rng.integers(-480, 481, (H, H)).astype(np.int16)      # the first-order samples Y19 copies (quality > 21)
        self.notes = []
        self.first_stale = rng.integers(-480, 481, (H, H)).astype(np.int16)  # what B_FIRST holds before: Y19 overwrites it, below quality 22 nothing reads it

    def arrays(self):
        """-> {jpeg [512,512], proc [512,512], ll1, l2save, first_order [256,256]} as int16, the domain asserted"""
        jpeg = np.zeros((512, 512), np.int16)
        jpeg[:H, :H] = self.first
        proc = np.zeros((512, 512), np.int16)
        proc[:H, :H] = self.ll1 + self.res
        proc[:H, H:] = self.lh; proc[H:, :H] = self.hl; proc[H:, H:] = self.hh
        a = dict(jpeg=jpeg, proc=proc, ll1=self.ll1.copy(), l2save=self.l2.copy(), first_order=self.first_stale.copy())
        check_domain(a)
        return a


def check_domain(a, code_plane_q=None):
    """the module docstring's domain on one image's planes (code_plane_q: ll1 is a code plane of that quality)"""
    jpeg, proc, ll1, l2, first = (np.asarray(a[k], np.int32).reshape(s) for k, s in
                                  (("jpeg", (512, 512)), ("proc", (512, 512)), ("ll1", (H, H)), ("l2save", (H, H)), ("first_order", (H, H))))
    assert np.abs(jpeg[:H, :H]).max() <= 480 and np.abs(first).max() <= 480, "first-order samples outside -480 .. 480"
    if code_plane_q is None:
        assert np.abs(ll1).max() <= 480, "LL1 outside -480 .. 480"
        assert np.abs(proc[:H, :H] - ll1).max() <= 16, "residual outside -16 .. 16"
    else:
        assert np.isin(ll1, [0] + codes_of(code_plane_q)).all(), "a code the quality's Y23 cannot leave"
    for name, band in (("LH1", proc[:H, H:]), ("HL1", proc[H:, :H]), ("HH1", proc[H:, H:])):
        assert np.abs(band).max() <= 520, f"{name} outside -520 .. 520"
    ll2 = l2[:128, :128]
    assert (((ll2 >= 0) & (ll2 <= 8000)) | ((ll2 >= 16000) & (ll2 <= 16255))).all(), "LL2 neither untagged (0 .. 8000) nor tagged (16000 .. 16255)"
    d2 = l2.copy(); d2[:128, :128] = 0
    assert np.abs(d2).max() <= 1040, "level-2 details outside -1040 .. 1040"


# ---------------------------------------------------------------------------------------------- pieces
def level2_block(rng):
    """the level-2 block as l2save holds it: LL2 samples up to 8000 with a tagged patch and cells on both sides of Y26's 8000, small details
    (Y20's parents below quality 14), a last row of loud and quiet cells over HL1's first row"""
    b = rng.choice(np.array([0, 0, 0, 1, -2, 3, -4, 5, -6, 7, -8, 9, -11, 12, 16, -20, 40, -300, 1040], np.int16), (H, H))
    b[:128, :128] = rng.integers(0, 256, (128, 128))
    b[10:14, 100:128] += np.int16(16000)
    b[20:28, 126] = (7999, 8000, 16000, 16007, 5, 6, 0, 255)
    b[255] = rng.choice(np.array([0, 0, 3, -5, 6, -6, 8, -9, 20, -40], np.int16), H)
    return b.astype(np.int16)


def sign_patches(rng, shape, w=8, h=1):
    """+-1 in patches of w columns and h rows: runs need neighbours of one sign"""
    s = np.where(rng.random((-(-shape[0] // h), -(-shape[1] // w))) < 0.5, -1, 1)
    return np.repeat(np.repeat(s, h, 0), w, 1)[:shape[0], :shape[1]].astype(np.int16)


def noise_residuals(rng, p_big, big=(4, 5, 6, 7, 8, 9, 10, 12, 16), small=(0, 0, 1, 1, 2, 2, 3, 3)):
    """dense, small, in patches of one sign; p_big: the share of cells from `big`"""
    m = np.where(rng.random((H, H)) < p_big, rng.choice(np.array(big, np.int16), (H, H)), rng.choice(np.array(small, np.int16), (H, H)))
    return (m * sign_patches(rng, (H, H), 8, 4)).astype(np.int16)


def detail_noise(rng, kind, loud=0.08):
    """a 256 x 256 band.  "partners": even columns from PARTNERS, odd ones from BEFORE (a band for Y22 / Y23's nudges); "runs": +-3 .. 9 in
    patches of one sign (Y21); "clean": |v| in 5 .. 11 and 14 .. 17 among zeros and +-6 (Y27); "low": what Y20 thins below quality 16,
    with the given share of cells of magnitude 12 and up (the pass counts them)"""
    if kind == "partners":
        b = rng.choice(BEFORE, (H, H))
        b[:, 0::2] = rng.choice(PARTNERS, (H, H // 2))
        return b.astype(np.int16)
    if kind == "runs":
        m = rng.choice(np.array([0, 0, 3, 4, 5, 6, 7, 8, 8, 9, 12], np.int16), (H, H), p=np.array([10, 8, 4, 10, 14, 14, 14, 8, 6, 2, 2]) / 92)
        return (m * sign_patches(rng, (H, H), 8, 1)).astype(np.int16)
    if kind == "clean":
        vals = np.array([0, 3, 5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 17, 24, 32], np.int16)
        p = np.array([30, 3, 5, 14, 9, 9, 7, 4, 3, 2, 3, 4, 2, 2, 3], float)
        m = rng.choice(vals, (H, H), p=p / p.sum())
        return (m * np.where(rng.random((H, H)) < 0.5, -1, 1)).astype(np.int16)
    assert kind == "low"
    m = rng.integers(0, 12, (H, H))
    m = np.where(rng.random((H, H)) < 0.45, 0, m)
    m = np.where(rng.random((H, H)) < loud, rng.integers(12, 41, (H, H)), m)
    return (m * np.where(rng.random((H, H)) < 0.5, -1, 1)).astype(np.int16)


def put_runs(band, rng, rows):
    """Y21: in each of `rows`, runs of +-4 .. 7 of lengths 2 .. 9 one after another, +-8 pairs, +-8 beside +-6 / +-7; the first starts at
    column 1, 2, 3 or 4 in turn (a lane has four cells: every residue of the start), the last run is cut at column 254"""
    for i, r in enumerate(rows):
        row = np.zeros(H, np.int16)
        c = 1 + i % 4
        k = i
        while c < 255:
            sign = -1 if (k >> 1) & 1 else 1
            kind = k % 7
            if kind < 4:
                n = 2 + (k * 5 + i) % 8
                seq = [sign * (4 + (k + t) % 4) for t in range(n)]
            elif kind == 4: seq = [8 * sign, 8 * sign]
            elif kind == 5: seq = [(6 + (k >> 3 & 1)) * sign, 8 * sign, 8 * sign, 3 * sign]
            else: seq = [8 * sign, (6 + (k >> 3 & 1)) * sign, 0, 8 * sign, 5 * sign, 5 * sign, 5 * sign]
            seq = seq[:255 - c]
            row[c:c + len(seq)] = seq
            c += len(seq) + (k * 3 + i) % 3                           # now and then no gap: a run meets the next
            k += 1
        band[r] = row


def put_ripples(band, rng, rows, to_col=255):
    """Y27's ripple in each of `rows`: an 8 (16, 24, 9 on its 1 modulo 8) in front of a run of 9s longer than a lane's four cells -- every cell
    of the run moves --, -7 beside 8, -16 / -15 / -17 / -24 behind a -8 or -9 with the cell after next on either side of 0; the last chain
    ends in column to_col (HL1: 255, from where it reaches column 256)"""
    for i, r in enumerate(rows):
        row = band[r].copy()
        c = 1 + i % 5
        k = i
        while c < to_col - 14:
            kind = k % 6
            if kind == 0: seq = [8] + [9] * (5 + k % 9)
            elif kind == 1: seq = [(16, 24, 9, 17)[k // 6 % 4], 9, 9, 9, 9, 9, 8, 0]
            elif kind == 2: seq = [-7, 8, 0, 8, -7, 0]
            elif kind == 3: seq = [(-8, -9, -16)[k // 6 % 3], (-16, -15, -17, -24, -23)[k // 6 % 5], (-1, 0, 1)[k // 6 % 3], 0]
            elif kind == 4: seq = [-8, -16, -16, -24, 1, 0]
            else: seq = [8, 8, 8, 8, 8, 8, 0, 7, 8, 7]
            row[c:c + len(seq)] = seq
            c += len(seq) + k % 3
            k += 1
        tail = ([8] + [9] * 9) if i % 3 == 0 else ([-8, -16, 0] if i % 3 == 1 else [0, 8, 9])
        row[to_col + 1 - len(tail):to_col + 1] = tail
        band[r] = row


# Y27's ripple looks two cells ahead only up to a band's last looking column: 253 in band-local columns in all three bands (ripple(v, j < W - 2) in
# LH1 and HH1, j < H - 2 in HL1: oracle/nhwo_luma.c).  The rows of put_look_edge: the first and last row of every wavefront's range, and lone rows
EDGE_ROWS_LH = (1, 64, 65, 128, 129, 192, 193, 254)
EDGE_ROWS_LOW = (0, 63, 64, 127, 128, 191, 192, 254)
LONE_ROWS = (33, 97, 161, 225)
LAST_LOOK = 253


def put_look_edge(pl, look_at_edges, low=False):
    """The bound of the ripple's look two ahead, in all three bands: a chain (v0, v1, v2) with v0 on 0 / 1 modulo 8 below -7, v1 below -14 on 0 / 1
    modulo 8 (so that only the look decides) -- at the last looking column with v2 in {0, -1, 1}: v1 moves for v2 <= 0 and stays for v2 = 1 --, and one
    column further, where the look is forbidden, with v2 <= 0: v1 stays although a look would move it.  There v2 lies behind the band: LH1's is
    the next row's first cell of the level-2 quadrant (both what the reconstruction and what l2save hold there are <= 0), HL1's is HH1's
    column 256, HH1's the next row's first HL1 cell.  look_at_edges: the edge rows get the looking placement and the lone rows the forbidden one,
    or the other way round (the two overlap, so a row has one).  v0 is -16, -9 (HH1: -24), -40, -48 in turn in the edge rows -- -40 and -48
    stand through every quality's Y20 -- and -8 between four loud neighbours in the lone rows; v1 is -16, -24, -40, -17 in turn.  low (the set of the
    qualities below 16, whose Y20 thins magnitudes up to 34): -40, -48, -41, -56 for both in every row.
    -> [(band, row, column of v1, looks, v2)] in band-local coordinates"""
    notes = []
    for name, band in (("lh", pl.lh), ("hl", pl.hl), ("hh", pl.hh)):
        edge = EDGE_ROWS_LH if name == "lh" else EDGE_ROWS_LOW
        for i, r in enumerate(edge + LONE_ROWS):
            lone = r in LONE_ROWS
            look = look_at_edges != lone
            c = LAST_LOOK if look else LAST_LOOK + 1
            v0 = -8 if lone else ((-16, -24, -40, -48) if name == "hh" else (-16, -9, -40, -48))[i % 4]
            v1 = (-16, -24, -40, -17)[(i + i // 4) % 4]
            if low: v0, v1 = (-40, -48, -41, -56)[i % 4], (-48, -41, -56, -40)[(i + i // 4) % 4]
            v2 = (0, -1, 1)[i % 3] if look else (0, -1)[i % 2]
            band[r, c - 1], band[r, c], band[r, c + 1] = 16, v0, v1
            if lone: band[r - 1, c] = band[r + 1, c] = 16
            if c + 2 < H: band[r, c + 2] = v2
            elif name == "lh":
                pl.ll1[r + 1, 0], pl.res[r + 1, 0] = -100 + v2, 0
                pl.l2[r + 1, 0] = 0 if r + 1 < 128 else v2
            elif name == "hl": pl.hh[r, 0] = v2
            else: pl.hl[r + 1, 0] = v2
            notes.append((name, r, c + 1, look, v2))
    return notes


def triple_of(t):
    """the t-th (res, a, d2) of [-9, 9]^3, t < 6859; beyond: zeros"""
    if t >= 6859: return 0, 0, 0
    return t // 361 - 9, t // 19 % 19 - 9, t % 19 - 9


def put_triples(pl, first_row, variant):
    """every (res, a, d2) of [-9, 9]^3 down a column at a pitch of four rows, a zero residual in the fourth: 27 groups of rows from first_row on,
    256 columns.  A group whose third row is row 256 has its d2 in HL1's first row (LL1 reads as zero there)."""
    t = (np.arange(27 * H) * 37 + 101 * variant) % (27 * H)         # (37 is prime to 6912: every triple once)
    tr = np.array([triple_of(int(x)) for x in t], np.int16).reshape(27, H, 3)
    for g in range(27):
        r = first_row + 4 * g
        for k in range(3):
            if r + k < H: pl.res[r + k] = tr[g, :, k]
            elif r + k == H: pl.hl[0] = tr[g, :, k]
        if r + 3 < H: pl.res[r + 3] = 0


def put_look_further(pl, first_row, first_col, rows_of_groups, end_col=H):
    """the arms that look at the column on the right -- (res, a) in {2, 3}^2 with d2 in {0, 1}, and the mirrored negatives with d2 = 0, against every
    (x0, x1, x2) of {1 .. 4}^2 x {-1, 0, 1} -- and at the row above: res = +-1, a = +-3, d2 = +-2 over a row above of -1, 0, 1.  Groups of five rows
    (the row above, the three, a zero row) from first_row on, pairs of columns from first_col up to end_col."""
    cases = []
    for res in (2, 3):
        for a in (2, 3):
            for d2 in (0, 1):
                cases += [((res, a, d2), (x0, x1, x2)) for x0 in (1, 2, 3, 4) for x1 in (1, 2, 3, 4) for x2 in (-1, 0, 1)]
            cases += [((-res, -a, 0), (-x0, -x1, -x2)) for x0 in (1, 2, 3, 4) for x1 in (1, 2, 3, 4) for x2 in (-1, 0, 1)]
    above = [((s, 3 * s, 2 * s), u) for s in (1, -1) for u in (-1, 0, 1)]
    n_pairs = (end_col - first_col) // 2
    k = 0
    for g in range(rows_of_groups):
        r = first_row + 5 * g
        if r + 2 > H: break
        for m in range(n_pairs):
            j = first_col + 2 * m
            if (k + g) % 9 == 8:
                (tri, u) = above[(k // 9) % len(above)]
                if r > 0: pl.res[r - 1, j] = u
                right = (0, 0, 0)
            else:
                tri, right = cases[k % len(cases)]
            for i in range(3):
                if r + i < H: pl.res[r + i, j] = tri[i]; pl.res[r + i, j + 1] = right[i]
                elif r + i == H: pl.hl[0, j] = tri[i]; pl.hl[0, j + 1] = right[i]
            if r + 3 < H: pl.res[r + 3, j:j + 2] = 0
            k += 1


def put_column_255(pl, rng):
    """The reference visits column 255 last, and the GPU's prologue rebuilds what that order means (residuals_fused_par):
      * column 255's "column on the right" at row x is LH1's first column (x, 256) AS COLUMN x's STEP 0 LEFT IT minus column 0's LL1 cell (x + 1, 0)
        AS COLUMN 0's WHOLE WALK LEFT IT;
      * every column's Y22 starts from the sample (j, 255) before column 255's visit, its Y23 from the sample after it.
    Groups of four rows down column 255: a look-further triple ((res, a) in {2, 3}^2, d2 in {0, 1}; the negatives with d2 = 0) whose three
    neighbour values are set through LL1's column 0 -- kind 0: they pass; kind 1: they pass on the cells as they were, but column 0's own walk
    has marked one of the three cells (a code there: the test fails); kind 2: they pass only because step 0 of columns x and x + 1 nudges the
    coefficients 7 and 8 to 9 and 10; kind 3: one of them is off.  LL1's column 255 is 2 or 3, so that the sample (j, 255) -- "the coefficient
    before" of every column's first step -- lies at the nudges' thresholds and moves across them when column 255 marks."""
    ll1, res, lh = pl.ll1, pl.res, pl.lh
    ll1[:, 255] = rng.integers(2, 4, H)
    res[0:2, 129:] = 0                                               # columns 129 ..: steps 0 and 1 see no residual, so step 0 only nudges
    res[:, 0] = 0
    sign = np.ones(H, np.int16)
    for m in range(H // 4):
        r, kind = 4 * m, m % 4
        s_ = -1 if (m // 4) % 3 == 2 else 1
        if kind == 2: s_ = 1
        sign[r:r + 4] = s_
        tri = (int(rng.integers(2, 4)), int(rng.integers(2, 4)), int(rng.integers(0, 2)) if s_ > 0 else 0)
        res[r:r + 3, 255] = s_ * np.array(tri, np.int16); res[r + 3, 255] = 0
        x = [s_ * int(rng.integers(2, 4)), s_ * int(rng.integers(2, 4)), s_]
        part = [int(v) for v in rng.choice(PARTNERS, 3)]
        if kind == 2 and r >= 132:
            part[0], part[1] = 7, 8
            x[0] -= 2; x[1] -= 2                                     # 0 or 1 before the nudge, 2 or 3 behind it
        elif kind == 3:
            x[int(rng.integers(0, 3))] = 0
        for dr in range(3):
            lh[r + dr, 0] = part[dr]
            if r + dr + 1 < H: ll1[r + dr + 1, 0] = part[dr] - x[dr]
        if kind == 1:
            o = 1 + (m // 4) % 3                                      # (3, 3, 3) from row r + o on: column 0 marks the cell (r + o, 0)
            res[r + o:min(r + o + 3, H), 0] = 3
    res[:, 254] = sign * rng.choice(np.array([2, 3, 0], np.int16), H)  # column 254 looks at column 255 as it was


def put_row_256(pl, rng):
    """Y22's last step, row 254, reaches row 256: a mark there rewrites HL1's first row (and column 255's does so from the prologue's walk).  In
    three columns of four a marking triple whose d2 -- HL1's first row -- is loud enough for Y27 to keep, so that the mark's step of 2 shows behind
    Y27: (2, 2, 7 .. 9) and (-2 | -3, -2 | -3, -9 .. -6); random triples in the others (column 255 marks).  Rows 252, 253 carry no residual: the triple is what row 254 sees."""
    pl.res[252:254] = 0
    for j in range(H):
        if j % 4 == 3 and j != H - 1: t = rng.integers(-9, 10, 3)
        elif (j // 4) % 2: t = (2, 2, int(rng.integers(7, 10)))
        else: t = (-int(rng.integers(2, 4)), -int(rng.integers(2, 4)), -int(rng.integers(6, 10)))
        pl.res[254, j], pl.res[255, j], pl.hl[0, j] = t


def put_q18_chains(pl, rng, cols):
    """quality 18: steps that write 14100 / 14000 into the cell below (res 3 or 4 over a = 5, res 3 over a = 4; the negatives), the next step
    starting from that cell -- residuals of one sign from {3, 4, 5} (now and then 7, 8: the snaps) down whole columns"""
    for i, j in enumerate(cols):
        s = sign_patches(rng, (H, 1), 1, 16 + i % 5)[:, 0]
        pl.res[:, j] = s * rng.choice(np.array([3, 4, 5, 3, 5, 4, 5, 7, 8, 0], np.int16), H)


# ---------------------------------------------------------------------------------------------- the crafted set
def crafted(variant, low=False):
    """plane `variant` (0 .. N_PLANES - 1) of the crafted set -> Planes.  low: the details are what Y20 thins below quality 16 (the set of
    qualities 7, 12 and 13 .. 15), with a loud count on each side of its three thresholds over the variants.
      0  every triple from row 0 on (rows 0, 1, 2 are the first group), partner bands, noise residuals below
      1  every triple in groups that end in rows 253, 254, 255; the same from row 1 on
      2  the look-further arms from row 0 and up to rows 253 / 254 (d2 in row 256), from column 0 and from column 1 (pairs 253 | 254 and
         254 | 255), column 255's walk (put_column_255)
      3  quality 18's chains, marking triples in rows 254, 255, 256 (put_row_256), big residuals over four tenths of the plane: more than 20 000 raw entries in the first list
      4  Y21's runs in LH1 and HL1 (rows 1 and 254, columns 1 and 254 of each band included), Y27's ripples under them
      5  Y27: dense bands, ripples in the rows on either side of every wavefront's range and into column 256, HL1's first row; the ripple's look two
         ahead at the last looking column in the first and last row of every wavefront's range, one column further in lone rows (put_look_edge)
      6  noise residuals, partner bands, runs and ripples mixed, the look-further arms in row 1; put_look_edge the other way round
      7  sparse: few residuals, quiet bands"""
    pl = Planes(7300 + 17 * variant + (1000 if low else 0))
    rng = pl.rng
    v = variant
    loud = (0.16, 0.087, 0.066, 0.03, 0.16, 0.087, 0.066, 0.03)[v]
    if v in (0, 1, 2, 3, 6):
        pl.res[:] = noise_residuals(rng, 0.12)
        pl.lh[:] = detail_noise(rng, "partners")
        pl.hl[:] = detail_noise(rng, "low", loud) if low else detail_noise(rng, "clean")
        pl.hh[:] = detail_noise(rng, "low", loud) if low else detail_noise(rng, "runs")
        pl.hl[0] = rng.integers(-9, 10, H)
    if v == 0:
        put_triples(pl, 0, 0)
    elif v == 1:
        pl.res[:] = noise_residuals(rng, 0.05)
        put_triples(pl, 1, 1)
        put_triples(pl, 149, 2)                                       # groups at rows 149 .. 253: the last one's d2 is row 255
    elif v == 2:
        put_look_further(pl, 0, 1, 1, 129)                            # a group in row 0 (no row above), pairs from column 1
        put_look_further(pl, 6, 0, 12)
        put_look_further(pl, 70, 1, 10)                               # .. pairs 1 | 2 to 253 | 254
        put_look_further(pl, 254 - 5 * 11, 0, 12, 128)                # the last group in rows 254, 255, 256
        put_look_further(pl, 253 - 5 * 9, 129, 10)                    # .. and in rows 253, 254, 255
        put_column_255(pl, rng)
    elif v == 3:
        pl.res[:] = (np.where(rng.random((H, H)) < 0.34, rng.integers(9, 17, (H, H)), rng.integers(0, 2, (H, H))) * sign_patches(rng, (H, H), 4, 2)).astype(np.int16)
        put_q18_chains(pl, rng, list(range(3, 250, 9)) + [0, 1, 254, 255])
        put_row_256(pl, rng)
    elif v == 4:
        pl.res[:] = noise_residuals(rng, 0.1)
        for band in (pl.lh, pl.hl, pl.hh):
            band[:] = detail_noise(rng, "low", loud) if low else detail_noise(rng, "runs")
        rows = [1, 2, 253, 254] + list(range(5, 250, 3))
        put_runs(pl.lh, rng, rows); put_runs(pl.hl, rng, rows)
        put_ripples(pl.hh, rng, range(4, 250, 6), 254)
    elif v == 5:
        pl.res[:] = noise_residuals(rng, 0.08)
        for band in (pl.lh, pl.hl, pl.hh):
            band[:] = detail_noise(rng, "low", loud) if low else detail_noise(rng, "clean")
        lh_rows = sorted(set(WAVE_ROWS_LH) | {1, 254} | set(range(10, 250, 7)))
        low_rows = sorted({r - H for r in WAVE_ROWS_LOW} | {0, 1, 254} | set(range(9, 250, 7)))
        put_ripples(pl.lh, rng, lh_rows, 254)
        put_ripples(pl.hl, rng, low_rows, 255)                        # HL1's last chain ends in column 255 and reaches column 256
        put_ripples(pl.hh, rng, low_rows, 254)
        pl.hh[:, 0] = rng.choice(np.array([9, 9, 8, 10, -16, -15, -17, 16, 0], np.int16), H)   # column 256: what HL1's ripple out of column 255 meets
        pl.hl[0, 1:] = rng.choice(np.array([6, 7, 8, -6, -7, -8, 9, 0], np.int16), H - 1)      # HL1's first row under the level-2 block's row 255
        pl.notes = put_look_edge(pl, True, low)
    elif v == 6:
        put_look_further(pl, 1, 0, 1)                                 # a group in row 1 under a row above; the last pair is 254 | 255
        rows = list(range(3, 250, 5))
        put_runs(pl.hh, rng, rows)
        put_ripples(pl.hl, rng, range(2, 250, 4), 255)
        put_q18_chains(pl, rng, range(5, 250, 31))
        pl.notes = put_look_edge(pl, False, low)
    elif v == 7:
        pl.res[:] = np.where(rng.random((H, H)) < 0.02, rng.integers(-16, 17, (H, H)), 0)
        for band in (pl.lh, pl.hl, pl.hh):
            band[:] = np.where(rng.random((H, H)) < 0.05, detail_noise(rng, "low" if low else "clean", loud), 0)
    return pl


_cache = {}


def crafted_set(low=False):
    """the N_PLANES crafted images as dicts of arrays (Planes.arrays), made once: nobody changes them"""
    if low not in _cache:
        made = [crafted(v, low) for v in range(N_PLANES)]
        _cache[low] = [pl.arrays() for pl in made]
        _cache["notes", low] = [pl.notes for pl in made]
        for a in _cache[low]:
            for x in a.values(): x.setflags(write=False)
    return _cache[low]


def set_for(q):
    return crafted_set(low=q < 16)


def look_edge_notes(q):
    """per plane of quality q's set what put_look_edge placed"""
    set_for(q)
    return _cache["notes", q < 16]


# ---------------------------------------------------------------------------------------------- code planes (Y24 and Y25 alone)
def code_plane(q, variant):
    """a code plane for Y24 and Y25 alone (nhw_stage_residuals form 2, the oracle's part 1) at quality q, of the codes codes_of(q) -> int16 [256, 256].
      rows 0 .. 35     in turn: a code in every column 0 .. 253, an empty row, codes only in columns 252 / 253
      rows 36 .. 99    few entries a row at random columns: the marker between two rows is pruned when the row's last entry lies right of the
                       next row's first one, and kept otherwise
      rows 100 .. 163  entries at column steps of 14 .. 17 and 30 .. 33 (the halved index steps 7 | 8 and 15 | 16 of the fusing rule), and runs of
                       consecutive columns of 100 .. 253 entries from an even or an odd column on: fusing entries by the hundred, ending on either parity
      rows 164 .. 249  121 .. 126 (the quality's) stacked in consecutive rows and columns: a first-order cell takes two and three contributions
      rows 250 .. 255  the same in the last rows, whose second and third contributions fall into the next column of the first-order plane
    and then codes of the first list are taken out of rows 0 .. 35 until their number is (variant % 3) - 1 modulo 256 -- the lists' totals around
    the multiples of 8 of the bit and word groups and of the 256 entries of a thread's chunk."""
    rng = np.random.default_rng(8800 + 100 * q + variant)
    codes = np.array(codes_of(q), np.int16)
    first = np.array([c for c in codes_of(q) if c in (140, 141, 125, 126, 148, 149)], np.int16)
    stack = np.array([c for c in codes_of(q) if 121 <= c <= 126], np.int16)
    p = np.zeros((H, H), np.int16)
    for r in range(36):
        kind = (r + variant) % 3
        if kind == 0: p[r, :254] = rng.choice(codes if r % 2 else first, 254)
        elif kind == 2: p[r, 252:254] = rng.choice(codes, 2)
    for r in range(36, 100):
        n = 1 + (r + variant) % 3
        cols = np.sort(rng.choice(254, n, replace=False))
        if r % 5 == 0: cols = np.array([0, 253])[:n]
        p[r, cols] = rng.choice(codes, len(cols))
    for r in range(100, 164):
        kind = (r + variant) % 4
        if kind < 2:
            steps = (14, 15, 16, 17) if kind == 0 else (30, 31, 32, 33)
            c = (r + variant) % 7
            k = r
            while c < 254:
                p[r, c] = codes[k % len(codes)]
                c += steps[k % 4]; k += 1
        else:
            n = 100 + (37 * r + 11 * variant) % 154
            c0 = (r * 3 + variant) % (254 - n + 1)
            p[r, c0:c0 + n] = rng.choice(first if kind == 2 else codes, n)
    dense = rng.random((H, H)) < (0.5 if variant % 2 else 0.8)
    p[164:, :] = np.where(dense[164:, :], rng.choice(stack, (H - 164, H)), 0)
    p[164:250, 120:] = np.where(rng.random((86, 136)) < 0.1, rng.choice(codes, (86, 136)), 0)
    p[:, 254:] = rng.choice(codes, (H, 2))                            # columns 254, 255 take no part: Y25 clears them, Y24 stops in front of them
    # the first list's total
    want = (variant % 3) - 1
    is_first = np.isin(p[:, :254], first)
    extra = (int(is_first.sum()) - want) % 256
    at = np.argwhere(is_first[:36])
    assert len(at) >= extra
    for r, c in at[rng.choice(len(at), extra, replace=False)]: p[r, c] = 0
    assert (int(np.isin(p[:, :254], first).sum()) - want) % 256 == 0
    return p


def code_set(q):
    """the inputs of Y24 and Y25 alone at quality q: the crafted set's planes with a code plane in place of LL1 (and B_FIRST as Y19 would have
    left it: the first-order samples)"""
    key = ("code", q)
    if key not in _cache:
        out = []
        for v, a in enumerate(crafted_set(False)):
            b = {k: x.copy() for k, x in a.items()}
            b["ll1"] = code_plane(q, v)
            b["first_order"] = b["jpeg"][:H, :H].copy()
            check_domain(b, code_plane_q=q)
            for x in b.values(): x.setflags(write=False)
            out.append(b)
        _cache[key] = out
    return _cache[key]
