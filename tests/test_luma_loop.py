"""The luma plane's first closed loop as production launches it (k_l2_recon<true>: synthesis, Y8, Y9 and the second level-2 analysis with Y13's
copy on one LDS residency of the block) against the staged kernels it replaces, plane by plane and cell by cell, and the files against the oracle.

What is compared, for every image of every case, behind nhw_stage_luma_loop (include/nhw_hip_debug.h) with the same bytes written into the planes
before each form (nhw_debug_write):
  * B_L2SAVE, the whole of B_PROC and of B_JPEG (the level-2 block AND every cell outside it: the fused kernel must not touch those -- the block of
    B_JPEG is still stored by the fused kernel, so nothing is left out of the comparison), B_LL1 with the cell behind it;
  * form 0 (production launches, first analysis to second) against form 3 (the staged kernels), on the planes a whole batch left;
  * form 1 (the fused kernel alone) against form 2 (synthesis, Y8 + Y9, analysis + copy) on planes aimed at the constants of precomp_pick / big_step
    (threshold_planes); form 0 against form 3 on low-amplitude LL1 blocks whose level-2 details sit at 2 .. 4 along the block's borders;
  * the files of whole production batches with the oracle's.
The CPU part walks ana_row_quad's lane arrangement (four cells a lane) against the line filter it stands for."""
import numpy as np
import pytest

from tests.enc_stages import B_LL1, N_IMAGES, Q, Hook, compare, oracle_files, synthetic_images

QUALITIES = (7, 10, 12, 13, 14, 16, 17, 18, 20, 21, 22, 23)
PATTERN = (-4, -3, 4, 3)    # a row of these differences hands a change of the incoming step on from cell to cell to its end (asserted below)


# ---------------------------------------------------------------------------------------------- the rules, as the reference states them
def big_step(d):
    for lim, s in ((11, 7), (7, 4), (5, 2), (4, 1)):
        if d > lim:
            return -s
        if d < -lim:
            return s
    return 0


def precomp_right(dn):
    return dn + big_step(dn) if abs(dn) > 4 else dn


def precomp_pick(d, a):
    s = big_step(d)
    if not s and abs(d) > 1:
        if d >= 4 and a >= 1: s = -1
        elif d <= -4 and a <= -1: s = 1
        elif d == 3 and a >= 0: s = -1
        elif d == -3 and a <= 0: s = 1
        elif abs(a) >= 3:
            if d > 0 and a > 0: s = -1
            elif d < 0 and a < 0: s = 1
            elif a >= 5: s = -2
            elif a <= -5: s = 2
            elif a >= 4: s = -1
            elif a <= -4: s = 1
    return s


PICK = np.array([[precomp_pick(d, a) for a in range(-5, 6)] for d in range(-12, 13)], np.int32)
RIGHT = np.array([precomp_right(d) for d in range(-40000, 40001)], np.int32)


def y9_walk(d, first, last):
    """Y9 along the rows of d [..., 256] with the difference before each row (first) and behind it (last): the steps, and which (d, a) of
    precomp_pick's table each cell met"""
    d = d.astype(np.int32)
    prev = first.astype(np.int32)
    steps = np.empty_like(d)
    met = np.zeros(PICK.shape, bool)
    for k in range(d.shape[-1]):
        dn = d[..., k + 1] if k + 1 < d.shape[-1] else last.astype(np.int32)
        di, ai = np.clip(d[..., k], -12, 12) + 12, np.clip(RIGHT[dn + 40000] + prev, -5, 5) + 5
        met[di, ai] = True
        steps[..., k] = PICK[di, ai]
        prev = d[..., k] + steps[..., k]
    return steps, met


def lane_rounds(d, first, last):
    """the rounds the kernel's lane-parallel form of the walk needs for one row: a lane four cells, its incoming step guessed from its left
    neighbour's untouched difference, then handed on until nothing moves"""
    d = [int(v) for v in d]
    guess = [first] + [d[4 * l - 1] for l in range(1, 64)]
    rounds = 0
    while True:
        rounds += 1
        out = []
        for l in range(64):
            prev = guess[l]
            for k in range(4 * l, 4 * l + 4):
                dn = d[k + 1] if k < 255 else last
                prev = d[k] + precomp_pick(max(-12, min(12, d[k])), max(-5, min(5, precomp_right(dn) + prev)))
            out.append(prev)
        new = [first] + out[:63]
        if new == guess:
            return rounds
        guess = new


# ---------------------------------------------------------------------------------------------- CPU part: the four-cells-a-lane first direction
def ana_line(x):
    """the analysis' first direction of a line (filters.c:40-86): un-normalised taps with the mirrored ends"""
    x = [int(v) for v in x]
    s = len(x)
    at = lambda i: x[-i] if i < 0 else x[2 * (s - 1) - i] if i >= s else x[i]
    lo = [6 * x[2 * k] + 2 * (at(2 * k - 1) + x[2 * k + 1]) - (at(2 * k - 2) + (x[2 * k + 2] if 2 * k + 2 < s else x[s - 2])) for k in range(s // 2)]
    hi = [2 * x[2 * k + 1] - (x[2 * k] + (x[2 * k + 2] if 2 * k + 2 < s else x[s - 2])) for k in range(s // 2)]
    return lo, hi


def taps(d, pv, nx, first):
    """ana_row_taps (nhw_dwt.h) on (even, odd) pairs"""
    e0, o0, e1 = d[0], d[1], nx[0]
    em1, om1 = (e1, o0) if first else pv
    return 6 * e0 + 2 * (om1 + o0) - (em1 + e1), 2 * o0 - (e0 + e1)


def quad_line(x):
    """ana_row_quad's arrangement: lane l holds a = cells (4l, 4l+1), b = (4l+2, 4l+3); the pair before a comes from lane l - 1's b, the cell
    behind b from lane l + 1's a, lane 63 hands in b itself"""
    a = [(int(x[4 * l]), int(x[4 * l + 1])) for l in range(64)]
    b = [(int(x[4 * l + 2]), int(x[4 * l + 3])) for l in range(64)]
    lo, hi = [0] * 128, [0] * 128
    for l in range(64):
        lo[2 * l], hi[2 * l] = taps(a[l], b[l - 1] if l else (0, 0), b[l], l == 0)
        lo[2 * l + 1], hi[2 * l + 1] = taps(b[l], a[l], a[l + 1] if l < 63 else b[l], False)
    return lo, hi


def test_four_cells_a_lane_first_direction_is_the_line_filter():
    """Every position of a 256-cell line carries an impulse in turn (the filter is linear: with the constant line and random lines of the whole
    int16 range that is its whole behaviour), the lane arrangement against the plain line filter with the reference's mirrored ends."""
    rng = np.random.default_rng(7)
    lines = [np.eye(256, dtype=np.int64)[i] * v for i in range(256) for v in (1, -32768)]
    lines += [np.full(256, 32767), np.full(256, -32768)] + [rng.integers(-32768, 32768, 256) for _ in range(64)]
    for x in lines:
        assert quad_line(x) == ana_line(x)


def test_pattern_row_hands_a_step_on_to_its_end():
    """the difference row the GPU cases use for Y9's fixed point: a change of the incoming step changes (almost) every cell, and the lane-parallel
    walk needs many rounds"""
    d = np.array([PATTERN[i % 4] for i in range(256)])[None]
    a, _ = y9_walk(d, np.array([0]), np.array([0]))
    b, _ = y9_walk(d, np.array([3]), np.array([0]))
    assert (a != b).sum() >= 250 and (a != b)[0, 250:].any()
    assert lane_rounds(d[0], 0, 0) > 32                          # (handed 3, every lane's guess is right at once)


# ---------------------------------------------------------------------------------------------- GPU part (the hook: tests/enc_stages.py)
def check_case(imgs, q, compat=False):
    n = len(imgs)
    h = Hook(n)
    try:
        if compat:
            h.e.set_compat(True)
        files = h.e.encode(imgs, q)                                 # the production path
        left = [p[:3] + [np.zeros(Q, np.int16)] for p in h.planes()]   # what the batch left: LL1 without its tags, the level-1 details round the block; l2save cleared
        fused = h.run(0, left)
        staged = h.run(3, left)
        compare(f"q{q} compat={compat} production launches against the staged kernels:", fused, staged)
        assert q <= 12 or all(p[3].any() for p in staged)           # (q <= 12: the copy is made behind Y12, outside these launches)
    finally:
        h.e.close()
    want = oracle_files(imgs, q, compat)
    bad = [i for i in range(n) if files[i] != want[i]]
    assert not bad, f"q{q} compat={compat}: files {bad[:16]} differ from the oracle"
    return n


def threshold_planes(h, q, seed):
    """Planes for forms 1 / 2 (from the synthesis on).  The coefficient block is random (LL2 in 300 .. 1200, details within +-8); its synthesis R is
    read off the device (form 5: the staged synthesis alone); LL1 = R - D with D the differences wanted:
      image % 4 == 0: every value of -14 .. 14 at random (every threshold of big_step and precomp_pick from both sides, every neighbour sum);
      image % 4 == 1: rows of PATTERN, rotated from row to row (Y9's fixed point runs the length of the row);
      image % 4 == 2: -5 .. 5 at random (the small-difference branches, a on both sides of 0, +-1, +-3, +-4, +-5);
      image % 4 == 3: PATTERN rows and random rows of -8 .. 8 interleaved;
    images 1 and 3 (mod 4) also get outer neighbours (columns 511 and 256 of proc) within +-6 of the LL1 cell they are compared with, so that
    the difference handed into a row is small; the other images keep the large ones real planes have;
    then tags (+16000 / +12000) on the first and last row and column of each detail quadrant and on one cell in twenty elsewhere in them (not in the images of PATTERN rows alone)."""
    n = h.n
    rng = np.random.default_rng(seed)
    coef = rng.integers(-8, 9, (n, 512, 512)).astype(np.int16)       # the work plane: the block and small cells round it
    coef[:, :128, :128] = rng.integers(300, 1201, (n, 128, 128))
    proc = rng.integers(-12, 13, (n, 512, 512)).astype(np.int16)     # cells outside the block: columns 511 and 256 are Y9's outer neighbours
    zero = np.zeros((256, 256), np.int16)
    recon = np.stack([p[1].reshape(512, 512)[:256, :256] for p in h.run(5, [(coef[i], proc[i], zero, zero) for i in range(n)])]).astype(np.int32)
    d = np.empty((n, 256, 256), np.int32)
    pat = np.array([[PATTERN[(c + r) % 4] for c in range(256)] for r in range(256)])
    for i in range(n):
        if i % 4 == 0: d[i] = rng.integers(-14, 15, (256, 256))
        elif i % 4 == 1: d[i] = pat
        elif i % 4 == 2: d[i] = rng.integers(-5, 6, (256, 256))
        else:
            d[i] = rng.integers(-8, 9, (256, 256))
            d[i, ::2] = pat[::2]
    ll1 = recon - d
    for i in range(n):
        if i % 4 in (1, 3):
            proc[i, :256, 511] = ll1[i, :, 255] + rng.integers(-6, 7, 256)          # proc[r][511] is the cell before row r + 1
            proc[i, :255, 256] = ll1[i, 1:, 0] + rng.integers(-6, 7, 255)
    assert ll1.min() > -1500 and ll1.max() < 9000                   # a tag can be told from a value
    tag = rng.random((n, 256, 256)) < 0.05
    tag[1::4] = False                                                # (a nudge in the middle of a PATTERN row would end its chain there)
    for lo in (0, 128):
        for hi in (127, 255):
            tag[:, lo, :] = tag[:, hi, :] = tag[:, :, lo] = tag[:, :, hi] = True
    tag[:, :128, :128] = False                                       # Y5 tags details only
    up = rng.random((n, 256, 256)) < 0.5
    tagged = (ll1 + np.where(tag, np.where(up, 16000, 12000), 0)).astype(np.int16)
    return coef, proc, ll1, tagged, tag, up, recon


def check_threshold_planes(q, n=16):
    h = Hook(n)
    try:
        h.e.encode(synthetic_images(q, n), q)                       # the hook works at the quality of the handle's last whole batch
        coef, proc, ll1, tagged, tag, up, recon = threshold_planes(h, q, 9100 + q)
        zero = np.zeros((256, 256), np.int16)
        inputs = [(coef[i], proc[i], tagged[i], zero) for i in range(n)]
        # ---- the situations: Y8's nudges (nhw_encoder.c:205-213), then Y9's walk on the differences
        nudged = recon.copy()
        step = np.where(tag, np.where(up, 1, -1), 0)
        nudged[:, 1::2, 0::2] += step[:, :128, 128:].transpose(0, 2, 1)     # tag (r, j >= 128) -> cell (2 (j - 128) + 1, 2 r)
        nudged[:, 0::2, 1::2] += step[:, 128:, :128].transpose(0, 2, 1)     # tag (r >= 128, j) -> cell (2 j, 2 (r - 128) + 1)
        nudged[:, 1::2, 1::2] += step[:, 128:, 128:].transpose(0, 2, 1)     # both                -> cell (2 (j - 128) + 1, 2 (r - 128) + 1)
        d = nudged - ll1
        behind = np.array([h.read(B_LL1, i, 2 * Q + 2)[Q] for i in range(n)], np.int32)
        flat = ll1.reshape(n, -1)
        o_before = np.concatenate([np.zeros((n, 1), np.int32), flat[:, 255:-1:256]], 1)           # the LL1 cell before a row (before the plane: the zero guard)
        o_behind = np.concatenate([flat[:, 256::256], behind[:, None]], 1)
        p = proc.astype(np.int32)
        p_before = np.concatenate([np.zeros((n, 1), np.int32), p[:, :255, 511]], 1)                # proc[r][-1] = proc[r - 1][511]
        steps, met = y9_walk(d, p_before - o_before, p[:, :256, 256] - o_behind)
        assert met.all(), f"q{q}: {(~met).sum()} entries of precomp_pick's table not met: {np.argwhere(~met)[:8].tolist()}"
        for v in range(-13, 14):
            assert (d == v).any(), f"q{q}: no difference of exactly {v}"
        edge_in, edge_out = p_before - o_before, p[:, :256, 256] - o_behind
        rounds = [lane_rounds(d[1, r], int(edge_in[1, r]), int(edge_out[1, r])) for r in range(2, 254, 19)]   # (rows 0, 1, 254, 255: nudged in every cell)
        assert max(rounds) >= 32, f"q{q}: Y9's fixed point settles within {max(rounds)} rounds on the PATTERN rows"   # a correction that runs half a row or more, lane by lane
        for lo in (0, 128):
            for hi in (127, 255):
                assert tag[:, lo, 128:].all() and tag[:, 128:, lo].all() and tag[:, hi, 128:].all() and tag[:, 128:, hi].all()
        # ---- every cell of every plane
        staged = h.run(2, inputs)
        fused = h.run(1, inputs)
        compare(f"q{q} threshold planes, the fused kernel against the staged ones:", fused, staged)
        ll1_out = np.stack([s[2][:Q].reshape(256, 256) for s in staged])
        assert (ll1_out == ll1).all(), "B_LL1 does not come back without its tags"
    finally:
        h.e.close()
    return n


def check_border_details(q, n=16):
    """forms 0 / 3 on written LL1 blocks of low amplitude: level-2 details of 2 .. 4 everywhere, the block's first and last rows and columns
    included (Y5 takes a sample's diagonal neighbours by linear index: row 0 has none above, column 255's lower one is a cell outside the
    block, row 255's lie in row 256 of the work plane) -- read off the tags form 4 leaves in B_LL1"""
    h = Hook(n)
    try:
        h.e.encode(synthetic_images(q, n), q)
        rng = np.random.default_rng(9300 + q)
        ll1 = (600 + rng.integers(-3, 4, (n, 256, 256)) * np.array([1, 2, 3, 4])[np.arange(n) % 4, None, None]).astype(np.int16)
        work = rng.integers(-4, 5, (n, 512, 512)).astype(np.int16)
        proc = rng.integers(-4, 5, (n, 512, 512)).astype(np.int16)
        proc[n // 2:, 256, :] = 0                                    # row 256 with and without non-zero neighbours
        zero = np.zeros((256, 256), np.int16)
        inputs = [(work[i], proc[i], ll1[i], zero) for i in range(n)]
        tags = np.stack([p[2][:Q].reshape(256, 256) for p in h.run(4, inputs)]) > 10000
        for name, m in (("row 0", tags[:, 0, 128:]), ("row 255", tags[:, 255, :]), ("column 255", tags[:, :, 255]), ("row 128", tags[:, 128, :]),
                        ("column 128", tags[:, :, 128]), ("row 127", tags[:, 127, 128:]), ("column 127", tags[:, 128:, 127]), ("column 0", tags[:, 128:, 0])):
            assert m.any() and not m.all(), f"q{q}: tags of {name}: {m.sum()} of {m.size}"
        assert not tags[:, :128, :128].any()
        staged = h.run(3, inputs)
        fused = h.run(0, inputs)
        compare(f"q{q} border details, production launches against the staged kernels:", fused, staged)
    finally:
        h.e.close()
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("q", QUALITIES)
def test_luma_loop_equals_the_staged_kernels_and_the_oracle(q, compat):
    """64 generator images a quality and mode: the files of the production batch byte for byte, then every plane behind the hook."""
    assert check_case(synthetic_images(q), q, compat) == N_IMAGES


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_luma_loop_on_threshold_planes(q):
    assert check_threshold_planes(q) == 16


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_luma_loop_on_border_details(q):
    assert check_border_details(q) == 16
