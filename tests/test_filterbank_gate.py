"""The analysis' second direction (ana_col_pair, nhwcodec_amd/csrc/nhw_dwt.h) at the gate between its two forms.

A wavefront -- one pair of columns of the first-direction plane -- takes the packed 16-bit form when every cell of both columns lies in
GATE_LO .. GATE_HI, and the 32-bit form otherwise.  This module holds
  * a numpy model of both forms and of the gate, held to oracle.analysis(..., keep=True) on the CPU: the packed form equals the oracle on every
    pair the gate lets through (the header's 10 x 3000 + 2 x 1300 < 32768, checked numerically), and differs from it on every "outlier" pair,
    so that a gate that lets such a pair through shows in the GPU comparisons;
  * planes AT the gate, one cell past it, mixed and far out, run through the staged kernels (k_dwt_ana<256>, <128>) against the oracle and through
    the fused kernels (k_chroma_loops, k_l2_recon) against the staged ones and the oracle;
  * pictures that cross the gate (hard-edged colour patterns), whole files against the oracle;
  * the ungated form of k_chroma_l1q on byte planes of the colour stage's extremes.
Every comparison is exact equality."""
import ctypes
import functools

import numpy as np
import pytest

from tests.enc_stages import B_CL2SAVE, B_CLL1, B_CPROC, Q, Hook, chroma_images, compare, synthetic_images, ws_index

GATE_LO, GATE_HI = -1300, 3000
SGN = np.array([1, 1, -1, 1])       # the sign of the low-pass taps around an output at 2k, from 2k on, period 4
STAGED = [(512, 256, 1), (256, 256, 0), (256, 128, 1), (512, 256, 0)]


# ---------------------------------------------------------------------------------------------- the model
def _w16(x):
    return ((x + 32768) & 0xFFFF) - 32768


def _diffuse(r, wrap):
    s = r >> 63
    a = wrap((r ^ s) - s)
    t = ((a & 63) ^ 32) - 32                                        # |r| mod 64 read as a signed 6-bit number
    d = (t + ((t >> 63) & 3)) >> 2
    return (d ^ s) - s


def second_direction(x, left, packed):
    """ana_col_pair on columns x [..., S] (the last axis runs along the second direction).  packed: every intermediate wraps to int16 as s16x2
    arithmetic does; else plain int64 with the one (int16_t)(r + carry) the code has.  Returns lo, hi [..., S / 2] and the accumulator r + carry."""
    x = np.asarray(x, np.int64)
    h = x.shape[-1] // 2
    w = _w16 if packed else (lambda v: v)
    e0, o0 = x[..., 0::2], x[..., 1::2]
    e1 = np.concatenate([e0[..., 1:], e0[..., -1:]], -1)            # x[S] = x[S - 2]
    em1 = np.concatenate([e1[..., :1], e0[..., :-1]], -1)           # x[-2] = x[2]
    om1 = np.concatenate([o0[..., :1], o0[..., :-1]], -1)           # x[-1] = x[1]
    r = w(w(w(e0 * 6) + w(w(om1 + o0) * 2)) - w(em1 + e1))
    a = w(e0 + e1)
    a = w(a + (a & w(em1 + e0) & (np.arange(h) & 1)))
    pp, tail = w(o0 - (a >> 1)), w(o0 - e0)
    last = np.arange(h) == h - 1
    rnd = lambda v, sh: w(v + (1 << (sh - 1)) + (v >> 63)) >> sh
    if left:
        carry = np.concatenate([np.zeros_like(r[..., :1]), _diffuse(r[..., :-1], w)], -1)
        acc = r + carry
        lo = rnd(_w16(acc), 6)
        hi = np.where(last, tail >> 3, rnd(pp, 3))
    else:
        acc = r
        lo = rnd(r, 4)
        hi = np.where(last, w(tail + 1) >> 1, rnd(pp, 1))
    return _w16(lo), _w16(hi), acc


def model_block(t, packed):
    """the coefficient block [S, S] of a first-direction plane t [S, S] (t[c] = column c), and the accumulators"""
    s = t.shape[0]
    h = s // 2
    ll, lh, acc_l = second_direction(t[:h], True, packed)
    hl, hh, acc_r = second_direction(t[h:], False, packed)
    return np.concatenate([np.concatenate([ll, lh], 1), np.concatenate([hl, hh], 1)], 0).astype(np.int16), np.concatenate([acc_l, acc_r], 0)


def wide_pairs(t):
    """the gate: pair p = columns 2p, 2p + 1 of the first-direction plane; wide when any cell of the two, over all rows, lies outside GATE_LO .. GATE_HI"""
    t = np.asarray(t, np.int64)
    out = (t < GATE_LO) | (t > GATE_HI)
    return out.reshape(t.shape[0] // 2, -1).any(1)


def reference(oracle, block, stride, size, final):
    """oracle.analysis of an S x S block in a stride x stride plane of zeros: coefficient block, kept first-direction plane, work plane behind it"""
    plane = np.zeros((max(stride, 2 * Q // stride), stride), np.int16)     # (keep copies 2 Q cells from the start of the plane)
    plane[:size, :size] = block
    j, p, k = oracle.analysis(plane.ravel(), stride, size, final, keep=True)
    j, p, k = (a.reshape(-1, stride) for a in (j, p, k))
    return p[:size, :size].copy(), k[:size, :size].copy(), j[:size, :size].copy()


# ---------------------------------------------------------------------------------------------- the planes
def pattern(size, phase, sign, margin=0):
    """GATE_HI where the taps of the outputs of lattice phase `phase` are positive, GATE_LO where negative (sign < 0: the other way round); margin:
    both that far inside the gate"""
    s = SGN[(np.arange(size) - phase) % 4] * sign
    return np.where(s > 0, GATE_HI - margin, GATE_LO + margin)


def plane_for(target, base, half):
    """The S x S input whose first direction leaves target [S / 2, S] (cell [k, j]: column k of the half, row j) in the left (half 0) or right half.
    Row j has constant even cells v: lo_k = 4 v + 2 (o_{k-1} + o_k) (o_{-1} = o_0), hi_k = 2 (o_k - v).  v puts the other half round 850, the middle
    of the gate (base [S]: the row's prevalent target value)."""
    h, s = target.shape
    t = target.astype(np.int64)
    if half == 0:
        v = np.rint((base / 2 - 850) / 4).astype(np.int64)
        assert not ((t[0] - 4 * v) % 4).any() and not (t % 2).any()
        o = np.empty((h, s), np.int64)
        o[0] = (t[0] - 4 * v) // 4
        for k in range(1, h):
            o[k] = (t[k] - 4 * v) // 2 - o[k - 1]
    else:
        assert not (t % 2).any()
        v = np.rint((850 - 2 * base) / 8).astype(np.int64)
        o = t // 2 + v
    p = np.empty((s, s), np.int64)
    p[:, 0::2] = v[:, None]
    p[:, 1::2] = o.T
    assert np.abs(p).max() < 32768
    return p.astype(np.int16)


def plane_opposite(size, phase, sign, hi_val, lo_val):
    """Lines of period 4 (a b c b): the even columns of the left half follow the pattern with hi_val / lo_val, the odd ones its opposite -- the
    two columns of every dword at opposite ends of the gate.  6a + 4b - 2c = X, 6c + 4b - 2a = Y."""
    up = SGN[(np.arange(size) - phase) % 4] * sign > 0
    x, y = np.where(up, hi_val, lo_val).astype(np.int64), np.where(up, lo_val, hi_val).astype(np.int64)
    d = (x - y) // 8
    assert not ((x - y) % 8).any() and not ((x - 6 * d) % 4).any()
    c = np.rint(((x - 6 * d) / 2 - d - 850) / 4).astype(np.int64)
    b = (x - 6 * d) // 4 - c
    a = c + d
    p = np.empty((size, size), np.int64)
    p[:, 0::4], p[:, 1::4], p[:, 2::4], p[:, 3::4] = a[:, None], b[:, None], c[:, None], b[:, None]
    return p.astype(np.int16)


def sweep_rows(size):
    rows = [0, 1, 2, 3, size // 2 - 2, size // 2 - 1, size // 2, size // 2 + 1, 100, 101, size - 2, size - 1]   # the mirrored ends, the tail cell, lanes 63 / 64 (the u index for S = 256)
    return rows + ([200, 201] if size == 256 else [])


@functools.lru_cache(maxsize=None)
def outlier_column(size, row, left, margin=0):
    """the column (phase, sign, value) with one cell moved past the gate at `row` for which the packed form leaves the oracle's value.  In the
    left half the reference itself wraps r + carry to 16 bits: there the two forms part only in the carry handed on (diffuse of the wrapped r has
    the other sign) and in the rounding offset, so the value is searched: 3300 / -3000 onwards in steps of 4 (row S - 1 feeds only
    the last output, whose taps sum to less: it needs more)."""
    vals = np.r_[3300:3800:4, 3800:6000:12, 6000:14000:40]
    best = None
    for phase in (0, 2, 1, 3):
        for sign in (1, -1):
            cols = np.tile(pattern(size, phase, sign, margin), (len(vals), 1))
            cols[:, row] = vals if cols[0, row] > 0 else 300 - vals
            a, b = second_direction(cols, left, True), second_direction(cols, left, False)
            hit = np.flatnonzero((a[0] != b[0]).any(1) | (a[1] != b[1]).any(1))
            if hit.size and (best is None or hit[0] < best[0]):
                best = (int(hit[0]), phase, sign, int(cols[hit[0], row]))
    if best:
        return best[1:]
    raise AssertionError(f"no outlier at row {row} makes the packed form wrap")


@functools.lru_cache(maxsize=None)
def families(size, margin=0):
    """[(family, name, block [S, S] int16, half, the pairs of that half meant to be wide)] -- `half`: the half the plane aims at"""
    h, out = size // 2, []
    npairs = h // 2
    for half in (0, 1):
        left = half == 0
        side = "left" if left else "right"
        for phase in range(4):
            for sign in (1, -1):
                col = pattern(size, phase, sign, margin)
                out.append(("gate", f"at the gate {side} phase {phase} sign {sign}", plane_for(np.tile(col, (h, 1)), col, half), half, ()))
        if left:
            out.append(("gate", "opposite extremes 3000 / -1288", plane_opposite(size, 0, 1, 3000, -1288), 0, ()))
            out.append(("gate", "opposite extremes 2988 / -1300", plane_opposite(size, 2, -1, 2988, -1300), 0, ()))
        combos = [(r, c) for r in sweep_rows(size) for c in (0, 1)]
        n = 0

        def with_outliers(cells):
            """per pair its own pattern, one cell of it moved out"""
            t = np.empty((h, size), np.int64)
            base = np.empty((npairs, size), np.int64)
            for p in range(npairs):
                base[p] = pattern(size, 0, 1, margin)
            vals = {}
            for k0, j0 in cells:
                phase, sign, val = outlier_column(size, j0, left, margin)
                base[k0 // 2] = pattern(size, phase, sign, margin)
                vals[(k0, j0)] = val
            t[0::2], t[1::2] = base, base
            for (k0, j0), val in vals.items():
                t[k0, j0] = val
            return plane_for(t, np.median(t, 0), half)

        for parity in (0, 1):                                           # mixed: every other pair wide, its neighbours at the gate
            for _ in range(2):
                cells = []
                for p in range(parity, npairs, 2):
                    r, c = combos[n % len(combos)]
                    n += 1
                    cells.append((2 * p + c, r))
                out.append(("mixed", f"every other pair wide {side} parity {parity} #{n}", with_outliers(cells), half, tuple(sorted({k // 2 for k, _ in cells}))))
        edge = [14, 15, 16, 17, h - 2, h - 1, 0, 1] if left else [0, 1, 14, 15, 16, 17, h - 2, h - 1]    # a wavefront's edge columns (c = 14 .. 17, 126 .. 129 of the plane)
        rows = sweep_rows(size)
        for i, k0 in enumerate(edge):                                    # one outlier: exactly one pair wide
            j0 = rows[(5 * i + (3 if left else 0)) % len(rows)]
            out.append(("outlier", f"one outlier {side} column {k0} row {j0}", with_outliers([(k0, j0)]), half, (k0 // 2,)))
        for i, val in enumerate((32766, -32768, 31468, -1302, 16000, -14000)):   # far out: the gate's own 16-bit sum wraps (31468 + 1300 = 32768, -1302 + 1300 = -2; every first-direction cell these planes can set is even)
            t = np.tile(pattern(size, 0, 1, margin), (h, 1)).astype(np.int64)
            k0, j0 = (17, h - 1, h - 3, 6, 33, 20)[i], (5, 100, size - 2, 1, 64, 127)[i]
            t[k0, j0] = val
            out.append(("far", f"far out {side} {val} at column {k0} row {j0}", plane_for(t, np.median(t, 0), half), half, (k0 // 2,)))
    return out


_REF = {}


def refs(oracle, stride, size, final, margin=0):
    key = (stride, size, final, margin)
    if key not in _REF:
        _REF[key] = [reference(oracle, f[2], stride, size, final) for f in families(size, margin)]
    return _REF[key]


# ---------------------------------------------------------------------------------------------- 1. CPU: the model, the gate, the planes
@pytest.mark.parametrize("stride,size,final", STAGED)
def test_model_and_case_planes(oracle, stride, size, final):
    fam = families(size)
    h = size // 2
    top, both_ends, kinds = -1 << 40, False, set()
    for (family, name, block, half, meant), (coef, kept, after) in zip(fam, refs(oracle, stride, size, final)):
        wide, acc = model_block(kept, False)
        assert np.array_equal(wide, coef), f"{name}: the wide model leaves the oracle's coefficients"
        if not final:
            assert np.array_equal(after[:h, :h], coef[:h, :h].T), f"{name}: LL copy"
        else:
            assert np.array_equal(after, kept), name
        gate = wide_pairs(kept)
        packed, _ = model_block(kept, True)
        ok = np.repeat(~gate, 2)
        assert np.array_equal(packed[ok], coef[ok]), f"{name}: the packed form leaves the oracle on a pair inside the gate"
        mine = gate[half * (h // 2):(half + 1) * (h // 2)]
        assert tuple(np.flatnonzero(mine)) == meant, f"{name}: wide pairs {np.flatnonzero(mine).tolist()}, meant {meant}"
        kinds.add((family, half, bool(gate.any()), bool((~gate).any())))
        if family == "gate":
            assert not gate.any(), f"{name}: the whole block is meant to take the packed form"
            top = max(top, int(acc.max()))
            pair = kept.reshape(h, 2 * size)
            both_ends |= bool(((pair == GATE_HI).any(1) & (pair == GATE_LO).any(1)).any())
        if family in ("outlier", "mixed"):
            for p in meant:
                rows = slice(2 * p + half * h, 2 * p + 2 + half * h)
                assert (packed[rows] != coef[rows]).any(), f"{name}: the packed form equals the oracle on pair {p}: a gate that lets it through would not show"
            assert (~mine).any()
    assert top == 10 * GATE_HI - 2 * GATE_LO == 32600, top
    assert both_ends
    for half in (0, 1):
        assert ("mixed", half, True, True) in kinds and ("outlier", half, True, True) in kinds and ("far", half, True, True) in kinds


def test_families_with_a_margin(oracle):
    """what the forms 1 / 2 of the luma hook get: the same planes with every cell that is meant to stay inside 100 away from the gate"""
    for (family, name, block, half, meant), (coef, kept, _) in zip(families(256, 100), refs(oracle, 512, 256, 1, 100)):
        if family == "gate":
            continue
        gate = wide_pairs(kept)
        mine = gate[half * 64:(half + 1) * 64]
        assert tuple(np.flatnonzero(mine)) == meant, name
        inside = kept[half * 128:(half + 1) * 128][np.repeat(~mine, 2)]
        assert inside.min() >= GATE_LO + 100 and inside.max() <= GATE_HI - 100, name
        packed = model_block(kept, True)[0]
        assert np.array_equal(model_block(kept, False)[0], coef), name
        if family != "far":
            for p in meant:
                rows = slice(2 * p + half * 128, 2 * p + 2 + half * 128)
                assert (packed[rows] != coef[rows]).any(), name


def test_opposite_extremes_share_a_dword(oracle):
    """the period-4 planes: the two columns of a pair at opposite ends of the gate in every row, and still packed"""
    for size in (256, 128):
        for f, ref in zip(families(size), refs(oracle, size, size, 1)):
            if f[1].startswith("opposite"):
                kept = ref[1][:size // 2].astype(np.int64)
                spread = np.abs(kept[0::2] - kept[1::2])[:-1]                 # (the last column mirrors its right neighbour)
                assert spread.min() >= 4288 and kept.max() <= GATE_HI and kept.min() >= GATE_LO and (kept.max() == GATE_HI or kept.min() == GATE_LO)


# ---------------------------------------------------------------------------------------------- 2. GPU: the staged kernels
@pytest.fixture(scope="module")
def enc():
    import nhwcodec_amd
    e = nhwcodec_amd.Encoder(0, max_batch=64)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride,size,final", STAGED)
def test_staged_analysis_at_the_gate(enc, oracle, stride, size, final):
    """k_dwt_ana<256> / <128> behind nhw_stage_analysis on every family: coefficient block, transposed first-direction plane, LL copy-back"""
    import torch
    fam = families(size)
    want = refs(oracle, stride, size, final)
    planes = np.zeros((len(fam), stride, stride), np.int16)
    for i, f in enumerate(fam):
        planes[i, :size, :size] = f[2]
    j, p = torch.from_numpy(planes).cuda(), torch.zeros(planes.shape, dtype=torch.int16, device="cuda")
    assert enc.lib.nhw_stage_analysis(enc.h, j.data_ptr(), p.data_ptr(), len(fam), stride * stride, stride, size, final, None) == 0
    torch.cuda.synchronize()
    gj, gp = j.cpu().numpy(), p.cpu().numpy()
    for i, (f, (coef, kept, after)) in enumerate(zip(fam, want)):
        bad = np.argwhere(gp[i, :size, :size] != coef)
        assert bad.size == 0, f"{f[1]}: {len(bad)} coefficients differ, first (row, cell) {bad[:6].tolist()}"
        bad = np.argwhere(gj[i, :size, :size] != after)
        assert bad.size == 0, f"{f[1]}: transposed plane / LL copy-back: {len(bad)} cells differ, first {bad[:6].tolist()}"


# ---------------------------------------------------------------------------------------------- 3. GPU: the fused kernels, through the hooks
B_CJPEG, B_PV = ws_index("CJPEG"), ws_index("PV")


@pytest.mark.gpu
@pytest.mark.parametrize("q", [15, 20])
def test_chroma_loops_at_the_gate(oracle, q):
    """The 128 x 128 families as B_CLL1.  Form 2 (k_dwt_ana<128> reading cll1) against the oracle; k_chroma_loops (form 1) against the seven
    staged kernels (form 8) on every plane; and its second analysis against the oracle's of the pre-compensated block, which form 5 leaves in
    cjpeg -- that block must itself have wide pairs beside packed ones.  q15 / q20: both forms of the first simulation."""
    import torch
    fam = families(128)
    want = refs(oracle, 256, 128, 1)
    n = len(fam)
    ll1 = np.stack([f[2] for f in fam])
    cproc = np.random.default_rng(4300 + q).integers(-12, 13, (n, 256, 256)).astype(np.int16)
    h = Hook(n)

    def run(comp, form):
        for i in range(n):
            h.write(B_CLL1, i, ll1[i])
            h.write(B_CPROC, i, cproc[i])
        assert h.e.lib.nhw_stage_chroma_loops(h.e.h, n, comp, form, None) == 0
        torch.cuda.synchronize()
        return [(h.read(B_CPROC, i, 2 * Q).reshape(256, 256), h.read(B_CL2SAVE, i, Q // 2).reshape(128, 128), h.read(B_CLL1, i, Q // 2 + 2),
                 h.read(B_CJPEG, i, 2 * Q).reshape(256, 256)[:128, :128]) for i in range(n)]

    try:
        h.e.encode(chroma_images(q, n), q)                          # the hook works at the quality of the handle's last whole batch
        for comp in (0, 1):
            for i, (g, (coef, kept, _)) in enumerate(zip(run(comp, 2), want)):
                assert np.array_equal(g[0][:128, :128], coef), f"q{q} comp {comp} {fam[i][1]}: first analysis, coefficients"
                assert np.array_equal(g[3], kept), f"q{q} comp {comp} {fam[i][1]}: first analysis, transposed plane"
            pre = [g[3].copy() for g in run(comp, 5)]               # the pre-compensated block (chroma_p3_par writes it into cjpeg)
            staged, fused = run(comp, 8), run(comp, 1)
            mixed = 0
            for i in range(n):
                assert np.abs(pre[i].astype(np.int32) - ll1[i]).max() <= 6, "cjpeg is not the pre-compensated block"
                for name, got, ref in zip(("cproc", "cl2save", "cll1 + neighbour"), fused[i], staged[i]):
                    bad = np.flatnonzero(got.ravel() != ref.ravel())
                    assert bad.size == 0, f"q{q} comp {comp} {fam[i][1]} {name}: {bad.size} cells differ, first {bad[:8].tolist()}"
                coef2, kept2, _ = reference(oracle, pre[i], 256, 128, 1)
                bad = np.argwhere(fused[i][1] != coef2)
                assert bad.size == 0, f"q{q} comp {comp} {fam[i][1]}: k_chroma_loops' second analysis leaves the oracle's in {len(bad)} cells, first {bad[:6].tolist()}"
                gate2 = wide_pairs(kept2)
                mixed += bool(gate2.any() and not gate2.all())
            assert mixed, "no pre-compensated block with wide pairs beside packed ones"
    finally:
        h.e.close()


def _luma_inputs(fam, seed):
    rng = np.random.default_rng(seed)
    n = len(fam)
    return rng.integers(-4, 5, (n, 512, 512)).astype(np.int16), rng.integers(-4, 5, (n, 512, 512)).astype(np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("q", [10, 14])
def test_luma_loop_at_the_gate_production_against_staged(oracle, q):
    """The 256 x 256 families as B_LL1 (the first level-2 analysis reads it through altb): form 0 against form 3 on every plane.
    q14: k_l2_recon<true> (the fused second analysis), q10: k_l2_recon<false> followed by k_dwt_ana<256>."""
    fam = [f for f in families(256) if f[2].max() < 10000]           # (an LL1 cell above 10000 reads as one of Y5's tags: the planes whose far-out cell needs such an input stay with the staged kernels)
    n = len(fam)
    assert n >= 48 and sum(f[0] == "far" for f in fam) >= 6
    work, proc = _luma_inputs(fam, 9500 + q)
    zero = np.zeros((256, 256), np.int16)
    h = Hook(n)
    try:
        h.e.encode(synthetic_images(q, n), q)
        inputs = [(work[i], proc[i], fam[i][2], zero) for i in range(n)]
        staged = h.run(3, inputs)
        fused = h.run(0, inputs)
        compare(f"q{q} families, production launches against the staged kernels:", fused, staged)
    finally:
        h.e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", [10, 14])
def test_luma_loop_at_the_gate_from_the_synthesis_on(oracle, q):
    """Forms 1 / 2: the analysis input is ll1 + Y9's step (at most 7: big_step), 12 x 7 = 84 in a first-direction cell -- the families with a margin
    of 100 (mixed, one outlier, far out).  The coefficient block is the oracle's analysis of the plane, so that the synthesis comes back close
    to it.  The transposed first-direction plane form 2 stores shows which pairs were wide: both kinds within one block; the model's wide form
    on that plane is the coefficient block both forms must leave (l2save: q14)."""
    fam = [f for f in families(256, 100) if f[0] != "gate" and f[2].max() < 10000]   # (an LL1 cell above 10000 reads as one of Y5's tags)
    assert len(fam) >= 30 and sum(f[0] == "far" for f in fam) >= 6
    n = len(fam)
    work, proc = _luma_inputs(fam, 9700 + q)
    for i, f in enumerate(fam):
        work[i, :256, :256] = reference(oracle, f[2], 512, 256, 1)[0]
    zero = np.zeros((256, 256), np.int16)
    h = Hook(n)
    try:
        h.e.encode(synthetic_images(q, n), q)
        inputs = [(work[i], proc[i], fam[i][2], zero) for i in range(n)]
        staged = h.run(2, inputs)
        fused = h.run(1, inputs)
        compare(f"q{q} families with a margin, the fused kernel against the staged ones:", fused, staged)
        both = 0
        for i, f in enumerate(fam):
            kept = fused[i][0].reshape(512, 512)[:256, :256]
            gate = wide_pairs(kept)
            half = slice(f[3] * 64, f[3] * 64 + 64)
            assert tuple(np.flatnonzero(gate[half])) == f[4], f"q{q} {f[1]}: wide pairs {np.flatnonzero(gate[half]).tolist()}, meant {f[4]}"
            both += bool(gate.any() and not gate.all())
            coef = model_block(kept, False)[0]
            assert np.array_equal(fused[i][1].reshape(512, 512)[:256, :256], coef), f"q{q} {f[1]}: coefficient block against the model's wide form"
            if q > 12:
                assert np.array_equal(fused[i][3].reshape(256, 256), coef), f"q{q} {f[1]}: l2save"
        assert both == n
    finally:
        h.e.close()


# ---------------------------------------------------------------------------------------------- 4. pictures that cross the gate
CORNER = dict(black=(0, 0, 0), white=(255, 255, 255), blue=(255, 0, 0), yellow=(0, 255, 255), red=(0, 0, 255), cyan=(255, 255, 0), green=(0, 255, 0), magenta=(255, 0, 255))   # BGR
PICTURE_Q = (10, 13, 16, 20, 23)
TAPS = {-2: -1, -1: 2, 0: 6, 1: 2, 2: -1}


def lattice_picture(a, b, cell, shift):
    """colour a where the (+ + - +) pattern of `cell`-pixel cells, shifted by `shift` cells, is positive in both directions or negative in both"""
    s = SGN[(np.arange(512) // cell - shift) % 4]
    pos = s[:, None] * s[None, :] > 0
    return np.where(pos[:, :, None], np.array(CORNER[a], np.uint8), np.array(CORNER[b], np.uint8)).astype(np.uint8)


def aimed_picture(a, b, cell, period=16):
    """Aimed at single cells of the level-2 first-direction plane: along a row, colour a where the weight of the picture's cell in output k (the
    level-1 low-pass followed by the level-2 first direction) is positive, for one k in every `period` cells; down the columns the level-1
    pattern.  The contrast rises from 0.7 to 1 along the row, a step a period: some column pairs end just inside the gate, some outside."""
    n = 512 // cell
    sx = -np.ones(n)
    for k in range(2, n // 4 - 2, period // 4):
        w = np.zeros(n)
        for m, t2 in TAPS.items():
            for d, t1 in TAPS.items():
                x = 2 * (2 * k + m) + d
                if 0 <= x < n:
                    w[x] += t2 * t1
        seg = np.arange(max(4 * k - period // 2, 0), min(4 * k + period // 2, n))
        sx[seg] = np.where(w[seg] > 0, 1, -1)
    pos = (SGN[np.arange(n) % 4][:, None] * sx[None, :]) > 0
    s = np.linspace(0.7, 1.0, n // period).repeat(period)[None, :, None]
    ca, cb = np.array(CORNER[a], float), np.array(CORNER[b], float)
    img = np.where(pos[:, :, None], cb + s * (ca - cb), cb)
    return np.rint(img).astype(np.uint8).repeat(cell, 0).repeat(cell, 1)


@functools.lru_cache(maxsize=None)
def gate_pictures():
    return (("black / white, 2-pixel cells", lattice_picture("white", "black", 2, 2)),
            ("white / black, 2-pixel cells", lattice_picture("black", "white", 2, 2)),
            ("blue / yellow, 4-pixel cells", lattice_picture("yellow", "blue", 4, 2)),
            ("red / cyan, 4-pixel cells", lattice_picture("cyan", "red", 4, 2)),
            ("aimed white on black", aimed_picture("white", "black", 1)),
            ("aimed red on cyan", aimed_picture("red", "cyan", 2)),
            ("aimed blue on yellow", aimed_picture("blue", "yellow", 2)))


def level2_first_direction(oracle, img, q):
    """the kept first-direction planes of the level-2 analyses of Y, U and V as the encoder reaches them"""
    oracle.lib.nhwo_prefilter_chroma.argtypes = [ctypes.c_void_p, ctypes.c_int]
    y, u, v = oracle.color(img, q)
    if q < 22:
        y = oracle.prefilter(y, q)
    ll1 = oracle.analysis(y, 512, 512, 0)[0].reshape(512, 512)[:256, :256]
    out = [reference(oracle, ll1, 256, 256, 1)[1]]
    for c in (u, v):
        plane = c.astype(np.int16)
        if q <= 14:
            oracle.lib.nhwo_prefilter_chroma(plane.ctypes.data, q)
        cll1 = oracle.analysis(plane, 256, 256, 0)[0].reshape(256, 256)[:128, :128]
        out.append(reference(oracle, cll1, 256, 128, 1)[1])
    return out


def reach(t):
    """some pair outside the gate; some pair with a cell within 100 of either end and still inside"""
    pair = t.astype(np.int64).reshape(t.shape[0] // 2, -1)
    wide = ((pair < GATE_LO) | (pair > GATE_HI)).any(1)
    near = ((pair > GATE_HI - 100) | (pair < GATE_LO + 100)).any(1) & ~wide
    return bool(wide.any()), bool(near.any())


# where full-range corner colours can cross at all: the colour stage scales with the quality, and below these a picture aimed at the
# filters' own signs stays inside the gate (asserted: what no picture can reach needs no second form)
REACHABLE = {"Y": (16, 20, 23), "U": (20, 23), "V": (20, 23)}


def test_pictures_reach_the_gate(oracle):
    for q in PICTURE_Q:
        hit = {"Y": False, "U": False, "V": False}
        top = {"Y": 0, "U": 0, "V": 0}
        for name, img in gate_pictures():
            for plane, t in zip("YUV", level2_first_direction(oracle, img, q)):
                hit[plane] |= all(reach(t))
                top[plane] = max(top[plane], int(t.max()))
                assert t.min() > GATE_LO - 300 and t.max() < 3600, f"q{q} {name} {plane}: {t.min()} .. {t.max()}"
        for plane in "YUV":
            if q in REACHABLE[plane]:
                assert hit[plane], f"q{q}: no picture with {plane} pairs on both sides of the gate"
            else:
                assert top[plane] < GATE_HI, f"q{q}: {plane} reaches {top[plane]}: add the quality to REACHABLE"


@pytest.mark.gpu
@pytest.mark.parametrize("q", PICTURE_Q)
def test_pictures_that_cross_the_gate_encode_as_the_oracle(oracle, q):
    """the pictures between two generator images: files byte for byte, and the decoder's pixels from them against the oracle's decoder"""
    import nhwcodec_amd
    from gpu_fuzz_classes import encode_with_status
    imgs = np.stack([oracle.synth(700 + q)] + [im for _, im in gate_pictures()] + [oracle.synth(800 + q)])
    enc = nhwcodec_amd.Encoder(0, len(imgs))
    try:
        files, status = encode_with_status(enc, imgs, q)
    finally:
        enc.close()
    ok = []
    for i, im in enumerate(imgs):
        try:
            want, rc = oracle.encode(im, q), 0
        except RuntimeError as ex:                                   # the code book overflows: the reference's exit, that image alone
            want, rc = b"", int(str(ex).split("rc=")[-1])
        assert status[i] == rc and files[i] == want, f"q{q} image {i}: status {status[i]} (oracle {rc}), files {'differ' if files[i] != want else 'equal'}"
        if rc == 0:
            ok.append(i)
    assert 0 in ok and len(imgs) - 1 in ok and len(ok) >= 3
    dec = nhwcodec_amd.Decoder(0, max_batch=len(ok))
    try:
        px, qs = dec.decode([files[i] for i in ok])
    finally:
        dec.close()
    for k, i in enumerate(ok):
        want, wq = oracle.decode(files[i])
        assert qs[k] == wq == q and np.array_equal(px[k], want), f"q{q} image {i}: decoded pixels"


# ---------------------------------------------------------------------------------------------- 5. k_chroma_l1q: no gate at all
def colour_extremes(oracle, q):
    """(lo, hi, colour of lo, colour of hi) of the U and of the V byte the colour stage emits for the eight corner colours"""
    names = list(CORNER)
    img = np.zeros((512, 512, 3), np.uint8)
    for i, nm in enumerate(names):
        img[64 * i:64 * i + 64] = CORNER[nm]
    _, u, v = oracle.color(img, q)
    out = []
    for c in (u, v):
        vals = c.reshape(256, 256)[16::32, 0][:8].astype(int)
        assert all((c.reshape(256, 256)[32 * i + 2:32 * i + 30] == vals[i]).all() for i in range(8))
        out.append((int(vals.min()), int(vals.max()), names[int(vals.argmin())], names[int(vals.argmax())]))
    return out


def byte_patterns(lo, hi):
    """256 x 256 byte planes of {lo, hi} in the worst-case sign pattern of both directions: four lattice phases, both signs"""
    out = []
    for phase in range(4):
        s = SGN[(np.arange(256) - phase) % 4]
        for sign in (1, -1):
            out.append(np.where(s[:, None] * s[None, :] * sign > 0, hi, lo).astype(np.uint8))
    return out


@pytest.mark.parametrize("q", [15, 20, 23])
def test_byte_planes_stay_inside_the_packed_form(oracle, q):
    """k_chroma_l1q runs ana_col_pair without the gate: first-direction cells of a byte plane lie in -510 .. 2550, and on the worst planes of the
    colour stage's own extremes (and of 0 / 255) the packed form is the oracle's"""
    for lo, hi in [e[:2] for e in colour_extremes(oracle, q)] + [(0, 255)]:
        for plane in byte_patterns(lo, hi):
            coef, kept, _ = reference(oracle, plane.astype(np.int16), 256, 256, 0)
            assert kept.min() >= -510 and kept.max() <= 2550
            assert not wide_pairs(kept).any()
            assert np.array_equal(model_block(kept, True)[0], coef)
    assert max(int(reference(oracle, p.astype(np.int16), 256, 256, 0)[1].max()) for p in byte_patterns(0, 255)) == 2550


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 1, 2])
def test_chroma_level1_from_bytes_on_the_worst_planes(oracle, order):
    """k_chroma_l1q behind nhw_stage_chroma_l1 (U, then V over it in the same planes: V's result is read), under the production launch and both
    forced slice orders.  Pictures of 2 x 2 pixel blocks of the two corner colours whose V bytes are the colour stage's extremes, in the worst-case
    pattern: the 4:2:0 plane the front leaves is the oracle's, which is that pattern smoothed; then the patterns themselves (V's extremes,
    U's, 0 / 255) written into the V byte plane."""
    import torch
    q = 20
    (ulo, uhi, _, _), (vlo, vhi, vlo_c, vhi_c) = colour_extremes(oracle, q)
    pats = byte_patterns(vlo, vhi)
    imgs = np.stack([np.where((p == vhi)[:, :, None], np.array(CORNER[vhi_c], np.uint8), np.array(CORNER[vlo_c], np.uint8)).astype(np.uint8).repeat(2, 0).repeat(2, 1) for p in pats])
    n = len(imgs)
    h = Hook(n)
    h.e.lib.nhw_stage_chroma_l1.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]

    def check(tag, planes):
        assert h.e.lib.nhw_stage_chroma_l1(h.e.h, n, None) == 0
        torch.cuda.synchronize()
        for i, p in enumerate(planes):
            oj, op = oracle.analysis(p.astype(np.int16), 256, 256, 0)
            assert np.array_equal(h.read(B_CPROC, i, 2 * Q), op.ravel()), f"{tag} plane {i}: coefficients"
            assert np.array_equal(h.read(B_CLL1, i, Q // 2).reshape(128, 128), oj.reshape(256, 256)[:128, :128]), f"{tag} plane {i}: LL1"

    try:
        assert h.e.lib.nhw_debug_slice_order(h.e.h, order) == 0
        h.e.encode(imgs, q)
        vs = [oracle.color(im, q)[2].reshape(256, 256) for im in imgs]   # (the 4:2:0 stage smooths along the row -- 0 behind 255 comes out as 64 -- so no picture gives the pattern itself)
        for i in range(n):
            assert np.array_equal(h.read(B_PV, i, Q).view(np.uint8).reshape(256, 256), vs[i]), f"picture {i}: the V plane"
        check("pictures", vs)
        for tag, more in (("V's extremes", pats), ("U's extremes", byte_patterns(ulo, uhi)), ("0 / 255", byte_patterns(0, 255))):
            for i, p in enumerate(more):
                h.write(B_PV, i, p)
            check(tag, more)
    finally:
        h.e.lib.nhw_debug_slice_order(h.e.h, 0)
        h.e.close()
