"""The stores of the luma level-2 block that a production batch leaves out: the transposed first-direction plane of both level-2
analyses in B_JPEG, and rows 128 .. 255 of the second analysis' block in B_PROC.  They rest on one claim -- a dequantiser simulation writes every cell
of the level-2 block of B_JPEG (the case list at wave_dequant_details, nhw_tail_wave.h) -- and on the LL2 emission being the one reader of the block of
B_PROC.  What is checked, on eight pictures of one tile (four of the generator's, four crafted ones whose level-2 details are dense in +-4 .. 8, so that
triples, vertical pairs and equal-sign pairs touch each other and the edges of the bands):
  * two production batches over planes filled with 0x7F and then 0x80, behind a batch as in a long-running encoder: the files are the oracle's.  A cell
    read without having been written in its batch differs under at least one fill.  Above quality 16 the marks the second simulation handed the
    quantiser (B_KMAP) must show every kind of mark, cover 1 % of the detail cells of a picture and reach the last rows and columns of the bands;
  * the claim itself, cell by cell: the block of B_JPEG filled with 0x7F7F in front of either simulation as a batch launches it (nhw_stage_luma_loop
    form 6, nhw_stage_ll2_walk forms 0 and 1) holds no 0x7F7F behind it, and what the batch's kernels leave where they still store is what the
    all-storing forms leave;
  * that the stores are gone from the batch's form of the fused kernel and still made by the hook's (forms 7 and 1).  At the END of a batch the block of
    either plane holds no fill whichever form ran (k_dwt_syn behind the second simulation rewrites the block of B_PROC, the simulations and the
    residual passes that of B_JPEG), so the cells are looked at directly behind the kernel."""
import ctypes

import numpy as np
import pytest

from tests.enc_stages import B_JPEG, B_PROC, Q, Hook, ws_index

B_KMAP = ws_index("KMAP")
QUALITIES = (7, 12, 13, 17, 20, 21, 23)          # 7 and 12: the first analysis' plane is left out there too (the first simulation has no marks below 17)
FILL = 0x7F7F
N = 8
MARKS = {"triple centre": (12700, 12900), "left of a triple / under a vertical pair": (10100,), "left of a vertical pair": (12100, 12200),
         "equal-sign pair": (10300, 10204)}
TEXTURES = (("h", 8, 4), ("v", 8, 4), ("c", 8, 4), ("sq", 8, 4), ("sqh", 8, 4), ("h", 12, 9), ("v", 12, 9), ("c", 6, 4), ("c", 12, 9), ("sq", 4, 2),
            ("sqh", 4, 2), ("v", 6, 4), ("h", 6, 4), ("sq", 16, 4), ("sqh", 16, 4), ("c", 12, 13))   # (kind, period, amplitude): each leaves many level-2 details in +-4 .. 7 at quality 17 .. 23


# ---------------------------------------------------------------------------------------------- the pictures
def texture(kind, p, yy, xx, ph):
    s = lambda t: np.sin(2 * np.pi * t / p + ph)
    if kind == "v": return s(xx)
    if kind == "h": return s(yy)
    if kind == "c": return s(xx) * s(yy)
    return np.sign(s(xx if kind == "sq" else yy) + 1e-9)


def mosaic(seed, tile, noise):
    """tiles of TEXTURES at random phases plus noise: runs of every length that end at tile seams, the picture's borders among them"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:512, 0:512]
    t = np.zeros((512, 512))
    for ty in range(0, 512, tile):
        for tx in range(0, 512, tile):
            kind, p, a = TEXTURES[rng.integers(len(TEXTURES))]
            sl = (slice(ty, ty + tile), slice(tx, tx + tile))
            t[sl] = a * texture(kind, p, yy[sl], xx[sl], rng.uniform(0, 6.28))
    return t + rng.integers(-noise, noise + 1, (512, 512))


def crafted():
    """four grey pictures: low-amplitude textures of period 4 .. 16 pixels over a ramp"""
    yy, xx = np.mgrid[0:512, 0:512]
    ramp = 48 + (xx + yy) * (150 / 1022)
    s = lambda t, p: np.sin(2 * np.pi * t / p + 0.1)
    ts = (4 * np.sign(s(xx, 8) + 1e-9),                              # one band full of long runs: triples and equal-sign pairs side by side
          6 * s(yy, 8) * s(xx, 40) + 6 * s(xx, 8) * s(yy, 40),       # two bands, the runs' lengths change slowly
          mosaic(7703, 64, 2), mosaic(7702, 16, 1))
    return [np.repeat(np.clip(np.rint(ramp + t), 0, 255).astype(np.uint8)[:, :, None], 3, 2) for t in ts]


_cache = {}


def pictures():
    if "imgs" not in _cache:
        from oracle.oraclepy import Oracle
        o = Oracle()
        _cache["imgs"] = np.stack([o.synth(64000 + i) for i in range(4)] + crafted())
    return _cache["imgs"]


def oracle_files(q):
    if q not in _cache:
        from oracle.oraclepy import Oracle
        o = Oracle()
        _cache[q] = [o.encode(im, q) for im in pictures()]
    return _cache[q]


def block(plane):
    return plane.reshape(512, 512)[:256, :256]


def with_block(plane, value):
    a = plane.reshape(512, 512).copy()
    a[:256, :256] = value
    return a.ravel()


# ---------------------------------------------------------------------------------------------- whole batches
@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_files_over_two_fills_are_the_oracles(q):
    imgs, want = pictures(), oracle_files(q)
    h = Hook(N)
    try:
        h.e.lib.nhw_debug_fill.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int]
        h.e.encode(imgs, q)                                         # a batch before, as in a long-running encoder
        for byte in (0x7F, 0x80):
            for buf in (B_JPEG, B_PROC):
                assert h.e.lib.nhw_debug_fill(h.e.h, buf, byte, 8 * Q, N) == 0
            got = h.e.encode(imgs, q)
            bad = [i for i in range(N) if got[i] != want[i]]
            assert not bad, f"q{q}, planes filled with {byte:#x}: files {bad} differ from the oracle"
        if q < 17:
            return
        # what the second simulation handed the quantiser: rows of 256 cells, the detail cells of the level-2 block
        km = np.stack([h.read(B_KMAP, i, 2 * Q).reshape(256, 256) for i in range(N)])
        after = [block(h.read(b, i, 8 * Q)) for b in (B_JPEG, B_PROC) for i in range(N)]
    finally:
        h.e.close()
    det = np.ones((256, 256), bool)
    det[:128, :128] = False
    marked = np.zeros(km.shape, bool)
    for name, values in MARKS.items():
        m = np.isin(km, values) & det
        print(f"q{q} {name}: {m.reshape(N, -1).sum(1).tolist()} cells a picture")
        assert m.any(), f"q{q}: no mark of kind '{name}' {values} in any picture"
        marked |= m
    share = marked.reshape(N, -1).sum(1) / det.sum()
    print(f"q{q} marked share of the detail cells, a picture: {np.round(share, 4).tolist()}")
    assert share.max() >= 0.01, f"q{q}: the marks cover {share.max():.4f} of the detail cells at most"
    edges = {"rows 126, 127": marked[:, 126:128, 128:], "rows 254, 255": marked[:, 254:], "columns 253 .. 255": marked[:, :, 253:]}
    for name, m in edges.items():
        print(f"q{q} marks in {name}: {int(m.sum())}")
        assert m.any(), f"q{q}: no mark reaches {name}"
    assert not any((a == FILL).any() for a in after), f"q{q}: the level-2 block of a plane holds the fill at the end of the batch"


# ---------------------------------------------------------------------------------------------- the claim, cell by cell
def run_walk(h, form):
    import torch
    assert h.e.lib.nhw_stage_ll2_walk(h.e.h, h.n, form, None) == 0, "nhw_stage_ll2_walk"
    torch.cuda.synchronize()
    return [h.read(B_JPEG, i, 8 * Q) for i in range(h.n)]


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_a_simulation_writes_every_cell_of_the_block(q):
    h = Hook(N)
    try:
        h.e.encode(pictures(), q)
        left = [[with_block(p[0], FILL)] + p[1:3] + [np.zeros(Q, np.int16)] for p in h.planes()]   # what the batch left, the block of B_JPEG filled
        full = h.run(0, left)
        lean = h.run(6, left)
        for i, (a, b) in enumerate(zip(lean, full)):
            tag = f"q{q} image {i}, the batch's launches (form 6) against the all-storing ones (form 0):"
            assert (a[2] == b[2]).all() and (a[3] == b[3]).all(), f"{tag} B_LL1 or B_L2SAVE differ"
            pa, pb = a[1].reshape(512, 512).copy(), b[1].reshape(512, 512).copy()
            ja, jb = a[0].reshape(512, 512).copy(), b[0].reshape(512, 512).copy()
            if q > 12:                                              # the cells the batch's fused kernel leaves: compared with what stood there instead
                assert not (block(a[0]) == FILL).any(), f"{tag} the first simulation left {(block(a[0]) == FILL).sum()} cells of the block unwritten"
                pa[128:256, :256] = pb[128:256, :256] = 0
                ja[:256, :256] = jb[:256, :256] = 0
            assert (pa == pb).all() and (ja == jb).all(), f"{tag} B_PROC or B_JPEG differ where both store"
        if q <= 12:
            return                                                  # (no second closed loop; the first simulation's plane is rewritten by the analysis behind k_l2_recon<false>)
        for form in (0, 1):                                         # the forked order's pair of kernels, the in-line order's
            h.run(0, left)
            want = run_walk(h, form)
            out = h.run(6, left)
            for i, p in enumerate(out):
                h.write(B_JPEG, i, with_block(p[0], FILL))
            got = run_walk(h, form)
            for i in range(N):
                assert not (block(got[i]) == FILL).any(), f"q{q} walk form {form} image {i}: the second simulation left {(block(got[i]) == FILL).sum()} cells unwritten"
                assert (got[i] == want[i]).all(), f"q{q} walk form {form} image {i}: B_JPEG behind the second simulation depends on what stood in the block"
    finally:
        h.e.close()


# ---------------------------------------------------------------------------------------------- the stores are gone, and the hook's forms keep them
@pytest.mark.gpu
@pytest.mark.parametrize("q", (13, 20))
def test_the_batchs_fused_kernel_leaves_the_cells_alone(q):
    h = Hook(N)
    try:
        h.e.encode(pictures(), q)
        left = [p[:3] + [np.zeros(Q, np.int16)] for p in h.planes()]
        sim1 = h.run(6, left)                                       # B_JPEG: the first simulation's plane (the batch's fused kernel does not store there)
        inputs = [[p[0], with_block(p[1], FILL), p[2], np.zeros(Q, np.int16)] for p in sim1]
        lean = h.run(7, inputs)
        full = h.run(1, inputs)
    finally:
        h.e.close()
    for i in range(N):
        tag = f"q{q} image {i}:"
        jin = inputs[i][0].reshape(512, 512)
        jl, jf = lean[i][0].reshape(512, 512), full[i][0].reshape(512, 512)
        pl, pf = lean[i][1].reshape(512, 512), full[i][1].reshape(512, 512)
        sl, sf = lean[i][3].reshape(256, 256), full[i][3].reshape(256, 256)
        assert (sl == sf).all() and (lean[i][2] == full[i][2]).all(), f"{tag} B_L2SAVE or B_LL1 differ between forms 7 and 1"
        assert sf.any()
        assert (jl == jin).all(), f"{tag} the batch's form stores into B_JPEG"
        assert (block(jf) != block(jin)).any() and not (block(jf) == FILL).any(), f"{tag} the hook's form does not store the block of B_JPEG"
        assert (pf[:256, :256] == sf).all(), f"{tag} the hook's form does not store the whole block of B_PROC"
        assert (pl[:128, :256] == sl[:128]).all(), f"{tag} rows 0 .. 127 of the block of B_PROC (the LL2 emission reads them)"
        assert (pl[128:256, :256] == np.int16(FILL)).all(), f"{tag} the batch's form stores rows 128 .. 255 of the block of B_PROC"
        pl, pf = pl.copy(), pf.copy()
        pl[:256, :256] = pf[:256, :256] = 0
        jf = jf.copy(); jf[:256, :256] = jin[:256, :256]
        assert (pl == pf).all() and (jf == jin).all(), f"{tag} a cell outside the block is written"
