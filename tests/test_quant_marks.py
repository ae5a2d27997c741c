"""The hand-over of the second dequantiser simulation's marks to the luma quantiser (pytest -m gpu).

Above quality 16 the quantiser's loops 2 and 3 (triples and vertical pairs of +-4..7, equal-sign 5..7 pairs; image_processing.c:241-309) are the
second simulation's two marking blocks (:2759-2905) on the same cells: the simulation leaves their outcome in the quantiser's alphabet in a free
plane (B_KMAP) and the quantiser reads the level-2 details from there, row 255 excepted (wave_dequant_details, nhwcodec_amd/csrc/nhw_tail_wave.h).

  * crafted level-2 planes behind nhw_stage_quant (include/nhw_hip_debug.h): form 0 (simulation + hand-over + quantiser) against form 1 (the
    quantiser alone with its own loops, the form the parity tests pin to the oracle): non-zero maps, fbase and value lists byte for byte;
  * reach: form 1's lists hold every symbol loop 4 makes of a mark, and marks lie in rows 254 and 255;
  * whole files, 64 images (suite seeds + mark-dense textures) at six qualities: the default handle against one made under NHW_QUANT_MARKS=0,
    the textures also against the oracle; the same under both forced slice orders; with the hand-over plane filled with a byte pattern between
    the batches of one handle;
  * under a debug stop the batch does not write the hand-over plane.
"""
import ctypes
import os

import numpy as np
import pytest

from tests.enc_stages import B_L2SAVE, B_PROC, Q, oracle_files, ws_index

B_KMAP, B_NZQ, B_VALS = ws_index("KMAP"), ws_index("NZQ"), ws_index("VALS")
HOOK_QUALITIES = (17, 20, 23)
FILE_QUALITIES = (17, 18, 20, 21, 22, 23)
N_FILES, N_DENSE = 64, 16
# loop 4 above quality 16 (wave_quantise_luma, image_processing.c:314-519): the symbol of a cell that loops 2 and 3 have marked
MARK_SYMBOL = {12700: 127, 12900: 129, 12100: 121, 12200: 122, 10300: 126, 10204: 125}   # (10100, the cells a mark silences, takes the zero symbol 128)
MARK_SYMBOLS = sorted(MARK_SYMBOL.values())


# ---------------------------------------------------------------------------------------------- crafted planes
def _run(b, r, c, vals):
    vals = np.asarray(vals, np.int16)
    n = min(len(vals), b.shape[1] - c)
    b[r, c:c + n] = vals[:n]


def _cycle(n, sign, start=0, lo=4):
    """n values of 4..7 (lo = 5: 5..7) in turn, of one sign"""
    span = 8 - lo
    return [sign * (lo + (start + i) % span) for i in range(n)]


def crafted_planes(variant):
    """-> (block [256,256], plane [512,512]): the level-2 block as l2save holds it, and the work plane around it (the block's copy in it with the
    LL2 quarter's cells up to 8000 cleared, as Y26 leaves it above quality 21; HL1's first row under row 255; small level-1 details)"""
    rng = np.random.default_rng(4100 + variant)
    b = np.zeros((256, 256), np.int16)
    edge = (3, 4, 7, 8)
    # the lower half: a row per run length, both signs, starts on even and odd columns, the predicates' edge values on either side
    r = 130
    for n in range(2, 10):
        for lo in (4, 5):
            c = 3 + (variant & 1)
            k = 0
            while c + n + 3 < 250:
                sign = 1 if (k & 1) == 0 else -1
                left, right = edge[(k + variant) & 3] * sign, edge[(k + n + variant) & 3] * sign
                if (k >> 1) & 1: left, right = -left, 0
                b[r, c - 1] = left
                _run(b, r, c, _cycle(n, sign, k, lo))
                b[r, c + n] = right
                c += n + 3 + ((k + n) & 1)                        # the next start changes parity now and then
                k += 1
            r += 1
    # stacked vertical pairs, three to six rows, beside runs that start inside the columns a mark of the row above silences
    r = 148
    for h in (3, 4, 5, 6):
        for k, c in enumerate(range(4 + variant % 3, 240, 17)):
            sign = -1 if (k + variant) & 1 else 1
            for i in range(h):
                _run(b, r + i, c, _cycle(2, sign, i + k))
            _run(b, r + 1, c + 2, _cycle(2 + k % 5, sign, k))      # row r + 1: the pair's cells are marked, a run of the raw row starts on them
            _run(b, r + 2, c + 1 + (k & 1), _cycle(3 + k % 4, sign, k, 5))
        r += h + 1
    # the same across the seam between the halves (rows 126..129) and at the bottom (rows 252..255)
    for r0 in (126, 252):
        for k, c in enumerate(range(129 if r0 == 126 else 1, 250, 11)):
            sign = -1 if k & 1 else 1
            kind = (k + variant) % 4
            if kind == 0:                                             # a pair over all four rows
                for i in range(4): _run(b, r0 + i, c, _cycle(2, sign, i))
            elif kind == 1:                                           # triples and longer in every row, staggered
                for i in range(4): _run(b, r0 + i, c + (i & 1), _cycle(3 + (i + k) % 4, sign, k))
            elif kind == 2:                                           # a pair in the last two rows only
                for i in (2, 3): _run(b, r0 + i, c, _cycle(2, sign, k, 5))
            else:                                                     # pairs of 5..7 behind a triple
                for i in range(4): _run(b, r0 + i, c, _cycle(3, sign, i) + _cycle(2, sign, k, 5))
    # runs touching the block's edges and the columns round 128
    for i, (r, c, n) in enumerate(((200, 0, 2), (201, 0, 3), (202, 1, 2), (203, 1, 4), (204, 125, 6), (205, 127, 2), (206, 127, 3), (207, 128, 2), (208, 126, 5),
                                   (209, 253, 3), (210, 254, 2), (211, 252, 4), (212, 251, 5), (213, 0, 9), (214, 247, 9),
                                   (40, 128, 2), (41, 128, 3), (42, 129, 2), (43, 129, 3), (44, 130, 4), (45, 253, 3), (46, 254, 2), (47, 252, 4), (48, 128, 9), (49, 247, 9))):
        _run(b, r, c, _cycle(n, -1 if (i + variant) & 1 else 1, i, 4 + (i & 1)))
    for r in (40, 41, 42, 43, 48, 126, 127):                          # vertical pairs of the upper half under some of them
        if r + 1 < 128 or r >= 126:
            b[r + 1, 128:131] = np.where(b[r, 128:131] != 0, b[r, 128:131], b[r + 1, 128:131])
    # the upper half's HL2 rows: the lower half's run rows once more, shifted to columns 128 and up
    for i, r in enumerate(range(60, 76)):
        _run(b, r, 129 + (i & 1), b[130 + i, 3:125])
    # 5..7 pairs directly behind a triple and behind a vertical pair
    for k, c in enumerate(range(6, 240, 13)):
        sign = -1 if k & 1 else 1
        _run(b, 218, c, _cycle(3, sign, k) + _cycle(2, sign, k, 5))
        _run(b, 220, c, _cycle(2, sign, k)); _run(b, 221, c, _cycle(2, sign, k + 1)); _run(b, 220, c + 3, _cycle(2, sign, k, 5))
        _run(b, 221, c + 2, _cycle(2, sign, k, 5))
    # the walk's +-8 rewrites inside marked rows: a +-7 beside a loud x6 / x7 and beside an 8 -- the quantiser must see the 7
    for k, c in enumerate(range(4, 230, 19)):
        for r, loud in ((224, 14), (225, 15), (226, 22), (227, 8)):
            b[r, c], b[r, c + 1] = loud, 7
            b[r, c + 3], b[r, c + 4] = -loud if loud != 8 else 8, -7
            b[r, c + 6], b[r, c + 7] = -7, 8
            _run(b, r, c + 9, _cycle(3 + k % 3, -1 if k & 1 else 1, k))
            b[r, c + 8] = 7 if k & 2 else -7                          # a 7 that is also the cell left of a run
    # LL2 cells just below and just above 8000 beside column 128, HL2 runs starting at column 128
    for i, v in enumerate((7999, 8000, 8001, 16007, 5, 6, -5, 0)):
        b[20 + i, 126], b[20 + i, 127] = v, (v if i & 1 else 5)
        _run(b, 20 + i, 128, _cycle(2 + i % 3, -1 if v == -5 else 1, i))
    b[:128, :128] = np.where(b[:128, :128] == 0, rng.integers(0, 256, (128, 128)).astype(np.int16), b[:128, :128])   # LL2 samples (untagged: up to 8000)
    b[10:14, 100:128] += np.int16(16000)                              # a patch of tagged ones
    # random marks over what is still empty: dense small values, every neighbourhood of the predicates by chance
    free = b[128:, :] == 0
    free[2:120, :] = False                                            # (rows 130 .. 247 hold the structured part)
    vals = np.array([-8, -7, -6, -5, -4, -3, 0, 3, 4, 5, 6, 7, 8, 14, -14], np.int16)
    prob = np.array([3, 8, 10, 10, 8, 4, 12, 4, 8, 10, 10, 8, 3, 1, 1], float)
    noise = rng.choice(vals, (128, 256), p=prob / prob.sum())
    keep = np.repeat(rng.random((128, 32)) < 0.55, 8, 1)              # in patches of one sign each: runs need neighbours of one sign
    sgn = np.repeat(np.where(rng.random((128, 32)) < 0.5, -1, 1), 8, 1).astype(np.int16)
    noise = np.where(np.abs(noise) < 9, np.abs(noise) * sgn, noise).astype(np.int16)
    b[128:, :] = np.where(free & keep, noise, b[128:, :])
    top_free = b[76:126, 128:] == 0
    b[76:126, 128:] = np.where(top_free, noise[:50, 128:], b[76:126, 128:])
    plane = np.zeros((512, 512), np.int16)
    # level-1 details: mostly inside the dead zone, some pairs on multiples of 8 (loop 1), some large values
    d = rng.choice(np.array([0, 0, 0, 0, 0, 2, -3, 5, -6, 7, -7, 8, 16, 24, -8, -16, 15, -15, 40, -50, 200, -300], np.int16), (512, 512))
    plane[:] = d
    plane[:256, :256] = b
    ll = plane[:128, :128]
    ll[ll <= 8000] = 0
    # HL1's first row under row 255: in and out of 4..7 under the pairs of row 255
    under = b[255].copy()
    flip = (np.arange(256) // 6 + variant) % 3
    plane[256, :256] = np.where(flip == 0, under, np.where(flip == 1, 0, np.where(under > 0, 8, -3))).astype(np.int16)
    return b, plane


def loops_2_3(block, row256):
    """the marks loops 2 and 3 leave in the level-2 block, as the reference walks them (image_processing.c:241-309): -> block of int32"""
    v = np.zeros((257, 256), np.int32)
    v[:256] = block
    v[256] = row256
    ll = v[:128, :128]
    ll[ll <= 8000] = 0
    P = lambda x: 4 <= x <= 7
    N = lambda x: -7 <= x <= -4
    for r in range(256):
        j = 1
        while j < 255:
            a = v[r]
            for T, t_c, v_l in ((P, 12700, 12100), (N, 12900, 12200)):
                if T(a[j - 1]) and T(a[j]):
                    if T(a[j + 1]):
                        a[j - 1], a[j] = 10100, t_c
                        j += 1
                        break
                    if T(v[r + 1, j - 1]) and T(v[r + 1, j]):
                        a[j - 1], a[j] = v_l, 10100
                        v[r + 1, j - 1] = v[r + 1, j] = 10100
                        j += 1
                        break
            j += 1
        j = 0
        while j < 255:
            a = v[r]
            if 5 <= a[j] <= 7 and 5 <= a[j + 1] <= 7: a[j] = 10300; j += 1
            elif -7 <= a[j] <= -5 and -7 <= a[j + 1] <= -5: a[j] = 10204; j += 1
            j += 1
    return v[:256]


N_CRAFTED = 6

_crafted = {}


def crafted(n):
    if n not in _crafted:
        _crafted[n] = [crafted_planes(k) for k in range(n)]
    return _crafted[n]


def test_crafted_planes_hold_what_they_promise():
    """the inputs of the hook test, checked on the CPU with a cell-by-cell walk of loops 2 and 3: every mark of the alphabet, marks in rows 126..129
    and 252..255, stacked vertical pairs, runs at the block's edges"""
    total = {m: 0 for m in list(MARK_SYMBOL) + [10100]}
    rows = set()
    for b, plane in crafted(N_CRAFTED):
        m = loops_2_3(b, plane[256, :256])
        for k in total: total[k] += int((m == k).sum())
        rows |= set(np.flatnonzero(np.isin(m, list(MARK_SYMBOL)).any(1)).tolist())
        for c in (0, 1, 128, 129, 253, 254):
            assert np.isin(m[:, c], list(total)).any(), f"no mark in column {c}"
        stacked = (m[:-2] == 12100) & (m[1:-1] == 10100) & (m[2:] == 12100) | (m[:-2] == 12200) & (m[1:-1] == 10100) & (m[2:] == 12200)
        assert stacked.any(), "no vertical pair two rows under another"
    assert all(total.values()), total
    assert {126, 127, 128, 129, 252, 253, 254, 255} <= rows, sorted(rows)


# ---------------------------------------------------------------------------------------------- images
def texture(i):
    """a low-contrast texture of period 4 or 8 under a slow envelope: level-2 details of 4..7 in long runs"""
    rng = np.random.default_rng(9100 + i)
    y, x = np.mgrid[0:512, 0:512]
    amp, per, kind = 3 + 2 * (i % 8), (4, 8)[(i // 8) % 2], i % 3
    if kind == 0: w = np.sin(2 * np.pi * x / per)
    elif kind == 1: w = np.sin(2 * np.pi * y / per)
    else: w = np.sin(2 * np.pi * x / per) * np.sin(2 * np.pi * y / per)
    env = 0.5 + 0.5 * np.sin(2 * np.pi * (x + 2 * y) / (96 + 16 * (i % 5)))
    g = 128 + amp * w * env + rng.normal(0, 1.0 + 0.3 * (i % 4), (512, 512))
    g = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return np.stack([g, g, g], -1)


_images = {}


def images():
    """64 pictures: 48 of the suite's generator, 16 mark-dense textures (the last 16)"""
    if "a" not in _images:
        from oracle.oraclepy import Oracle
        o = Oracle()
        _images["a"] = np.stack([o.synth(83000 + i) for i in range(N_FILES - N_DENSE)] + [texture(i) for i in range(N_DENSE)])
    return _images["a"]


def test_textures_are_mark_dense():
    """on the CPU: the oracle's quantised plane of the textures holds every mark symbol, hundreds of them"""
    from oracle.oraclepy import Oracle
    o = Oracle()
    count = {s: 0 for s in MARK_SYMBOLS}
    for i in (3, 6, 9, 12, 15):
        _, tr = o.encode(texture(i), 20, trace=True)
        p = np.frombuffer(dict(tr)["offsetY"][0], np.int16).reshape(512, 512)[:256, :256]
        for s in count: count[s] += int((p == s).sum())
    assert min(count.values()) >= 40 and sum(count.values()) >= 2000, count


# ---------------------------------------------------------------------------------------------- GPU part
def _read(e, buf, i, nbytes):
    out = np.empty(nbytes, np.uint8)
    assert e.lib.nhw_debug_read(e.h, buf, i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(nbytes)) == 0
    return out


def _write(e, buf, i, a):
    a = np.ascontiguousarray(a)
    assert e.lib.nhw_debug_write(e.h, buf, i, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0


def _fill(e, byte, n, nbytes=2 * Q):
    assert e.lib.nhw_debug_fill(e.h, B_KMAP, byte, ctypes.c_size_t(nbytes), n) == 0


def symbol_list(e, i):
    """(non-zero map [32 flushes, 128 strips], fbase [33], the values) of image i as the quantiser left them"""
    raw = _read(e, B_NZQ, i, 4096 * 8 + 33 * 4)
    nzq, fbase = raw[:4096 * 8].view(np.uint64).reshape(32, 128), raw[4096 * 8:].view(np.uint32)
    total = int(fbase[32])
    assert total <= 4 * Q
    vals = _read(e, B_VALS, i, (total + 1) & ~1)[:total]
    return nzq.copy(), fbase.copy(), vals.copy()


def dense_symbols(nzq, fbase, vals):
    """the list as a plane of symbols: bit 4 i + k of (flush f, strip s) is row 16 f + i, column 4 s + k, odd rows mirrored inside the strip"""
    bits = np.unpackbits(nzq.reshape(-1).view(np.uint8), bitorder="little").astype(bool).reshape(32, 128, 64)
    f, s, b = np.nonzero(bits)                                        # flush after flush, strip after strip, a slice in stream order: the list's order
    assert len(f) == len(vals) == int(fbase[32])
    row, k = 16 * f + (b >> 2), b & 3
    out = np.full((512, 512), 128, np.uint8)
    out[row, 4 * s + np.where(row & 1, 3 - k, k)] = vals
    return out


def run_hook(e, form, planes):
    import torch
    for i, (b, plane) in enumerate(planes):
        _write(e, B_L2SAVE, i, b)
        _write(e, B_PROC, i, plane)
    _fill(e, 0x27 if form == 0 else 0xD8, len(planes), 8 * Q)        # what an earlier batch may have left in the hand-over plane: any bytes
    assert e.lib.nhw_stage_quant(e.h, len(planes), form, None) == 0, "nhw_stage_quant"
    torch.cuda.synchronize()
    return [symbol_list(e, i) for i in range(len(planes))]


@pytest.mark.gpu
@pytest.mark.parametrize("q", HOOK_QUALITIES)
def test_crafted_planes_quantise_alike(q):
    """form 1 (the quantiser's own loops: the parent's kernel path, pinned to the oracle by the parity tests) is the reference for form 0"""
    import nhwcodec_amd
    planes = crafted(N_CRAFTED)
    n = len(planes)
    e = nhwcodec_amd.Encoder(0, max_batch=n)
    try:
        e.encode(images()[:n], q)                                   # the hook works at the quality of the handle's last whole batch
        own = run_hook(e, 1, planes)
        handed = run_hook(e, 0, planes)
    finally:
        e.close()
    seen = set()
    rows = set()
    for i, ((b, plane), (nzq1, fb1, v1), (nzq0, fb0, v0)) in enumerate(zip(planes, own, handed)):
        sym = dense_symbols(nzq1, fb1, v1)
        # the reference is what the reference's loops make of the plane: the marks of the cell-by-cell walk, through loop 4's table
        m = loops_2_3(b, plane[256, :256])
        for mark, s in MARK_SYMBOL.items():
            at = m == mark
            assert (sym[:256, :256][at] == s).all(), f"q{q} image {i}: form 1 does not code every {mark} as {s}"
        assert not np.isin(sym[:256, :256][~np.isin(m, list(MARK_SYMBOL))], MARK_SYMBOLS).any(), f"q{q} image {i}: form 1 has a mark symbol where the walk leaves no mark"
        seen |= set(np.unique(v1).tolist()) & set(MARK_SYMBOLS)
        rows |= set(np.flatnonzero(np.isin(sym[:256, :256], MARK_SYMBOLS).any(1)).tolist())
        assert np.array_equal(nzq0, nzq1), f"q{q} image {i}: non-zero maps differ in {np.argwhere(nzq0 != nzq1)[:6].tolist()} (flush, strip)"
        assert np.array_equal(fb0, fb1), f"q{q} image {i}: fbase differs"
        assert v0.tobytes() == v1.tobytes(), f"q{q} image {i}: value lists differ, first at {np.flatnonzero(v0 != v1)[:6].tolist()}"
    assert seen == set(MARK_SYMBOLS), f"q{q}: form 1's lists lack the symbols {sorted(set(MARK_SYMBOLS) - seen)}"
    assert 254 in rows and 255 in rows, f"q{q}: no mark in row 254 or in row 255 (rows with marks end at {max(rows)})"


_files = {}


def default_files(q):
    """the default handle's files of the 64 pictures at quality q: made once, shared"""
    if q not in _files:
        import nhwcodec_amd
        e = nhwcodec_amd.Encoder(0, max_batch=N_FILES)
        try:
            _files[q] = e.encode(images(), q)
            marks = sum(int(np.isin(symbol_list(e, i)[2], MARK_SYMBOLS).sum()) for i in range(N_FILES - N_DENSE, N_FILES))
        finally:
            e.close()
        assert marks >= 1000, f"q{q}: the textures' symbol lists hold only {marks} mark symbols"
    return _files[q]


def handle_with_own_loops(n):
    """a handle made under NHW_QUANT_MARKS=0 (the switch is read when a handle is made)"""
    import nhwcodec_amd
    old = os.environ.get("NHW_QUANT_MARKS")
    os.environ["NHW_QUANT_MARKS"] = "0"
    try:
        return nhwcodec_amd.Encoder(0, max_batch=n)
    finally:
        if old is None: del os.environ["NHW_QUANT_MARKS"]
        else: os.environ["NHW_QUANT_MARKS"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("q", FILE_QUALITIES)
def test_files_with_and_without_the_hand_over(q):
    got = default_files(q)
    e = handle_with_own_loops(N_FILES)
    try:
        own = e.encode(images(), q)
    finally:
        e.close()
    bad = [i for i in range(N_FILES) if got[i] != own[i]]
    assert not bad, f"q{q}: files {bad[:16]} differ between the hand-over and the quantiser's own loops"
    want = oracle_files(images()[N_FILES - N_DENSE:], q)
    bad = [i for i in range(N_DENSE) if got[N_FILES - N_DENSE + i] != want[i]]
    assert not bad, f"q{q}: the files of textures {bad} differ from the oracle's"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("q", FILE_QUALITIES)
def test_files_under_forced_slice_orders(q, mode):
    """the hand-over crosses a kernel boundary: kernels that split an item run slice after slice, ascending and descending"""
    import nhwcodec_amd
    want = default_files(q)
    e = nhwcodec_amd.Encoder(0, max_batch=N_FILES)
    try:
        assert e.lib.nhw_debug_slice_order(e.h, mode) == 0
        got = e.encode(images(), q)
    finally:
        e.close()
    bad = [i for i in range(N_FILES) if got[i] != want[i]]
    assert not bad, f"q{q} slice order {mode}: files {bad[:16]} differ"


@pytest.mark.gpu
@pytest.mark.parametrize("q", (20, 23))
def test_left_over_bytes_in_the_hand_over_plane(q):
    """one handle, two batches, the plane filled with a byte pattern in front of each: the quantiser reads only cells that the simulation of the
    same batch wrote"""
    import nhwcodec_amd
    want = default_files(q)
    imgs = images()
    e = nhwcodec_amd.Encoder(0, max_batch=N_FILES)
    try:
        _fill(e, 0xA5, N_FILES, 8 * Q)
        first = e.encode(imgs, q)
        _fill(e, 0x05, N_FILES, 8 * Q)
        second = e.encode(imgs[::-1], q)
        _fill(e, 0x00, N_FILES, 8 * Q)
        third = e.encode(imgs, q)
    finally:
        e.close()
    assert first == want and third == want and second == want[::-1]


@pytest.mark.gpu
def test_a_debug_stop_leaves_the_hand_over_plane_alone():
    """the stage checks read the quantiser's own work plane: under nhw_debug_stop_after neither kernel takes part in the hand-over"""
    import torch
    import nhwcodec_amd
    n, q = 4, 20
    e = nhwcodec_amd.Encoder(0, max_batch=n)
    d_in = torch.from_numpy(images()[N_FILES - n:]).cuda()
    try:
        for stage in (11, 13):                                      # behind the second simulation; behind the quantiser and Y31
            _fill(e, 0xA5, n, 8 * Q)
            e.lib.nhw_debug_stop_after(e.h, stage)
            e.encode_device(d_in, q)
            torch.cuda.synchronize()
            for i in range(n):
                assert (_read(e, B_KMAP, i, 2 * Q) == 0xA5).all(), f"stage {stage} image {i}: the batch wrote the hand-over plane under a debug stop"
        e.lib.nhw_debug_stop_after(e.h, 0)
        files = e.encode(images()[N_FILES - n:], q)
        assert not (_read(e, B_KMAP, 0, 2 * Q)[Q:] == 0xA5).all(), "a whole batch hands the marks over"
    finally:
        e.lib.nhw_debug_stop_after(e.h, 0)
        e.close()
    assert files == default_files(q)[N_FILES - n:]
