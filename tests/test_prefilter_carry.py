"""GPU tests of the carry paths of the pre-filter's pass A on the pictures of tests/prefilter_cases.py (P1 .. P4): bands that go back to row 0 or
stop in the middle, rows whose open lanes take their state from the lane on their left, and the same beside noise.
tests/test_prefilter_census.py asserts on the CPU that the pictures reach those paths and that a wrong state on them changes map cells; here the
kernels run on them.  Every expected value is the oracle's (oracle/nhwo_prelow.c, opened up by tests/low_machine/oracle_side.c; oracle.encode).

The stage tests compare the CONTRAST MAP and the FLAG PLANE as the kernels leave them in the workspace (B_PROC, B_SCAN), not only the filtered
picture: a wrong carry moves map cells by one, and on these pictures none of them crosses a threshold a later pass tests, so the
filtered picture alone would pass.  Compared: every cell of rows 1 .. 510, columns 1 .. 510 -- all the cells pass A has; no cell is excluded.  The
border cells are not pass A's: the oracle keeps zeros there, row 0 of the flag plane holds k_low_apply's list of marker rows.

nhw_stage_prefilter launches the kernels with neither debug switch (it passes no force bits and opens no slice scope), so the forced go-back
and the slice orders run through the batch driver stopped behind the pre-filter (nhw_debug_stop_after 2), which honours both, from the BGR
pictures; the planes are the same three."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import prefilter_cases as pc
from tests.enc_stages import oracle_files, ws_index

pytestmark = pytest.mark.gpu

S = 512
B_PROC, B_KMAP, B_SCAN = (ws_index(n) for n in ("PROC", "KMAP", "SCAN"))
NAMES = [n for n, _ in pc.CRAFTED]


@pytest.fixture(scope="module")
def enc():
    import nhwcodec_amd
    e = nhwcodec_amd.Encoder(0, max_batch=8)
    e.lib.nhw_debug_front_fallback.argtypes = [ctypes.c_void_p, ctypes.c_int]
    e.lib.nhw_debug_stop_after.argtypes = [ctypes.c_void_p, ctypes.c_int]
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _want(q):
    """the oracle's (filtered picture, contrast map, flag plane) of P1 .. P4 at quality q"""
    return [pc.oracle_planes(y, q) for y in pc.crafted_lumas(q)]


def _read(e, buf, i, dtype):
    out = np.empty(S * S, dtype)
    assert e.lib.nhw_debug_read(e.h, buf, i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(out.nbytes)) == 0
    return out


def _compare(tag, q, filtered, maps, flags):
    bad = []
    for i, (wy, wk, ws) in enumerate(_want(q)):
        inner = lambda a: a.reshape(S, S)[1:-1, 1:-1]
        for what, g, w in (("picture", filtered[i].reshape(S, S), wy.reshape(S, S)), ("map", inner(maps[i]), inner(wk)), ("flags", inner(flags[i]), inner(ws))):
            d = np.argwhere(g != w)
            print(f"{tag} q{q} {NAMES[i]} {what}: {len(d)} cells differ")
            if len(d):
                r, c = d[0]
                bad.append(f"{NAMES[i]} {what}: {len(d)} cells, first ({r}, {c}) of the compared block: hip {g[r, c]} oracle {w[r, c]}")
    assert not bad, f"{tag} q{q}: " + "; ".join(bad)


def _stage_planes(e, q):
    import torch
    ys = np.stack([y.reshape(-1).astype(np.int16) for y in pc.crafted_lumas(q)])
    d = torch.from_numpy(ys).cuda()
    assert e.lib.nhw_stage_prefilter(e.h, d.data_ptr(), len(ys), q, None) == 0
    torch.cuda.synchronize()
    n = len(ys)
    return d.cpu().numpy(), [_read(e, B_PROC, i, np.int16) for i in range(n)], [_read(e, B_SCAN, i, np.uint8) for i in range(n)]


def _driver_planes(e, q):
    """the same planes behind the batch driver's pre-filter stage, from the BGR pictures"""
    import torch
    d = torch.from_numpy(pc.crafted_pictures(q)).cuda()
    assert e.lib.nhw_debug_stop_after(e.h, 2) == 0
    try:
        e.encode_device(d, q)
        torch.cuda.synchronize()
        n = d.shape[0]
        return ([_read(e, B_KMAP, i, np.int16) for i in range(n)], [_read(e, B_PROC, i, np.int16) for i in range(n)],
                [_read(e, B_SCAN, i, np.uint8) for i in range(n)])
    finally:
        e.lib.nhw_debug_stop_after(e.h, 0)


@pytest.mark.parametrize("q", range(1, 17))
def test_stage_leaves_the_oracles_map_and_flags(enc, q):
    """nhw_stage_prefilter on the four luma planes, one batch a quality: the filtered picture, the contrast map and the flag plane"""
    _compare("stage", q, *_stage_planes(enc, q))


@pytest.mark.parametrize("q", [1, 8, 10, 16])
def test_forced_go_back_on_top_of_a_deep_one(enc, q):
    """nhw_debug_front_fallback: every band is held back three rows more, on bands that go back 2, 3, 4 and 31 .. 481 rows of their own"""
    plain = _driver_planes(enc, q)
    _compare("driver", q, *plain)
    assert enc.lib.nhw_debug_front_fallback(enc.h, 1) == 0
    try:
        forced = _driver_planes(enc, q)
    finally:
        enc.lib.nhw_debug_front_fallback(enc.h, 0)
    _compare("forced", q, *forced)


@pytest.mark.parametrize("mode", [1, 2])
def test_slice_orders_give_the_same_planes(enc, mode):
    """the bands of k_low_pre and k_low_apply one launch each, ascending and descending (the hand-over between k_low_apply's bands)"""
    assert enc.lib.nhw_debug_slice_order(enc.h, mode) == 0
    try:
        got = _driver_planes(enc, 10)
    finally:
        enc.lib.nhw_debug_slice_order(enc.h, 0)
    _compare(f"slice order {mode}", 10, *got)


@pytest.mark.parametrize("q", [1, 6, 8, 10, 13, 16, 17, 19, 21])
def test_whole_encode_matches_oracle(enc, q):
    """the files of P1 .. P4, byte for byte; quality 17, 19, 21: the same carry inside k_front_image, with its own replay"""
    imgs = pc.crafted_pictures(q)
    got = enc.encode(imgs, q)
    o = pc._oracle()
    assert [NAMES[i] for i in range(len(imgs)) if got[i] != o.encode(imgs[i], q)] == []


@pytest.mark.parametrize("q", [10, 19])
def test_open_picture_between_ordinary_ones(enc, q):
    """P3 among six generator pictures in one batch"""
    o = pc._oracle()
    imgs = np.stack([o.synth(61000 + i) for i in range(3)] + [pc.crafted_pictures(q)[2]] + [o.synth(61003 + i) for i in range(3)])
    got = enc.encode(imgs, q)
    assert [i for i in range(7) if got[i] != o.encode(imgs[i], q)] == []


def test_sub_batches_cut_between_crafted_pictures():
    """nhw_launch_low_prefilter's sub-batch path (batches of 1024 and more): an odd batch of 1025 pictures at quality 10, six distinct ones repeated
    (P1, a generator picture, P3, noise, P4, blocks) with a crafted one on both sides of every cut that 2, 3 or 4 parts make, under
    NHW_LOW_PARTS 1 .. 4: every file equals the in-line one, the six distinct files the oracle's"""
    import torch
    import nhwcodec_amd
    from oracle.harness import class_image
    q, n = 10, 1025
    o = pc._oracle()
    p = pc.crafted_pictures(q)
    six = np.stack([p[0], o.synth(61000), p[2], class_image("noise", 1), p[3], class_image("blocks", 2)])
    order = np.arange(n) % 6
    cuts = sorted({n * k // parts for parts in (2, 3, 4) for k in range(1, parts)})
    assert cuts == [256, 341, 512, 683, 768]
    for c in cuts:
        order[c - 1], order[c] = 2, 0                                   # P3 ends a part, P1 begins the next
    assert set(order.tolist()) == set(range(6))
    bgr = torch.from_numpy(six).cuda()[torch.from_numpy(order).cuda()].contiguous()
    files = {}
    for parts in (1, 2, 3, 4):
        os.environ["NHW_LOW_PARTS"] = str(parts)
        try:
            e = nhwcodec_amd.Encoder(0, n, device_only=True)
        finally:
            del os.environ["NHW_LOW_PARTS"]
        out, sizes, status = e.encode_device(bgr, q)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        sz, a = sizes.cpu().numpy(), out.cpu().numpy()
        files[parts] = [a[i, :sz[i]].tobytes() for i in range(n)]
        e.close()
    for parts in (2, 3, 4):
        assert [i for i in range(n) if files[parts][i] != files[1][i]] == [], f"NHW_LOW_PARTS={parts}"
    want = oracle_files(six, q)
    assert [i for i in range(n) if files[1][i] != want[order[i]]] == []
