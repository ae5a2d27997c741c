"""Grey pictures, windows, crops and warps out of .nhwp containers, end to end on the GPU: the host calls
nhw_dec_windows_grey, nhw_dec_windows_grey_to_device, nhw_dec_crops_grey_to_device and nhw_dec_warps_grey_to_device and their Python wrappers.
The grey picture of a container is the oracle's (grey_picture_cases.grey_picture), a crop or warp what the colour kernel makes of the grey window
replicated into three channels, and the statuses and statistics are the colour calls' on the same rects."""
import ctypes
import math

import numpy as np
import pytest

from tests.grey_cases import grey_format
from tests.grey_picture_cases import NHW_E_ARG, NHW_E_FORMAT, assert_tensors, bits_of, grey_picture, reference_resize, reference_warp
from tests.picture_cases import SIZES, Rect, World, fixed_rects, make_container, parse_container, random_rects, selected
from tests.support import CANARY

pytestmark = pytest.mark.gpu
SCALES = (1, 2, 4)
QUALITIES = (22, 10, 18)                                             # picture p at QUALITIES[p]: a quality >= 20, one <= 16, one of 17 .. 19
BIG = 2                                                              # 1023 x 1025: a 2 x 3 grid, odd sides, six tiles over two chunks of the decoder


@pytest.fixture(scope="module")
def world(oracle):
    import nhwcodec_amd as na
    w = World()
    e = na.Encoder(0, max_batch=24)
    scene = na.untile_images(e.synth_device(24, 1300).cpu().numpy(), 4, 6)
    pics = [np.ascontiguousarray(scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES]
    w.containers = [e.encode_pictures([p], q)[0] for p, q in zip(pics, QUALITIES)]
    e.close()
    w.dec = na.Decoder(0, max_batch=4)
    w.grey = {}
    w.full = lambda s: w.grey.setdefault(s, [grey_picture(oracle, c, s) for c in w.containers])   # the reference, once a scale, never written to
    yield w
    w.dec.close()


def _rects(world, scale, seed, n=12):
    rng = np.random.default_rng(seed)
    out = []
    for ci, g in enumerate(world.full(scale)):
        H, W = g.shape
        out += [(ci, *r) for r in fixed_rects(W, H, 512 // scale, residues=False) + random_rects(W, H, n, rng, 300, 24)]
    return out


def _call(dec, name, containers, rects, scale, px):
    """nhw_dec_windows (px 3) or nhw_dec_windows_grey (px 1) by ctypes into a canary-filled host buffer with 7 bytes of slack behind every
    window -> (rc, status, buffer, offsets)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    out_off = np.zeros(len(rects) + 1, np.uint64)
    out_off[1:] = np.cumsum([px * r[3] * r[4] + 7 for r in rects])
    out = np.full(int(out_off[-1]) + 16, CANARY, np.uint8)
    rc = getattr(dec.lib, name)(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out.ctypes.data,
                                out_off.ctypes.data, status.ctypes.data)
    return rc, status, out, out_off


@pytest.mark.parametrize("scale", SCALES)
def test_decode_pictures_grey_is_the_oracles_grey_picture(world, scale):
    import nhwcodec_amd as na
    got = world.dec.decode_pictures_grey(world.containers, scale)
    for c, g, want in zip(world.containers, got, world.full(scale)):
        assert g.dtype == np.uint8 and g.shape == want.shape == na.scaled_size(*na.picture_info(c), scale)[::-1]
        bad = g != want
        assert not bad.any(), f"scale {scale}: {int(bad.sum())} pixels differ, first at {tuple(np.argwhere(bad)[0])}"
    assert world.dec.region_stats()[0] == 9                          # every tile of the three pictures, once


@pytest.mark.parametrize("scale", SCALES)
def test_grey_windows_are_slices_with_the_colour_calls_statistics(world, scale):
    import torch
    rects = _rects(world, scale, 240 + scale)
    full = world.full(scale)
    got = world.dec.decode_windows_grey(world.containers, rects, scale)
    grey_stats = world.dec.region_stats()
    for (ci, x, y, w, h), g in zip(rects, got):
        assert g.shape == (h, w) and np.array_equal(g, full[ci][y:y + h, x:x + w]), (scale, ci, x, y, w, h)
    world.dec.decode_windows(world.containers, rects, scale)
    assert world.dec.region_stats() == grey_stats and grey_stats[0] == 9
    # the device form: destinations of their own pitches in one canary-filled buffer, some packed, some with an odd pitch above the width
    at, place = 64, []
    for i, (_, _, _, w, h) in enumerate(rects):
        pitch = w if i % 2 else w + 1 + w % 2
        at += i % 16
        place.append((at, pitch))
        at += pitch * (h - 1) + w + 32
    buf = torch.full((at + 64,), CANARY, dtype=torch.uint8, device="cuda")
    views = [buf.as_strided((h, w), (pitch, 1), a) for (a, pitch), (_, _, _, w, h) in zip(place, rects)]
    back = world.dec.decode_windows_grey_device(world.containers, rects, scale, out=views)
    host, clean = buf.cpu().numpy(), np.ones(at + 64, bool)
    for (ci, x, y, w, h), (a, pitch), v in zip(rects, place, back):
        assert np.array_equal(v.cpu().numpy(), full[ci][y:y + h, x:x + w]), (scale, ci, x, y, w, h)
        for r in range(h):
            clean[a + r * pitch:a + r * pitch + w] = False
    assert (host[clean] == CANARY).all(), "a byte outside the windows was written"
    fresh = world.dec.decode_windows_grey_device(world.containers, rects[:3], scale)
    assert all(tuple(t.shape) == (r[4], r[3]) and np.array_equal(t.cpu().numpy(), full[r[0]][r[2]:r[2] + r[4], r[1]:r[1] + r[3]]) for t, r in zip(fresh, rects))


@pytest.mark.parametrize("scale", SCALES)
def test_crops_of_their_own_size_are_the_windows(world, scale):
    rng = np.random.default_rng(250 + scale)
    full = world.full(scale)
    w, h = 33, 21
    crops = [(ci, int(rng.integers(0, g.shape[1] - w + 1)), int(rng.integers(0, g.shape[0] - h + 1)), w, h) for ci, g in enumerate(full) if g.shape[1] >= w
             for _ in range(4)]
    assert len(crops) == 8
    fmt = grey_format("uint8", "HWC", "file")
    for filter in ("two_tap", "area", "cubic"):
        got, scales = world.dec.decode_crops_grey_device(world.containers, crops, (h, w), fmt, scale=scale, filter=filter)
        assert scales == [scale] * len(crops) and tuple(got.shape) == (len(crops), h, w, 1)
        for (ci, x, y, _, _), g in zip(crops, got.cpu().numpy()):
            assert np.array_equal(g[:, :, 0], full[ci][y:y + h, x:x + w]), (scale, filter, ci, x, y)


@pytest.mark.parametrize("filter", ("two_tap", "area", "cubic"))
def test_grey_crops_choose_their_scales_and_equal_the_colour_kernel(world, filter):
    import nhwcodec_amd as na
    import torch
    size = (24, 40)                                                  # out_h, out_w
    rng = np.random.default_rng(260)
    W, H = SIZES[BIG]
    crops = [(BIG, 5, 7, 900, 1000), (BIG, 100, 50, 170, 110), (BIG, 511, 500, 42, 30), (BIG, 0, 0, W, H), (1, 3, 1, 480, 360), (1, 250, 200, 20, 12), (0, 0, 100, 1, 500)]
    crops += [(BIG, int(rng.integers(0, 500)), int(rng.integers(0, 500)), int(rng.integers(40, 520)), int(rng.integers(24, 520))) for _ in range(5)]
    flips = [bool(i % 2) for i in range(len(crops))]
    want_scales = [na.crop_scale(w, h, size[1], size[0]) for _, _, _, w, h in crops]
    assert set(want_scales) == {1, 2, 4}
    windows = []
    for (ci, x, y, w, h), s in zip(crops, want_scales):
        wx, wy, ww, wh = na.crop_window(x, y, w, h, s)
        windows.append(world.full(s)[ci][wy:wy + wh, wx:wx + ww])
    want = reference_resize(windows, size, flips, filter)
    for fmt in (grey_format("uint8", "CHW", "file"), grey_format("float16", "CHW", "reversed")):
        n, per = len(crops), size[0] * size[1]
        buf = torch.full((n * per * fmt.dtype.itemsize + 256,), CANARY, dtype=torch.uint8, device="cuda")
        got, scales = world.dec.decode_crops_grey_device(world.containers, crops, size, fmt, flips=flips, out=buf[:n * per * fmt.dtype.itemsize].view(fmt.dtype), filter=filter)
        assert scales == want_scales and tuple(got.shape) == (n, 1) + size and got.data_ptr() == buf.data_ptr()
        assert_tensors(bits_of(got), want, fmt, f"decode_crops_grey_device, {filter}, {fmt}")
        assert bool((buf[n * per * fmt.dtype.itemsize:] == CANARY).all()), "elements behind the batch were written"


def test_grey_warps_choose_their_scales_and_equal_the_colour_kernel(world):
    import nhwcodec_amd as na
    size = (24, 40)
    W, H = SIZES[BIG]
    specs = [(BIG, 100, 120, 300, 200, 10.0, False), (BIG, 400, 300, 200, 150, 30.0, True), (BIG, 5, 5, 900, 900, 0.0, False), (BIG, 200, 100, 700, 800, -25.0, False),
             (1, 10, 10, 400, 300, 45.0, True), (BIG, 900, 900, 200, 200, 15.0, False), (0, 0, 200, 1, 300, 0.0, False), (BIG, 300, 300, 100, 60, 5.0, False)]
    which = [s[0] for s in specs]
    mats = [na.crop_warp(x, y, w, h, size, angle=math.radians(a), flip=f) for _, x, y, w, h, a, f in specs]
    want_scales = [na.warp_scale(m) for m in mats]
    assert set(want_scales) == {1, 2, 4}
    for border, fill in (("fill", 200), ("replicate", 3)):
        windows, fixed = [], []
        for ci, m, s in zip(which, mats, want_scales):
            (wx, wy, ww, wh), fx = na.warp_window(m, size, *SIZES[ci], s)
            windows.append(world.full(s)[ci][wy:wy + wh, wx:wx + ww])
            fixed.append(np.array(fx, np.int64))
        want = reference_warp(windows, fixed, size, fill, border)
        if border == "fill":
            assert (want[5] == fill).any(), "no tap of the warp at the picture's corner fell outside it"
        for fmt in (grey_format("uint8", "HWC", "file"), grey_format("bfloat16", "CHW", "reversed")):
            got, scales = world.dec.decode_warps_grey_device(world.containers, which, mats, size, fmt, fill=fill, border=border)
            assert scales == want_scales and tuple(got.shape) == (len(specs),) + fmt.shape(*size)
            assert_tensors(bits_of(got), want, fmt, f"decode_warps_grey_device, {border}, {fmt}")


@pytest.mark.parametrize("scale", (1, 4))
def test_a_damaged_tile_fails_exactly_the_rects_that_select_it(world, scale):
    import nhwcodec_amd as na
    k = 3                                                            # tile (ty 1, tx 1) of the 2 x 3 grid
    W, H, files = parse_container(world.containers[BIG])
    bad = list(files)
    bad[k] = b"\x07" + files[k][1:]                                  # res_high 7: the decoder refuses the tile
    broken = make_container(W, H, bad)
    full = world.full(scale)[BIG]
    rng = np.random.default_rng(270 + scale)
    rects = [(0, *r) for r in fixed_rects(full.shape[1], full.shape[0], 512 // scale, residues=False) + random_rects(full.shape[1], full.shape[0], 40, rng, 300, 24)]
    hit = [k in [n for n, _, _ in selected(W, scale, *r[1:])] for r in rects]
    assert 5 < sum(hit) < len(rects) - 5
    rc, status, out, out_off = _call(world.dec, "nhw_dec_windows_grey", [broken], rects, scale, 1)
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    grey_stats = world.dec.region_stats()
    rc3, status3, _, _ = _call(world.dec, "nhw_dec_windows", [broken], rects, scale, 3)
    assert rc3 == 0 and status3.tolist() == status.tolist() and world.dec.region_stats() == grey_stats
    clean = np.ones(out.size, bool)
    for (_, x, y, w, h), st, a in zip(rects, status, out_off):
        if st == 0:
            a = int(a)
            assert np.array_equal(out[a:a + w * h].reshape(h, w), full[y:y + h, x:x + w]), (x, y, w, h)
            clean[a:a + w * h] = False
    assert (out[clean] == CANARY).all(), "a failed rect's destination, or a byte between the windows, was written"
    with pytest.raises(na.NhwError):
        world.dec.decode_windows_grey([broken], rects, scale)
    # a crop that selects the tile fails, its tensor keeps the canary; the other goes through
    import torch
    fmt = grey_format("float16", "CHW", "file")
    crops = [r for r, h in zip(rects, hit) if h][:1] + [r for r, h in zip(rects, hit) if not h][:1]
    buf = torch.full((2 * 8 * 8 * 2,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(na.NhwError):
        world.dec.decode_crops_grey_device([broken], crops, (8, 8), fmt, scale=scale, out=buf.view(torch.float16))
    host = buf.cpu().numpy()
    assert (host[:128] == CANARY).all() and not (host[128:] == CANARY).all()


def test_a_debug_stop_refuses_the_grey_calls(world):
    dec = world.dec
    rects = [(1, 3, 4, 20, 10)]
    for scale in SCALES:
        dec.lib.nhw_dec_debug_stop_after(dec.h, 4)
        try:
            rc, status, out, _ = _call(dec, "nhw_dec_windows_grey", world.containers, rects, scale, 1)
        finally:
            dec.lib.nhw_dec_debug_stop_after(dec.h, 0)
        assert rc == NHW_E_ARG and b"debug stop" in dec.lib.nhw_dec_last_error() and (out == CANARY).all(), scale
    assert np.array_equal(dec.decode_windows_grey(world.containers, rects, 1)[0], world.full(1)[1][4:14, 3:23])


def test_one_handle_serves_colour_grey_and_colour(world):
    rects = _rects(world, 2, 280, n=4)
    before = world.dec.decode_windows(world.containers, rects, 2)
    grey = world.dec.decode_windows_grey(world.containers, rects, 2)
    after = world.dec.decode_windows(world.containers, rects, 2)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    full = world.full(2)
    assert all(np.array_equal(g, full[ci][y:y + h, x:x + w]) for (ci, x, y, w, h), g in zip(rects, grey))
