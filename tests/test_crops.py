"""Crops resized into tensors of one size: the rule, the kernel k_resize_to_tensor (nhw_resize_to_tensor_device), the
host call nhw_dec_crops_to_device and the Python wrappers crop_scale, crop_window, resize_to_tensor_device and Decoder.decode_crops_device.
The rule is stated here in numpy, in 64-bit integers, from the window's bytes alone; the elements come from tensor_cases.py's
expected_tensor.  Every comparison is exact: bytes for uint8, bit patterns for the float types."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.picture_cases import SIZES, Rect, World, expected_stats, make_container, parse_container, selected
from tests.support import CANARY, ROOT, load_lib
from tests.tensor_cases import ALL_FORMATS, expected_tensor, tensor_bits

NEW_SYMBOLS = ("nhw_crop_scale", "nhw_resize_to_tensor_device", "nhw_dec_crops_to_device")
PROTOTYPES = """
int nhw_crop_scale(uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height);
int nhw_resize_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                            uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status);
"""
NHW_E_ARG, NHW_E_FORMAT = -4, -6
GUARD = 4096                                                        # canary bytes kept in front of and behind a batch
SCALES = (1, 2, 4)
QUALITY = 20
BIG = 2                                                             # 1023 x 1025: a 2 x 3 grid of tiles, odd sides

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
NEGATIVE = dict(scale=(-1 / 255, -0.5, -2.0), bias=(1.0, 127.5, 3.25))


def _fmt(dtype, layout, channels, rows, k=0):
    """the TensorFormat of a parameter tuple; the float types take the ImageNet constants and a set with negative scales in turn"""
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, channels, rows)
    return na.TensorFormat(dtype, layout, channels, rows, **(IMAGENET, NEGATIVE)[k % 2])


# ---------------------------------------------------------------- the rule, in the test's own words
def positions(n, m):
    """output indices 0 .. m - 1 along an axis of source length n -> (i0, i1, f), all int64"""
    o = np.arange(m, dtype=np.int64)
    n, m = np.int64(n), np.int64(m)
    t = np.maximum((2 * o + 1) * n - m, 0)
    X = np.minimum(128 * t // m, 256 * (n - 1))
    i0, f = X >> 8, X & 255
    return i0, np.minimum(i0 + 1, n - 1), f


def rule(P, out_w, out_h, flip=False):
    """P uint8 [h, w, 3] -> R uint8 [out_h, out_w, 3], mirrored left-right with `flip`"""
    h, w = P.shape[:2]
    y0, y1, fy = positions(h, out_h)
    x0, x1, fx = positions(w, out_w)
    P = P.astype(np.int64)
    fy, fx = fy[:, None, None], fx[None, :, None]
    acc = ((256 - fx) * (256 - fy) * P[y0][:, x0] + fx * (256 - fy) * P[y0][:, x1] + (256 - fx) * fy * P[y1][:, x0] + fx * fy * P[y1][:, x1] + 32768)
    assert acc.max() < 1 << 32
    R = acc >> 16
    assert R.min() >= 0 and R.max() <= 255
    R = R.astype(np.uint8)
    return np.ascontiguousarray(R[:, ::-1]) if flip else R


@pytest.fixture(scope="module")
def lib():
    return load_lib()


# ---------------------------------------------------------------- without a GPU
def test_crop_symbols_and_prototypes(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    hdr = squeeze(open(os.path.join(ROOT, "include", "nhw_hip.h")).read())
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 3
    for decl in decls:
        assert squeeze(decl) in hdr, decl
    import nhwcodec_amd as na
    assert callable(na.crop_scale) and callable(na.crop_window) and callable(na.resize_to_tensor_device) and callable(na.Decoder.decode_crops_device)


def crop_scale_rule(w, h, out_w, out_h):
    for s in (4, 2):
        if s * out_w <= w and s * out_h <= h:
            return s
    return 1


def test_crop_scale_equals_the_c_function(lib):
    import nhwcodec_amd as na
    outs = [(1, 1), (224, 224), (32, 24), (4096, 4096), (299, 7)]
    n = 0
    for ow, oh in outs:
        sides_w = sorted({1, ow - 1, ow, ow + 1, 2 * ow - 1, 2 * ow, 2 * ow + 1, 4 * ow - 1, 4 * ow, 4 * ow + 1, 65535} - {0})
        sides_h = sorted({1, oh - 1, oh, oh + 1, 2 * oh - 1, 2 * oh, 2 * oh + 1, 4 * oh - 1, 4 * oh, 4 * oh + 1, 65535} - {0})
        for w in sides_w:
            for h in sides_h:
                want = crop_scale_rule(w, h, ow, oh)
                assert lib.nhw_crop_scale(w, h, ow, oh) == want == na.crop_scale(w, h, ow, oh), (w, h, ow, oh)
                n += 1
    assert n > 400
    assert {crop_scale_rule(2 * 224, 2 * 224, 224, 224), crop_scale_rule(2 * 224 - 1, 2 * 224, 224, 224), crop_scale_rule(4 * 224, 4 * 224, 224, 224),
            crop_scale_rule(4 * 224, 4 * 224 - 1, 224, 224)} == {1, 2, 4}
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 4097, 1), (5, 5, 1, 4097), (5, 5, 0xFFFFFFFF, 1)):
        assert lib.nhw_crop_scale(*bad) == NHW_E_ARG, bad
        with pytest.raises(na.NhwError):
            na.crop_scale(*bad)
    assert lib.nhw_crop_scale(0xFFFFFFFF, 0xFFFFFFFF, 4096, 4096) == 4


def test_crop_window_covers_the_crop_and_lies_inside_the_scaled_picture(lib):
    import nhwcodec_amd as na
    rng = np.random.default_rng(18)
    for W, H in ((1023, 1025), (1, 700)):
        crops = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (W - 1, 0, 1, H), (0, H - 1, W, 1), (max(W - 5, 0), max(H - 7, 0), min(5, W), min(7, H))]
        for _ in range(200):
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            x, y = (W - w, int(rng.integers(0, H - h + 1))) if rng.integers(2) else (int(rng.integers(0, W - w + 1)), H - h)   # the right or the bottom edge
            crops.append((x, y, w, h))
        for x, y, w, h in crops:
            assert x + w == W or y + h == H or (x, y) == (0, 0)
            for s in SCALES:
                sw, sh = -(-W // s), -(-H // s)
                assert (sw, sh) == na.scaled_size(W, H, s)
                x2, y2, w2, h2 = na.crop_window(x, y, w, h, s)
                assert (x2, y2) == (x // s, y // s) and w2 == -(-(x + w) // s) - x2 and h2 == -(-(y + h) // s) - y2
                assert w2 >= 1 and h2 >= 1 and x2 + w2 <= sw and y2 + h2 <= sh, (W, H, x, y, w, h, s)
                assert s * x2 <= x and s * (x2 + w2) >= x + w and s * y2 <= y and s * (y2 + h2) >= y + h       # it covers the crop ...
                assert s * (x2 + 1) > x and s * (x2 + w2 - 1) < x + w and s * (y2 + 1) > y and s * (y2 + h2 - 1) < y + h   # ... and no smaller one does
                assert na.window_tiles(W, H, s, x2, y2, w2, h2) >= 1
    assert na.crop_window(10, 20, 30, 40, 1) == (10, 20, 30, 40)
    for bad in ((0, 0, 0, 1, 1), (0, 0, 1, 0, 1), (-1, 0, 1, 1, 1), (0, 0, 1, 1, 3), (0, 0, 1, 1, 0)):
        with pytest.raises(na.NhwError):
            na.crop_window(*bad)


def test_the_rule_by_hand(lib):
    """what follows from the rule, worked by hand: the identity, the 2 x 2 box mean, a single source pixel, two rows of numbers"""
    import nhwcodec_amd as na
    rng = np.random.default_rng(1)
    for w, h in ((1, 1), (5, 3), (33, 17), (64, 2)):
        P = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert all((f == 0).all() for f in (positions(w, w)[2], positions(h, h)[2]))
        assert np.array_equal(rule(P, w, h), P)                      # out == (w, h): R == P
        assert np.array_equal(rule(P, w, h, True), P[:, ::-1])
    for ow, oh in ((1, 1), (7, 3), (16, 16)):
        P = rng.integers(0, 256, (2 * oh, 2 * ow, 3), dtype=np.uint8)
        q = P.astype(np.int64)
        box = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
        assert np.array_equal(rule(P, ow, oh), box.astype(np.uint8))  # w = 2 out_w, h = 2 out_h: the rounded box mean
        assert na.crop_scale(2 * ow, 2 * oh, ow, oh) == 2 and lib.nhw_crop_scale(2 * ow, 2 * oh, ow, oh) == 2
    P = np.array([[[9, 200, 31]]], np.uint8)
    assert np.array_equal(rule(P, 5, 4), np.broadcast_to(P, (4, 5, 3)))   # a 1 x 1 source fills the output
    row = lambda v: np.repeat(np.array(v, np.uint8)[None, :, None], 3, axis=2)
    assert rule(row([0, 255]), 3, 1)[0, :, 0].tolist() == [0, 128, 255]
    x0, x1, fx = positions(3, 2)
    assert (256 * x0 + fx).tolist() == [64, 448] and x1.tolist() == [1, 2]
    assert rule(row([10, 20, 40]), 2, 1)[0, :, 1].tolist() == [13, 35]
    assert rule(row([10, 20, 40]), 2, 1, True)[0, :, 2].tolist() == [35, 13]
    assert rule(row([10, 20, 40]).transpose(1, 0, 2), 1, 2)[:, 0, 0].tolist() == [13, 35]   # the same down a column
    i0, i1, f = positions(65535, 4096)                               # the extremes stay inside the axis
    assert i0.min() >= 0 and i1.max() <= 65534 and (i1 - i0).max() == 1
    i0, i1, f = positions(2, 4096)                                   # both clamps: the first and the last quarter of the outputs sit on a source pixel
    assert (i0[0], f[0], i0[-1], i1[-1], f[-1]) == (0, 0, 1, 1, 0) and (f[:1024] == 0).all() and (f[3072:] == 0).all() and f[2048] == 128 and f[3071] == 255


# ---------------------------------------------------------------- on the MI355X: the kernel alone
SRC_SIZES = [(1, 1), (7, 1), (2, 2), (5, 3), (33, 17), (256, 255), (300, 200)]      # W, H
OUT_SIZES = [(1, 1), (3, 2), (4, 5), (16, 16), (224, 224), (299, 299), (4096, 1)]   # W, H
FLAGS = [0, 1, 0, 1, 1, 0, 1]


class Sources:
    pass


@pytest.fixture(scope="module")
def sources():
    return _make_sources()


def _make_sources():
    """the seven sources as views of one device buffer of random bytes, every row followed by a gap of 1 .. bytes and every picture at an odd
    address; .own their bytes on the host; .rule(k, out_w, out_h, flip) the rule applied to source k, computed once"""
    import torch
    import nhwcodec_amd as na
    s = Sources()
    rng = np.random.default_rng(180)
    host = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    at, places = 1, []
    for k, (w, h) in enumerate(SRC_SIZES):
        pitch = 3 * w + 1 + 2 * k
        places.append((at, pitch))
        at = (at + h * pitch + 7) | 1
    assert at < host.size
    s.own = [np.stack([host[o + r * p: o + r * p + 3 * w] for r in range(h)]).reshape(h, w, 3).copy() for (o, p), (w, h) in zip(places, SRC_SIZES)]
    s.buf = torch.from_numpy(host).cuda()
    s.views = [s.buf.as_strided((h, w, 3), (p, 3, 1), o) for (o, p), (w, h) in zip(places, SRC_SIZES)]
    assert all(v.data_ptr() % 2 == 1 for v in s.views)
    s.table, _, _ = na._picture_table(s.views, "test")
    cache = {}

    def cached(k, out_w, out_h, flip):
        key = (k, out_w, out_h, bool(flip))
        if key not in cache:
            cache[key] = rule(s.own[k], out_w, out_h, bool(flip))
        return cache[key]
    s.rule = cached
    return s


def _guarded(n, per, fmt):
    """a canary-filled byte buffer with room for n tensors of `per` elements between two guards -> (buffer, the byte offset of tensor 0)"""
    import torch
    es = fmt.dtype.itemsize
    buf = torch.full((2 * GUARD + n * per * es,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, GUARD


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h", OUT_SIZES)
def test_gpu_resize_kernel_on_random_bytes(sources, out_w, out_h):
    """all seven sources in one launch, flags mixed, under all 32 formats; every fourth format also with a null flag table; the batch between
    guards"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    n, per = len(SRC_SIZES), 3 * out_w * out_h
    d_flags = torch.tensor(FLAGS, dtype=torch.uint8, device="cuda")
    for k, four in enumerate(ALL_FORMATS):
        fmt = _fmt(*four, k=k // 2)
        es = fmt.dtype.itemsize
        buf, at = _guarded(n, per, fmt)
        addr = torch.tensor([buf.data_ptr() + at + i * per * es for i in range(n)], dtype=torch.int64, device="cuda")
        c = fmt.c_struct()
        for flags in ((FLAGS, None) if k % 4 == 0 else (FLAGS,)):
            buf.fill_(CANARY)
            assert L.nhw_resize_to_tensor_device(sources.table.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_flags.data_ptr() if flags else None,
                                                 addr.data_ptr(), None) == 0, L.nhw_last_error()
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert (host[:at] == CANARY).all() and (host[at + n * per * es:] == CANARY).all(), f"{fmt}: a byte outside the batch was written"
            for i in range(n):
                want = expected_tensor(sources.rule(i, out_w, out_h, flags[i] if flags else 0), fmt)
                got = host[at + i * per * es: at + (i + 1) * per * es].view(want.dtype).reshape(want.shape)
                assert np.array_equal(got, want), f"{fmt} source {SRC_SIZES[i]} to {out_w} x {out_h}, flags {flags}: {int((got != want).sum())} elements differ"
    # the wrapper: the same tensors, as one batch
    fmt = _fmt("float16", "CHW", "RGB", "reversed")
    got = na.resize_to_tensor_device(sources.views, (out_h, out_w), fmt, flips=[bool(f) for f in FLAGS])
    assert got.dtype == fmt.dtype and tuple(got.shape) == (n, 3, out_h, out_w)
    bits = tensor_bits(got)
    for i in range(n):
        assert np.array_equal(bits[i], expected_tensor(sources.rule(i, out_w, out_h, FLAGS[i]), fmt))
    plain = na.resize_to_tensor_device(sources.views, (out_h, out_w), _fmt("uint8", "HWC", "BGR", "file"))
    assert tuple(plain.shape) == (n, out_h, out_w, 3)
    for i in range(n):
        assert np.array_equal(plain[i].cpu().numpy(), sources.rule(i, out_w, out_h, 0))


@pytest.mark.gpu
def test_gpu_resize_entries_that_store_nothing(sources):
    """a zero address, a misaligned address, a zero-width and an oversize source: their slots keep the canary, their neighbours are right"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    out_w, out_h = 16, 9
    per = 3 * out_w * out_h
    table = sources.table.cpu().numpy().view(na.PICTURE_DTYPE).copy()
    picks = [4, 5, 6, 4, 5, 6]
    tab = table[picks]
    tab["width"][3] = 0                                              # a zero-width source
    tab["height"][4] = 65536                                         # an oversize one
    d_tab = torch.from_numpy(tab.view(np.int64).copy()).cuda()
    for four in (("float16", "CHW", "RGB", "reversed"), ("float32", "HWC", "BGR", "file"), ("bfloat16", "HWC", "RGB", "file")):
        fmt = _fmt(*four)
        es = fmt.dtype.itemsize
        buf, at = _guarded(len(picks), per, fmt)
        addrs = [buf.data_ptr() + at + i * per * es for i in range(len(picks))]
        addrs[1] = 0                                                 # no address
        addrs[2] += 1                                                # no multiple of the element size
        addr = torch.tensor(addrs, dtype=torch.int64, device="cuda")
        c = fmt.c_struct()
        assert L.nhw_resize_to_tensor_device(d_tab.data_ptr(), len(picks), out_w, out_h, ctypes.byref(c), None, addr.data_ptr(), None) == 0
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        for i, k in enumerate(picks):
            got = host[at + i * per * es: at + (i + 1) * per * es]
            if i in (0, 5):
                want = expected_tensor(sources.rule(k, out_w, out_h, 0), fmt)
                assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), (fmt, i)
            else:
                assert (got == CANARY).all(), (fmt, i)
        assert (host[:at] == CANARY).all() and (host[at + len(picks) * per * es:] == CANARY).all()


@pytest.mark.gpu
def test_gpu_resize_many_crops_take_bands_of_64_rows(sources):
    """4096 crops to 3 x 130: with so many crops a band has the most rows it can have, 64, so a crop is two full bands and one of two rows,
    and a pass of the workgroup walks 64 rows of 4 lanes"""
    import torch
    import nhwcodec_amd as na
    n, out_w, out_h = 4096, 3, 130
    table = sources.table.cpu().numpy().view(na.PICTURE_DTYPE)
    d_tab = torch.from_numpy(table[np.arange(n) % len(SRC_SIZES)].view(np.int64).copy()).cuda()
    flags = (np.arange(n) // len(SRC_SIZES)) % 2
    fmt = _fmt("float16", "CHW", "BGR", "reversed")
    per = 3 * out_w * out_h
    buf, at = _guarded(n, per, fmt)
    addr = torch.from_numpy(buf.data_ptr() + at + np.arange(n, dtype=np.int64) * (per * 2)).cuda()
    c = fmt.c_struct()
    d_flags = torch.from_numpy(flags.astype(np.uint8)).cuda()
    assert na._library().nhw_resize_to_tensor_device(d_tab.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_flags.data_ptr(), addr.data_ptr(), None) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:at] == CANARY).all() and (host[at + n * per * 2:] == CANARY).all()
    got = host[at:at + n * per * 2].view(np.uint16).reshape(n, 3, out_h, out_w)
    for k in range(len(SRC_SIZES)):
        for f in (0, 1):
            mine = got[(np.arange(n) % len(SRC_SIZES) == k) & (flags == f)]
            assert len(mine) > 200 and (mine == expected_tensor(sources.rule(k, out_w, out_h, f), fmt)[None]).all(), (k, f)


# ---------------------------------------------------------------- on the MI355X: the host path
@pytest.fixture(scope="module")
def world():
    """the windows' pictures (SIZES: 1 x 700, 500 x 375, 1023 x 1025, crops of one seeded scene of generated images) as containers at q20, and a
    decoder of 4 tiles a chunk: the six tiles of the large picture span two chunks"""
    import nhwcodec_amd as na
    w = World()
    e = na.Encoder(0, max_batch=24)
    scene = na.untile_images(e.synth_device(24, 1300).cpu().numpy(), 4, 6)
    w.pics = [np.ascontiguousarray(scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES]
    w.containers = e.encode_pictures(w.pics, QUALITY)
    e.close()
    w.dec = na.Decoder(0, max_batch=4)
    yield w
    w.dec.close()


def seeded_windows(scale, n, rng):
    """n windows at `scale` over the three pictures, mixed sizes and aspects, some on the picture's edges -> [(container, x, y, w, h)]"""
    out = []
    for i in range(n):
        ci = (2, 2, 1, 2, 0)[i % 5]
        W, H = -(-SIZES[ci][0] // scale), -(-SIZES[ci][1] // scale)
        w, h = int(rng.integers(1, min(W, 400) + 1)), int(rng.integers(1, min(H, 300) + 1))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        if i % 7 == 3:
            x, y = W - w, H - h                                      # the last column and row of the scaled picture
        out.append((ci, x, y, w, h))
    return out


def slots(rects, scale):
    """the slots of every rect's tiles: a tile gets the next slot when the first rect selects it (section 15)"""
    slot, out = {}, []
    for ci, x, y, w, h in rects:
        out.append([slot.setdefault((ci, k), len(slot)) for k, _, _ in selected(SIZES[ci][0], scale, x, y, w, h)])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_gpu_crops_of_their_own_size_are_the_windows(world, scale):
    import torch
    import nhwcodec_amd as na
    w, h = 56, 40
    big_w, big_h = na.scaled_size(*SIZES[BIG], scale)
    rects = [(BIG, x, y, w, h) for x, y in ((0, 0), (big_w - w, big_h - h), (big_w // 2 - 30, big_h // 2 - 10), (7, big_h - h), (big_w - w, 3))]
    rects += [(1, 3, 5, w, h)]
    wins = world.dec.decode_windows_device(world.containers, rects, scale)
    for four in (("uint8", "HWC", "BGR", "file"), ("float16", "CHW", "RGB", "reversed"), ("float32", "HWC", "RGB", "reversed"), ("bfloat16", "CHW", "BGR", "file")):
        fmt = _fmt(*four)
        want = torch.stack(na.pictures_to_tensor_device(wins, fmt))
        got, scales = world.dec.decode_crops_device(world.containers, rects, (h, w), fmt, scale=scale)
        assert scales == [scale] * len(rects) and got.dtype == fmt.dtype and tuple(got.shape) == (len(rects),) + fmt.shape(h, w)
        assert np.array_equal(tensor_bits(got), tensor_bits(want)), (scale, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h,four", [(32, 24, ("uint8", "HWC", "BGR", "file")), (224, 224, ("float16", "CHW", "RGB", "reversed"))])
@pytest.mark.parametrize("scale", SCALES)
def test_gpu_crops_equal_the_rule_on_decode_windows(world, scale, out_w, out_h, four):
    """60 seeded crops in one call on a decoder of max_batch 4: the nine tiles go in three chunks and crops of the large picture span them"""
    import torch
    import nhwcodec_amd as na
    fmt = _fmt(*four)
    rng = np.random.default_rng(1800 + 10 * scale + out_w)
    rects = seeded_windows(scale, 60, rng)
    flips = [bool(v) for v in rng.integers(0, 2, len(rects))]
    assert 10 < sum(flips) < 50
    assert sum(len({k // 4 for k in ks}) > 1 for ks in slots(rects, scale)) >= 3      # crops whose tiles lie in two chunks of four
    wins = world.dec.decode_windows(world.containers, rects, scale)
    stats = world.dec.region_stats()
    got, scales = world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, flips=flips, scale=scale)
    assert scales == [scale] * len(rects) and tuple(got.shape) == (len(rects),) + fmt.shape(out_h, out_w)
    assert world.dec.region_stats() == stats == expected_stats(world.containers, rects, scale, unique=True)
    assert 8 <= stats[0] <= 9 < sum(len(k) for k in slots(rects, scale))                            # (nearly) every tile there is, each once
    bits = tensor_bits(got)
    for i, (r, P, f) in enumerate(zip(rects, wins, flips)):
        assert P.shape == (r[4], r[3], 3)
        assert np.array_equal(bits[i], expected_tensor(rule(P, out_w, out_h, f), fmt)), (scale, r, f)
    # the crops in another order, into a tensor of the caller's: the same slots in that order, and nothing behind them
    perm = rng.permutation(len(rects))
    per = 3 * out_w * out_h
    mine = torch.full((len(rects) * per + 64,), 1, dtype=fmt.dtype, device="cuda")
    before = tensor_bits(mine[len(rects) * per:]).copy()
    again, _ = world.dec.decode_crops_device(world.containers, [rects[i] for i in perm], (out_h, out_w), fmt, flips=[flips[i] for i in perm], scale=scale, out=mine)
    assert again.data_ptr() == mine.data_ptr() and world.dec.region_stats() == stats
    assert np.array_equal(tensor_bits(again), bits[perm])
    assert np.array_equal(tensor_bits(mine[len(rects) * per:]), before)


@pytest.mark.gpu
def test_gpu_crops_choose_their_scale(world):
    """full-resolution crops of the large picture to 64 x 48: all three scales in one call, each crop decoded as crop_window at crop_scale"""
    import nhwcodec_amd as na
    W, H = SIZES[BIG]
    out_w, out_h = 64, 48
    rng = np.random.default_rng(185)
    crops = [(BIG, 0, 0, W, H), (BIG, W - 256, H - 192, 256, 192), (BIG, W - 255, H - 192, 255, 192), (BIG, 511, 513, 128, 96), (BIG, 300, 1, 127, 96),
             (BIG, W - 31, H - 17, 31, 17), (BIG, 5, 7, 64, 48), (1, 0, 0, 500, 375), (1, 100, 100, 200, 97), (0, 0, 100, 1, 500)]
    for _ in range(30):
        w, h = int(rng.integers(8, 600)), int(rng.integers(8, 600))
        crops.append((BIG, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    flips = [bool(v) for v in rng.integers(0, 2, len(crops))]
    fmt = _fmt("float32", "CHW", "RGB", "reversed", k=1)
    got, scales = world.dec.decode_crops_device(world.containers, crops, (out_h, out_w), fmt, flips=flips)
    assert scales == [crop_scale_rule(w, h, out_w, out_h) for _, _, _, w, h in crops] == [na.crop_scale(w, h, out_w, out_h) for _, _, _, w, h in crops]
    assert scales[:7] == [4, 4, 2, 2, 1, 1, 1] and all(scales.count(s) >= 5 for s in SCALES)
    bits = tensor_bits(got)
    for s in SCALES:
        idx = [i for i, v in enumerate(scales) if v == s]
        rects = [(crops[i][0], *na.crop_window(*crops[i][1:], s)) for i in idx]
        for i, P in zip(idx, world.dec.decode_windows(world.containers, rects, s)):
            assert np.array_equal(bits[i], expected_tensor(rule(P, out_w, out_h, flips[i]), fmt)), (s, crops[i])
    with pytest.raises(na.NhwError):                                 # a crop beyond the picture has no window
        world.dec.decode_crops_device(world.containers, [(BIG, W - 10, 0, 11, 20)], (out_h, out_w), fmt)
    with pytest.raises(na.NhwError):
        world.dec.decode_crops_device(world.containers, [(BIG, 0, 0, 0, 20)], (out_h, out_w), fmt)


def _call_crops(dec, containers, rects, scale, out_w, out_h, c_fmt, flags, addrs):
    """nhw_dec_crops_to_device by ctypes: the wrapper raises on a status -> (rc, status)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    addr = np.array(addrs if addrs is not None else [], np.uint64)
    f = np.array(flags, np.uint8) if flags is not None else None
    rc = dec.lib.nhw_dec_crops_to_device(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out_w, out_h,
                                         ctypes.byref(c_fmt) if c_fmt is not None else None, f.ctypes.data if f is not None else None,
                                         addr.ctypes.data if addrs is not None else None, status.ctypes.data)
    return rc, status


@pytest.mark.gpu
@pytest.mark.parametrize("scale", (1, 4))
def test_gpu_a_refused_tile_fails_exactly_the_crops_that_select_it(world, scale):
    import torch
    import nhwcodec_amd as na
    k = 3                                                            # 1023 x 1025, 2 x 3 tiles: tile (ty 1, tx 1)
    W, H, files = parse_container(world.containers[BIG])
    bad = list(files)
    bad[k] = b"\x07" + files[k][1:]                                  # res_high 7: the decoder refuses the tile
    broken = make_container(W, H, bad)
    assert na.picture_info(broken) == (W, H)
    rng = np.random.default_rng(186 + scale)
    rects = [(0, *r[1:]) for r in seeded_windows(scale, 60, rng) if r[0] == BIG] + [(0, 0, 0, 5, 5), (0, (W - 1) // scale, (H - 1) // scale, 1, 1)]
    hit = [k in [n for n, _, _ in selected(W, scale, *r[1:])] for r in rects]
    assert 5 < sum(hit) < len(rects) - 5
    out_w, out_h = 32, 24
    fmt = _fmt("float16", "CHW", "RGB", "reversed")
    per, es = 3 * out_w * out_h, 2
    buf, at = _guarded(len(rects), per, fmt)
    addrs = [buf.data_ptr() + at + i * per * es for i in range(len(rects))]
    flips = [i % 3 == 0 for i in range(len(rects))]
    rc, status = _call_crops(world.dec, [broken], rects, scale, out_w, out_h, fmt.c_struct(), flips, addrs)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    assert world.dec.region_stats() == expected_stats([broken], rects, scale, unique=True)
    host = buf.cpu().numpy()
    ok = [r for r, h in zip(rects, hit) if not h]
    wins = iter(world.dec.decode_windows([broken], ok, scale))
    for i, (r, h) in enumerate(zip(rects, hit)):
        got = host[at + i * per * es: at + (i + 1) * per * es]
        if h:
            assert (got == CANARY).all(), r                          # a failed crop's destination is not written
        else:
            want = expected_tensor(rule(next(wins), out_w, out_h, flips[i]), fmt)
            assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), r
    assert (host[:at] == CANARY).all() and (host[at + len(rects) * per * es:] == CANARY).all()
    with pytest.raises(na.NhwError):
        world.dec.decode_crops_device([broken], rects, (out_h, out_w), fmt, scale=scale)
    good, _ = world.dec.decode_crops_device([broken], ok, (out_h, out_w), fmt, scale=scale)
    assert tuple(good.shape) == (len(ok), 3, out_h, out_w)


@pytest.mark.gpu
def test_gpu_crop_refusals_launch_nothing(world, sources):
    import torch
    import nhwcodec_amd as na
    L = na._library()
    fmt = _fmt("float32", "CHW", "RGB", "reversed")
    out_w, out_h = 8, 8
    per = 3 * out_w * out_h
    buf, at = _guarded(8, per, fmt)
    addrs = [buf.data_ptr() + at + i * per * 4 for i in range(7)]
    d_addr = torch.tensor(addrs, dtype=torch.int64, device="cuda")
    good = fmt.c_struct()

    def bad_format(**kw):
        c = fmt.c_struct()
        for key, v in kw.items():
            if key in ("scale", "bias"):
                getattr(c, key)[1] = v
            else:
                setattr(c, key, v)
        return c

    formats = [bad_format(dtype=4), bad_format(layout=2), bad_format(channels=-1), bad_format(rows=2), bad_format(reserved=1), bad_format(scale=float("nan")),
               bad_format(bias=float("inf")), bad_format(dtype=0, scale=2.0)]
    tab = sources.table.data_ptr()
    # the pointwise entry
    for ow, oh in ((0, 8), (8, 0), (4097, 8), (8, 4097), (0xFFFFFFFF, 8)):
        assert L.nhw_resize_to_tensor_device(tab, 7, ow, oh, ctypes.byref(good), None, d_addr.data_ptr(), None) == NHW_E_ARG, (ow, oh)
    for c in formats:
        assert L.nhw_resize_to_tensor_device(tab, 7, out_w, out_h, ctypes.byref(c), None, d_addr.data_ptr(), None) == NHW_E_ARG
    assert L.nhw_resize_to_tensor_device(tab, 7, out_w, out_h, None, None, d_addr.data_ptr(), None) == NHW_E_ARG
    assert L.nhw_resize_to_tensor_device(None, 7, out_w, out_h, ctypes.byref(good), None, d_addr.data_ptr(), None) == NHW_E_ARG
    assert L.nhw_resize_to_tensor_device(tab, 7, out_w, out_h, ctypes.byref(good), None, None, None) == NHW_E_ARG
    assert L.nhw_resize_to_tensor_device(tab, 0, out_w, out_h, ctypes.byref(good), None, d_addr.data_ptr(), None) == NHW_E_ARG
    # the host call
    rects = [(BIG, 10, 20, 30, 40), (1, 0, 0, 50, 50)]
    two = addrs[:2]
    world.dec.decode_windows(world.containers, rects, 1)
    stats = world.dec.region_stats()
    for ow, oh in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert _call_crops(world.dec, world.containers, rects, 1, ow, oh, good, None, two)[0] == NHW_E_ARG, (ow, oh)
    for s in (3, 0, 8, -1):
        assert _call_crops(world.dec, world.containers, rects, s, out_w, out_h, good, None, two)[0] == NHW_E_ARG, s
    for c in formats + [None]:
        assert _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, c, None, two)[0] == NHW_E_ARG
    assert _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, good, None, [two[0], 0])[0] == NHW_E_ARG          # no address
    assert _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, good, None, [two[0], two[1] + 2])[0] == NHW_E_ARG  # float32 at 2 mod 4
    assert _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, good, None, None)[0] == NHW_E_ARG
    world.dec.lib.nhw_dec_debug_stop_after(world.dec.h, 3)            # a handle with a debug stop: no scaled call of any kind
    try:
        for s in (2, 4):
            assert _call_crops(world.dec, world.containers, rects, s, out_w, out_h, good, None, two)[0] == NHW_E_ARG
    finally:
        world.dec.lib.nhw_dec_debug_stop_after(world.dec.h, 0)
    # the wrappers
    dec, cs = world.dec, world.containers
    size = (out_h, out_w)
    for kw in (dict(flips=[True]), dict(flips=[True, False, True]), dict(flips=[0.5, 1.0]), dict(scale=3), dict(scale=True),
               dict(out=torch.empty(2 * per, dtype=torch.float16, device="cuda")), dict(out=torch.empty(2 * per, dtype=torch.float32)),
               dict(out=torch.empty(2 * per - 1, dtype=torch.float32, device="cuda")),
               dict(out=torch.empty((2 * per, 2), dtype=torch.float32, device="cuda")[:, 0])):
        with pytest.raises(na.NhwError):
            dec.decode_crops_device(cs, rects, size, fmt, **{"scale": 1, **kw})
    for bad_size in ((0, 8), (8, 4097), (8,), 8, (8.0, 8)):
        with pytest.raises(na.NhwError):
            dec.decode_crops_device(cs, rects, bad_size, fmt, scale=1)
        with pytest.raises(na.NhwError):
            na.resize_to_tensor_device(sources.views, bad_size, fmt)
    with pytest.raises(na.NhwError):
        dec.decode_crops_device(cs, rects, size, "float32", scale=1)
    with pytest.raises(na.NhwError):
        na.resize_to_tensor_device(sources.views, size, fmt, flips=[True] * 6)
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()), "a refused call wrote"
    assert world.dec.region_stats() == stats                         # ... and none of them reached the decoder
    got, _ = dec.decode_crops_device(cs, rects, size, fmt, scale=1)     # the same call with nothing wrong does run
    assert tuple(got.shape) == (2, 3, out_h, out_w)


@pytest.mark.gpu
def test_gpu_one_handle_serves_files_pictures_windows_and_crops(world):
    import nhwcodec_amd as na
    cs = world.containers
    files = parse_container(cs[BIG])[2]
    fmt = _fmt("bfloat16", "HWC", "RGB", "reversed")
    rects = {1: [(BIG, 500, 500, 100, 100), (1, 0, 0, 500, 375), (BIG, 0, 0, 1023, 1025), (0, 0, 699, 1, 1)],
             2: [(BIG, 250, 250, 50, 50), (1, 0, 0, 250, 188), (BIG, 0, 0, 512, 513), (0, 0, 349, 1, 1)],
             4: [(BIG, 125, 125, 25, 25), (1, 0, 0, 125, 94), (BIG, 0, 0, 256, 257), (0, 0, 174, 1, 1)]}
    steps = [("files", lambda d: d.decode(files[:4])[0]), ("pictures", lambda d: d.decode_pictures(cs))]
    for s in SCALES:
        steps += [(f"windows {s}", lambda d, s=s: d.decode_windows(cs, rects[s], s)),
                  (f"crops {s}", lambda d, s=s: [tensor_bits(d.decode_crops_device(cs, rects[s], (24, 40), fmt, flips=[True, False, False, True], scale=s)[0])]),
                  (f"windows again {s}", lambda d, s=s: d.decode_windows(cs, rects[s], s))]
    steps.append(("crops any", lambda d: [tensor_bits(d.decode_crops_device(cs, rects[1], (24, 40), fmt)[0])]))
    fresh = []
    for name, step in steps:                                         # every step on a handle of its own
        d = na.Decoder(0, max_batch=4)
        fresh.append([np.array(a) for a in step(d)])
        d.close()
    one = na.Decoder(0, max_batch=4)
    for _ in range(2):
        for (name, step), want in zip(steps, fresh):
            got = step(one)
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), name
    one.close()
    for s in SCALES:                                                 # the windows before and after a crop call are the same pictures
        before, after = (fresh[[n for n, _ in steps].index(f"{k} {s}")] for k in ("windows", "windows again"))
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        crops = fresh[[n for n, _ in steps].index(f"crops {s}")][0]
        for i, P in enumerate(before):
            assert np.array_equal(crops[i], expected_tensor(rule(P, 40, 24, i in (0, 3)), fmt)), (s, i)
