"""The area filter: the rule, the kernel k_area_to_tensor (nhw_area_to_tensor_device), the host calls
nhw_dec_crops_to_device_filter and nhw_enc_pictures_resized, the Python wrappers (resize_to_tensor_device and Decoder.decode_crops_device with
filter="area", Encoder.encode_pictures_resized, Encoder.encode_resized_device) and nhw-enc --resize.  Both axis rules are stated here in numpy,
in 64-bit integers: section 18's two taps for an axis that does not shrink, the exact area for one that does -- once as a list of taps, once as
a difference of prefix sums, which keeps a 65535-pixel axis cheap.  Every comparison is exact: bytes for uint8, bit patterns for the floats."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from tests.picture_cases import SIZES, Rect, World, expected_stats, parse_container
from tests.support import CANARY, ROOT, built_cli, load_lib, run, same_files
from tests.tensor_cases import ALL_FORMATS, expected_tensor, tensor_bits

NEW_SYMBOLS = ("nhw_area_to_tensor_device", "nhw_dec_crops_to_device_filter", "nhw_enc_pictures_resized")
PROTOTYPES = """
int nhw_area_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                              const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_to_device_filter(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr, int32_t *status,
                                   int filter);
int nhw_enc_pictures_resized(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, int n,
                             uint32_t out_width, uint32_t out_height, int quality, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, int32_t *status);
"""
DEFINES = {"NHW_FILTER_TWO_TAP": 0, "NHW_FILTER_AREA": 1, "NHW_AREA_MAX_REDUCTION": 128}
NHW_E_ARG = -4
LIMIT = 128
GUARD = 4096                                                        # canary bytes kept in front of and behind a batch
SCALES = (1, 2, 4)
BIG = 2                                                             # 1023 x 1025: a 2 x 3 grid of tiles, odd sides

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
NEGATIVE = dict(scale=(-1 / 255, -0.5, -2.0), bias=(1.0, 127.5, 3.25))
BYTES = ("uint8", "HWC", "BGR", "file")                             # the two formats section 18's tests use
HALF = ("float16", "CHW", "RGB", "reversed")


def _fmt(dtype, layout, channels, rows, k=0):
    """the TensorFormat of a parameter tuple; the float types take the ImageNet constants and a set with negative scales in turn"""
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, channels, rows)
    return na.TensorFormat(dtype, layout, channels, rows, **(IMAGENET, NEGATIVE)[k % 2])


# ---------------------------------------------------------------- the rule, in the test's own words
def two_taps(n, m):
    """section 18's positions of output indices 0 .. m - 1 along an axis of source length n -> (i0, i1, f), int64"""
    o = np.arange(m, dtype=np.int64)
    n, m = np.int64(n), np.int64(m)
    t = np.maximum((2 * o + 1) * n - m, 0)
    X = np.minimum(128 * t // m, 256 * (n - 1))
    i0, f = X >> 8, X & 255
    return i0, np.minimum(i0 + 1, n - 1), f


def taps(n, m, o):
    """the rule's taps of output index o as a list -> (source indices, weights, the axis total A)"""
    if m >= n:
        i0, i1, f = (int(v[o]) for v in two_taps(n, m))
        return [i0, i1], [256 - f, f], 256
    first, last = o * n // m, -(-(o + 1) * n // m) - 1
    idx = list(range(first, last + 1))
    return idx, [min((i + 1) * m, (o + 1) * n) - max(i * m, o * n) for i in idx], n


def along(A, m):
    """the weighted sums of the rule along axis 0 of A, int64 [n, ...] -> ([m, ...], the axis total).  A shrinking axis without a tap list:
    with C the prefix sums of A, F(t) = m C[t // m] + (t % m) A[t // m] is the sum over [0, t) in units of 1 / m pixel, and output o is
    F((o + 1) n) - F(o n)"""
    n = A.shape[0]
    col = (-1,) + (1,) * (A.ndim - 1)
    if m >= n:
        i0, i1, f = two_taps(n, m)
        return (256 - f).reshape(col) * A[i0] + f.reshape(col) * A[i1], 256
    zero = np.zeros((1,) + A.shape[1:], np.int64)
    C, Ap = np.concatenate([zero, np.cumsum(A, axis=0)]), np.concatenate([A, zero])
    t = np.arange(m + 1, dtype=np.int64) * n
    F = m * C[t // m] + (t % m).reshape(col) * Ap[t // m]
    return F[1:] - F[:-1], n


def rule(P, out_w, out_h, flip=False):
    """P uint8 [h, w, 3] -> R uint8 [out_h, out_w, 3] under the area rule, mirrored left-right with `flip`"""
    h, w = P.shape[:2]
    assert 1 <= w <= 65535 and 1 <= h <= 65535 and w <= LIMIT * out_w and h <= LIMIT * out_h
    rows, Ax = along(P.astype(np.int64).transpose(1, 0, 2), out_w)          # [out_w, h, 3]: a row's sums, at most 255 x 65535
    assert rows.max() < 1 << 24
    S, Ay = along(rows.transpose(1, 0, 2), out_h)                           # [out_h, out_w, 3]
    D = Ax * Ay
    assert S.min() >= 0 and S.max() <= 255 * D < 1 << 40 and D < 1 << 32
    R = ((2 * S + D) // (2 * D)).astype(np.uint8)
    return np.ascontiguousarray(R[:, ::-1]) if flip else R


def rule_by_taps(P, out_w, out_h):
    """the same from the tap lists, pixel by pixel: for small pictures"""
    h, w = P.shape[:2]
    R = np.zeros((out_h, out_w, 3), np.uint8)
    for oy in range(out_h):
        ys, wy, Ay = taps(h, out_h, oy)
        for ox in range(out_w):
            xs, wx, Ax = taps(w, out_w, ox)
            S = sum(a * b * P[y, x].astype(np.int64) for y, a in zip(ys, wy) for x, b in zip(xs, wx))
            R[oy, ox] = (2 * S + Ay * Ax) // (2 * Ay * Ax)
    return R


def section_18(P, out_w, out_h):
    """section 18's rule as DESIGN.md states it: four taps, weights in 1 / 256, (sum + 32768) >> 16"""
    h, w = P.shape[:2]
    y0, y1, fy = two_taps(h, out_h)
    x0, x1, fx = two_taps(w, out_w)
    P = P.astype(np.int64)
    fy, fx = fy[:, None, None], fx[None, :, None]
    acc = (256 - fx) * (256 - fy) * P[y0][:, x0] + fx * (256 - fy) * P[y0][:, x1] + (256 - fx) * fy * P[y1][:, x0] + fx * fy * P[y1][:, x1] + 32768
    return (acc >> 16).astype(np.uint8)


def row(v):
    return np.repeat(np.array(v, np.uint8)[None, :, None], 3, axis=2)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


# ---------------------------------------------------------------- without a GPU
def test_area_symbols_prototypes_and_constants(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    text = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    hdr = squeeze(text)
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 3
    for decl in decls:
        assert squeeze(decl) in hdr, decl
    for name, value in DEFINES.items():
        assert re.search(rf"^#define {name} {value}$", text, re.M), name
    import nhwcodec_amd as na
    assert na.FILTERS == {"two_tap": 0, "area": 1} and na.AREA_MAX_REDUCTION == LIMIT
    assert callable(na.Encoder.encode_pictures_resized) and callable(na.Encoder.encode_resized_device)


def test_the_area_rule_by_hand():
    line = lambda v, m, c=0, **kw: rule(row(v), m, 1, **kw)[0, :, c].tolist()
    assert line([0, 255, 0], 2) == [85, 85]
    assert line([10, 20, 40, 80, 160], 2) == [20, 104]
    assert line([10, 20, 40, 80, 160], 3, 1) == [14, 44, 128]
    assert line([10, 20, 40], 2, 2) == [13, 33]
    assert section_18(row([10, 20, 40]), 2, 1)[0, :, 2].tolist() == [13, 35]       # where the two-tap rule differs
    assert line([10, 20, 40], 2, flip=True) == [33, 13]
    assert line([0, 255], 3) == [0, 128, 255]                                    # an axis that grows: section 18
    assert rule(row([10, 20, 40, 80, 160]).transpose(1, 0, 2), 1, 2)[:, 0, 0].tolist() == [20, 104]   # the same down a column
    assert taps(5, 2, 0) == ([0, 1, 2], [2, 2, 1], 5) and taps(5, 2, 1) == ([2, 3, 4], [1, 2, 2], 5)
    assert taps(3, 2, 1) == ([1, 2], [1, 2], 3) and taps(2, 3, 1) == ([0, 1], [128, 128], 256)
    rng = np.random.default_rng(19)
    for (w, h), (ow, oh) in (((5, 3), (2, 2)), ((7, 1), (3, 4)), ((9, 8), (4, 11)), ((33, 17), (5, 3)), ((3, 5), (3, 5)), ((6, 4), (1, 1))):
        P = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(rule(P, ow, oh), rule_by_taps(P, ow, oh)), (w, h, ow, oh)       # the prefix sums and the tap lists agree


def test_area_rule_without_shrinking_is_section_18():
    rng = np.random.default_rng(190)
    pairs = [((1, 1), (1, 1)), ((1, 1), (5, 4)), ((5, 3), (5, 3)), ((7, 1), (7, 2)), ((1, 9), (300, 9)), ((33, 17), (224, 224)), ((64, 2), (4096, 2))]
    for _ in range(40):
        w, h = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        pairs.append(((w, h), (w + int(rng.integers(0, 3)) * int(rng.integers(0, 300)), h + int(rng.integers(0, 3)) * int(rng.integers(0, 300)))))
    assert sum(s[0] == o[0] for s, o in pairs) > 5 and sum(s[0] == 1 or s[1] == 1 for s, o in pairs) >= 4
    for (w, h), (ow, oh) in pairs:
        P = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(rule(P, ow, oh), section_18(P, ow, oh)), (w, h, ow, oh)
        if (w, h) == (ow, oh):
            assert np.array_equal(rule(P, ow, oh), P)


def test_integer_factors_constants_and_tap_weights():
    rng = np.random.default_rng(191)
    for k in (2, 3, 5):
        for ow, oh in ((1, 1), (7, 3), (16, 9)):
            P = rng.integers(0, 256, (k * oh, k * ow, 3), dtype=np.uint8)
            box = P.astype(np.int64).reshape(oh, k, ow, k, 3).sum(axis=(1, 3))
            assert np.array_equal(rule(P, ow, oh), (2 * box + k * k) // (2 * k * k))
            if k == 2:
                q = P.astype(np.int64)
                assert np.array_equal(rule(P, ow, oh), (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2)
    for v in (0, 1, 127, 254, 255):
        for (w, h), (ow, oh) in (((300, 200), (7, 300)), ((65535, 2), (512, 1)), ((129, 77), (2, 5)), ((5, 5), (9, 2))):
            assert (rule(np.full((h, w, 3), v, np.uint8), ow, oh) == v).all(), (v, w, h, ow, oh)
    most = {}
    for n, m in ((65535, 512), (65535, 4096), (128, 1), (4097, 4096), (300, 130), (7, 3)):
        assert n <= LIMIT * m
        most[n, m] = 0
        for o in range(m):
            idx, wts, A = taps(n, m, o)
            assert A == n == sum(wts) and min(wts) >= 1 and max(wts) <= m and idx == list(range(idx[0], idx[0] + len(idx))) and 0 <= idx[0] and idx[-1] < n
            assert all(x == m for x in wts[1:-1])                     # between the first and the last tap every weight is m
            most[n, m] = max(most[n, m], len(idx))
        assert most[n, m] <= 129
    assert most[65535, 512] == 129 and most[65535, 4096] == 17 and most[128, 1] == 128 and most[4097, 4096] == 2


def test_unknown_filter_raises_before_any_device():
    import nhwcodec_amd as na
    fmt = _fmt(*BYTES)
    for bad in ("bilinear", "AREA", "", None, 1, b"area"):
        with pytest.raises(na.NhwError, match="'two_tap', 'area'"):
            na.resize_to_tensor_device(["not a tensor"], (8, 8), fmt, filter=bad)
        with pytest.raises(na.NhwError, match="'two_tap', 'area'"):
            na.Decoder.decode_crops_device(object.__new__(na.Decoder), [b""], [(0, 0, 0, 1, 1)], (8, 8), fmt, filter=bad)


# ---------------------------------------------------------------- on the MI355X: the kernel alone
SRC_SIZES = [(1, 1), (2, 2), (3, 1), (5, 3), (7, 1), (33, 17), (128, 128), (256, 255), (300, 200)]      # W, H
OUT_SIZES = [(1, 1), (2, 1), (3, 2), (16, 16), (100, 75), (100, 299), (224, 224), (299, 299), (4096, 1)]   # W, H
ALL_32 = (100, 75)                                                  # the output size that meets all 32 formats
FLAGS = [0, 1, 0, 1, 1, 0, 1, 1, 0]


def within(src, out):
    return src[0] <= LIMIT * out[0] and src[1] <= LIMIT * out[1]


class Sources:
    """sizes -> views of one device buffer of random bytes (or of `fill`), every row followed by a gap of 1 .. bytes and every picture at an odd
    address; .own their bytes on the host; .table the nhw_picture table on the host; .rule(k, out_w, out_h, flip) the rule on source k, once"""

    def __init__(self, sizes, seed, fill=None):
        import torch
        import nhwcodec_amd as na
        at, places = 1, []
        for k, (w, h) in enumerate(sizes):
            pitch = 3 * w + 1 + 2 * (k % 5)
            places.append((at, pitch))
            at = (at + h * pitch + 7) | 1
        host = np.random.default_rng(seed).integers(0, 256, at + 64, dtype=np.uint8)
        if fill is not None:
            for (o, p), (w, h) in zip(places, sizes):
                for r in range(h):
                    host[o + r * p: o + r * p + 3 * w] = fill
        self.sizes = sizes
        self.own = [np.stack([host[o + r * p: o + r * p + 3 * w] for r in range(h)]).reshape(h, w, 3).copy() for (o, p), (w, h) in zip(places, sizes)]
        self.buf = torch.from_numpy(host).cuda()
        self.views = [self.buf.as_strided((h, w, 3), (p, 3, 1), o) for (o, p), (w, h) in zip(places, sizes)]
        assert all(v.data_ptr() % 2 == 1 for v in self.views)
        self.table = na._picture_table(self.views, "test")[0].cpu().numpy().view(na.PICTURE_DTYPE).copy()
        self._cache = {}

    def rule(self, k, out_w, out_h, flip=0):
        key = (k, out_w, out_h, bool(flip))
        if key not in self._cache:
            self._cache[key] = rule(self.own[k], out_w, out_h, bool(flip))
        return self._cache[key]


@pytest.fixture(scope="module")
def sources():
    return Sources(SRC_SIZES, 192)


def _guarded(n, per, fmt):
    """a canary-filled byte buffer with room for n tensors of `per` elements between two guards -> (buffer, the byte offset of tensor 0)"""
    import torch
    buf = torch.full((2 * GUARD + n * per * fmt.dtype.itemsize,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, GUARD


def _launch(table, out_w, out_h, fmt, flags=None, other_addr=None):
    """one launch of nhw_area_to_tensor_device over a host table into a guarded batch; other_addr: {entry: function of its slot's address} for
    the entries that get another address -> (rc, the batch's slots as byte arrays, guards intact)"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    n, per, es = len(table), 3 * out_w * out_h, fmt.dtype.itemsize
    buf, at = _guarded(n, per, fmt)
    slots = [buf.data_ptr() + at + i * per * es for i in range(n)]
    addr = torch.tensor([(other_addr or {}).get(i, int)(s) for i, s in enumerate(slots)], dtype=torch.int64, device="cuda")
    d_tab = torch.from_numpy(np.ascontiguousarray(table).view(np.int64).copy()).cuda()
    d_flags = torch.tensor(list(flags), dtype=torch.uint8, device="cuda") if flags is not None else None
    c = fmt.c_struct()
    rc = L.nhw_area_to_tensor_device(d_tab.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_flags.data_ptr() if d_flags is not None else None, addr.data_ptr(), None)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:at] == CANARY).all() and (host[at + n * per * es:] == CANARY).all())
    return rc, [host[at + i * per * es: at + (i + 1) * per * es] for i in range(n)], intact


def _same(got, px, fmt):
    want = expected_tensor(px, fmt)
    return np.array_equal(got.view(want.dtype).reshape(want.shape), want)


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h", OUT_SIZES)
def test_gpu_area_kernel_on_random_bytes(sources, out_w, out_h):
    """every source within the limit in one launch, flags mixed, also with a null flag table: under all 32 formats for one output size, under
    the two formats of section 18's tests for the others; the batch between guards; then the wrapper"""
    import nhwcodec_amd as na
    ks = [k for k, s in enumerate(SRC_SIZES) if within(s, (out_w, out_h))]
    assert len(ks) >= 7 and (len(ks) < len(SRC_SIZES)) == (out_w < 3 or out_h < 2)
    flags = [FLAGS[k] for k in ks]
    formats = [_fmt(*four, k=i // 2) for i, four in enumerate(ALL_FORMATS)] if (out_w, out_h) == ALL_32 else [_fmt(*BYTES), _fmt(*HALF)]
    for i, fmt in enumerate(formats):
        for fl in ((flags, None) if i % 4 == 0 else (flags,)):
            rc, slots, intact = _launch(sources.table[ks], out_w, out_h, fmt, fl)
            assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
            for j, k in enumerate(ks):
                assert _same(slots[j], sources.rule(k, out_w, out_h, fl[j] if fl else 0), fmt), f"{fmt} source {SRC_SIZES[k]} to {out_w} x {out_h}, flags {fl}"
    fmt = _fmt(*HALF)
    views = [sources.views[k] for k in ks]
    got = na.resize_to_tensor_device(views, (out_h, out_w), fmt, flips=[bool(f) for f in flags], filter="area")
    assert got.dtype == fmt.dtype and tuple(got.shape) == (len(ks), 3, out_h, out_w)
    bits = tensor_bits(got)
    for j, k in enumerate(ks):
        assert np.array_equal(bits[j], expected_tensor(sources.rule(k, out_w, out_h, flags[j]), fmt))
    plain = na.resize_to_tensor_device(views, (out_h, out_w), _fmt(*BYTES), filter="area").cpu().numpy()
    for j, k in enumerate(ks):
        assert np.array_equal(plain[j], sources.rule(k, out_w, out_h, 0))
    if len(ks) < len(SRC_SIZES):                                     # the wrapper knows the sizes: a picture beyond the limit raises
        with pytest.raises(na.NhwError, match="limit"):
            na.resize_to_tensor_device(sources.views, (out_h, out_w), fmt, filter="area")


@pytest.mark.gpu
def test_gpu_area_integer_edges():
    """the longest side at the largest reduction (129 taps), at the widest output (17 taps), a sum of 255s that needs all 40 bits of S / D, and
    a picture exactly at the limit on both axes: 128 x 128 taps under one pixel"""
    cases = [((65535, 2), (512, 1), None), ((65535, 1), (4096, 1), None), ((65535, 3), (512, 1), 255), ((128, 128), (1, 1), None), ((128, 128), (1, 1), 255)]
    for j, (size, (out_w, out_h), fill) in enumerate(cases):
        src = Sources([size], 193 + j, fill)
        want = src.rule(0, out_w, out_h)
        if fill is not None:
            assert (want == fill).all()
        for four, flag in ((BYTES, 0), (HALF, 1)):
            fmt = _fmt(*four)
            rc, slots, intact = _launch(src.table, out_w, out_h, fmt, [flag])
            assert rc == 0 and intact and _same(slots[0], src.rule(0, out_w, out_h, flag), fmt), (size, out_w, out_h, fill, fmt)


@pytest.mark.gpu
def test_gpu_area_entries_that_store_nothing(sources):
    """an entry one pixel beyond the limit on either axis, a zero side, an oversize side, a zero address and a misaligned one: their slots keep
    the canary, the other entries of the same launch are right"""
    edge = Sources([(129, 1), (128, 1), (1, 129), (1, 128)], 198)
    for four in (BYTES, HALF):
        fmt = _fmt(*four)
        rc, slots, intact = _launch(edge.table, 1, 1, fmt)                       # 129 x 1 -> 1 x 1 and 1 x 129 -> 1 x 1 are beyond it
        assert rc == 0 and intact
        assert (slots[0] == CANARY).all() and (slots[2] == CANARY).all()
        assert _same(slots[1], edge.rule(1, 1, 1), fmt) and _same(slots[3], edge.rule(3, 1, 1), fmt)
    out_w, out_h = 2, 200
    picks = [8, 7, 5, 6, 7, 5, 6, 7]                                 # 300 x 200 -> 2 x 200 is beyond the limit, 256 x 255 exactly at it
    tab = sources.table[picks]
    tab["width"][2] = 0
    tab["height"][3] = 65536
    for four in (HALF, ("float32", "HWC", "BGR", "file"), ("bfloat16", "HWC", "RGB", "file")):
        fmt = _fmt(*four)
        rc, slots, intact = _launch(tab, out_w, out_h, fmt, [1] * len(picks), {4: lambda a: 0, 5: lambda a: a + 1})   # no address; no multiple of the element size
        assert rc == 0 and intact
        for i, k in enumerate(picks):
            if i in (1, 6, 7):
                assert _same(slots[i], sources.rule(k, out_w, out_h, 1), fmt), (fmt, i)
            else:
                assert (slots[i] == CANARY).all(), (fmt, i)


@pytest.mark.gpu
def test_gpu_area_without_shrinking_equals_the_two_tap_kernel(sources):
    import nhwcodec_amd as na
    n = 0
    for out_w, out_h in ((300, 255), (301, 256), (512, 300), (4096, 1), (7, 3), (33, 17)):
        ks = [k for k, (w, h) in enumerate(SRC_SIZES) if w <= out_w and h <= out_h]
        views = [sources.views[k] for k in ks]
        flips = [bool(FLAGS[k]) for k in ks]
        for four in (BYTES, HALF):
            fmt = _fmt(*four)
            a = na.resize_to_tensor_device(views, (out_h, out_w), fmt, flips=flips, filter="area")
            b = na.resize_to_tensor_device(views, (out_h, out_w), fmt, flips=flips, filter="two_tap")
            c = na.resize_to_tensor_device(views, (out_h, out_w), fmt, flips=flips)
            assert np.array_equal(tensor_bits(a), tensor_bits(b)) and np.array_equal(tensor_bits(b), tensor_bits(c)), (out_w, out_h, fmt)
        n += len(ks)
    assert n >= 25


@pytest.mark.gpu
def test_gpu_area_many_entries_take_bands_of_64_rows():
    """4096 entries to 3 x 130: with so many a band has the most rows it can have, 64, so an entry is two full bands and one of two rows, and
    a pass of the workgroup walks 64 rows of 4 lanes; both axes shrink"""
    n, out_w, out_h = 4096, 3, 130
    src = Sources([(7, 300)] * 5, 199)
    which = np.arange(n) % 5
    flags = (np.arange(n) // 5) % 2
    fmt = _fmt("float16", "CHW", "BGR", "reversed")
    rc, slots, intact = _launch(src.table[which], out_w, out_h, fmt, flags.tolist())
    assert rc == 0 and intact
    got = np.stack(slots).view(np.uint16).reshape(n, 3, out_h, out_w)
    for k in range(5):
        for f in (0, 1):
            mine = got[(which == k) & (flags == f)]
            assert len(mine) > 400 and (mine == expected_tensor(src.rule(k, out_w, out_h, f), fmt)[None]).all(), (k, f)


# ---------------------------------------------------------------- on the MI355X: the host paths
@pytest.fixture(scope="module")
def world():
    """the crops' pictures (SIZES: 1 x 700, 500 x 375, 1023 x 1025, crops of one seeded scene of generated images) as containers at q20, a
    decoder of 4 tiles a chunk, and the encoder and the scene for the encode tests"""
    import nhwcodec_amd as na
    w = World()
    w.enc = na.Encoder(0, max_batch=24)
    w.scene = na.untile_images(w.enc.synth_device(24, 1300).cpu().numpy(), 4, 6)
    w.pics = [np.ascontiguousarray(w.scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES]
    w.containers = w.enc.encode_pictures(w.pics, 20)
    w.dec = na.Decoder(0, max_batch=4)
    yield w
    w.dec.close()
    w.enc.close()


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


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h,four", [(32, 24, BYTES), (224, 224, HALF)])
@pytest.mark.parametrize("scale", SCALES)
def test_gpu_area_crops_equal_the_rule_on_decode_windows(world, scale, out_w, out_h, four):
    """40 seeded crops with flips in one call on a decoder of max_batch 4; the statistics are those of the two-tap call; then the crops
    shuffled, into a tensor of the caller's"""
    import torch
    fmt = _fmt(*four)
    rng = np.random.default_rng(1900 + 10 * scale + out_w)
    rects = seeded_windows(scale, 40, rng)
    flips = [bool(v) for v in rng.integers(0, 2, len(rects))]
    assert 8 < sum(flips) < 32 and sum(r[3] > out_w or r[4] > out_h for r in rects) >= 5                 # crops with an axis that shrinks ...
    assert sum(r[3] > out_w and r[4] < out_h or r[3] < out_w and r[4] > out_h for r in rects) >= 4            # ... while the other grows
    assert out_w > 32 or sum(r[3] >= 2 * out_w or r[4] >= 2 * out_h for r in rects) >= 30                     # ... by 2 and more, where two taps alias
    wins = world.dec.decode_windows(world.containers, rects, scale)
    world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, flips=flips, scale=scale)
    stats = world.dec.region_stats()
    got, scales = world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, flips=flips, scale=scale, filter="area")
    assert scales == [scale] * len(rects) and got.dtype == fmt.dtype and tuple(got.shape) == (len(rects),) + fmt.shape(out_h, out_w)
    assert world.dec.region_stats() == stats == expected_stats(world.containers, rects, scale, unique=True)
    bits = tensor_bits(got)
    for i, (r, P, f) in enumerate(zip(rects, wins, flips)):
        assert P.shape == (r[4], r[3], 3)
        assert np.array_equal(bits[i], expected_tensor(rule(P, out_w, out_h, f), fmt)), (scale, r, f)
    perm = rng.permutation(len(rects))
    per = 3 * out_w * out_h
    mine = torch.full((len(rects) * per + 64,), 1, dtype=fmt.dtype, device="cuda")
    before = tensor_bits(mine[len(rects) * per:]).copy()
    again, _ = world.dec.decode_crops_device(world.containers, [rects[i] for i in perm], (out_h, out_w), fmt, flips=[flips[i] for i in perm], scale=scale, out=mine,
                                             filter="area")
    assert again.data_ptr() == mine.data_ptr() and world.dec.region_stats() == stats
    assert np.array_equal(tensor_bits(again), bits[perm])
    assert np.array_equal(tensor_bits(mine[len(rects) * per:]), before)


@pytest.mark.gpu
def test_gpu_area_crops_choose_their_scale_as_before(world):
    """full-resolution crops of the pictures to 64 x 48 with scale=None: the scales and windows are crop_scale's and crop_window's, all three
    scales in one call, and every crop is the rule on its window"""
    import nhwcodec_amd as na
    W, H = SIZES[BIG]
    out_w, out_h = 64, 48
    rng = np.random.default_rng(195)
    crops = [(BIG, 0, 0, W, H), (BIG, W - 256, H - 192, 256, 192), (BIG, W - 255, H - 192, 255, 192), (BIG, 511, 513, 128, 96), (BIG, 300, 1, 127, 96),
             (BIG, W - 31, H - 17, 31, 17), (BIG, 5, 7, 64, 48), (1, 0, 0, 500, 375), (1, 100, 100, 200, 97), (0, 0, 100, 1, 500), (BIG, 0, 300, W, 60)]
    for _ in range(25):
        w, h = int(rng.integers(8, 600)), int(rng.integers(8, 600))
        crops.append((BIG, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    flips = [bool(v) for v in rng.integers(0, 2, len(crops))]
    fmt = _fmt("float32", "CHW", "RGB", "reversed", k=1)
    got, scales = world.dec.decode_crops_device(world.containers, crops, (out_h, out_w), fmt, flips=flips, filter="area")
    assert scales == world.dec.decode_crops_device(world.containers, crops, (out_h, out_w), fmt, flips=flips)[1] == [na.crop_scale(w, h, out_w, out_h) for _, _, _, w, h in crops]
    assert scales[:7] == [4, 4, 2, 2, 1, 1, 1] and scales[10] == 1 and all(scales.count(s) >= 4 for s in SCALES)   # crop 10: 1023 x 60, a reduction of 16 left to the filter
    bits = tensor_bits(got)
    for s in SCALES:
        idx = [i for i, v in enumerate(scales) if v == s]
        rects = [(crops[i][0], *na.crop_window(*crops[i][1:], s)) for i in idx]
        for i, P in zip(idx, world.dec.decode_windows(world.containers, rects, s)):
            assert np.array_equal(bits[i], expected_tensor(rule(P, out_w, out_h, flips[i]), fmt)), (s, crops[i])
    stats = world.dec.region_stats()
    with pytest.raises(na.NhwError, match="limit"):                  # 700 rows to 5: raised before any call
        world.dec.decode_crops_device(world.containers, [(1, 0, 0, 10, 10), (0, 0, 0, 1, 700)], (5, 5), fmt, filter="area")
    assert world.dec.region_stats() == stats


def _call_crops(dec, containers, rects, scale, out_w, out_h, fmt, flags, addrs, filter=None):
    """nhw_dec_crops_to_device (filter None) or nhw_dec_crops_to_device_filter by ctypes -> (rc, status)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    addr = np.array(addrs, np.uint64)
    f = np.array(flags, np.uint8) if flags is not None else None
    c = fmt.c_struct()
    args = (dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out_w, out_h, ctypes.byref(c),
            f.ctypes.data if f is not None else None, addr.ctypes.data, status.ctypes.data)
    rc = dec.lib.nhw_dec_crops_to_device(*args) if filter is None else dec.lib.nhw_dec_crops_to_device_filter(*args, filter)
    return rc, status


@pytest.mark.gpu
def test_gpu_crops_filter_argument(world):
    """filter 0 is nhw_dec_crops_to_device byte for byte; with filter 1 a rect beyond the limit is NHW_E_ARG, selects no tile and keeps its
    slot's canary while its neighbours are right; filter 2 is refused at call level and nothing is launched"""
    import torch
    rng = np.random.default_rng(196)
    fmt = _fmt(*HALF)
    out_w, out_h = 32, 24
    per, es = 3 * out_w * out_h, 2
    rects = seeded_windows(2, 12, rng)
    flips = [i % 3 == 0 for i in range(len(rects))]
    results = []
    for filter in (None, 0):
        buf, at = _guarded(len(rects), per, fmt)
        rc, status = _call_crops(world.dec, world.containers, rects, 2, out_w, out_h, fmt, flips, [buf.data_ptr() + at + i * per * es for i in range(len(rects))], filter)
        torch.cuda.synchronize()
        assert rc == 0 and not status.any()
        results.append((buf.cpu().numpy(), world.dec.region_stats()))
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1] == expected_stats(world.containers, rects, 2, unique=True)
    assert (results[0][0][GUARD:-GUARD] != CANARY).any()
    # beyond the limit: 300 columns to 2.  The rect alone selects tile (ty 2, tx 1) of the large picture, which no other rect touches
    out_w, out_h = 2, 2
    per = 3 * out_w * out_h
    rects = [(BIG, 0, 0, 100, 50), (BIG, 600, 1024, 300, 1), (BIG, 600, 1024, 256, 1), (1, 10, 10, 256, 256), (BIG, 0, 0, 257, 5), (1, 0, 0, 5, 257), (BIG, 3, 3, 30, 30)]
    bad = [False, True, False, False, True, True, False]
    ok = [r for r, b in zip(rects, bad) if not b]
    buf, at = _guarded(len(rects), per, fmt)
    rc, status = _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, fmt, None, [buf.data_ptr() + at + i * per * es for i in range(len(rects))], 1)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_ARG if b else 0 for b in bad]
    assert world.dec.region_stats() == expected_stats(world.containers, ok, 1, unique=True)
    assert world.dec.region_stats()[0] == expected_stats(world.containers, ok[:1] + ok[2:], 1, unique=True)[0] + 1   # the tile of rect 2 is there for rect 2 alone
    host = buf.cpu().numpy()
    wins = iter(world.dec.decode_windows(world.containers, ok, 1))
    for i, b in enumerate(bad):
        got = host[at + i * per * es: at + (i + 1) * per * es]
        if b:
            assert (got == CANARY).all(), rects[i]
        else:
            assert _same(got, rule(next(wins), out_w, out_h), fmt), rects[i]
    assert (host[:at] == CANARY).all() and (host[at + len(rects) * per * es:] == CANARY).all()
    rc, status = _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, fmt, None, [buf.data_ptr() + at + i * per * es for i in range(len(rects))], 0)
    assert rc == 0 and not status.any()                              # the two-tap filter has no limit
    # an unknown filter
    stats = world.dec.region_stats()
    buf.fill_(CANARY)
    for filter in (2, -1, 256):
        rc, status = _call_crops(world.dec, world.containers, ok, 1, out_w, out_h, fmt, None, [buf.data_ptr() + at + i * per * es for i in range(len(ok))], filter)
        assert rc == NHW_E_ARG and (status == 99).all() and b"filter" in world.dec.lib.nhw_dec_last_error()
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and world.dec.region_stats() == stats


ENC_SIZES = [(700, 500), (513, 1), (1024, 1024)]                    # W, H
ENC_OUT = [(512, 512), (600, 300)]                                  # W, H: one tile, two tiles


def _enc_pictures(world):
    return [np.ascontiguousarray(world.scene[301:301 + h, 1203:1203 + w]) for w, h in ENC_SIZES]


@pytest.mark.gpu
@pytest.mark.parametrize("quality", (20, 10))
def test_gpu_encode_pictures_resized(world, quality):
    """container for container, encode_pictures_resized is encode_pictures of the rule's pictures"""
    import nhwcodec_amd as na
    pics = _enc_pictures(world)
    for out_w, out_h in ENC_OUT:
        want = world.enc.encode_pictures([rule(p, out_w, out_h) for p in pics], quality)
        got = world.enc.encode_pictures_resized(pics, (out_h, out_w), quality)
        assert [na.picture_info(c) for c in got] == [(out_w, out_h)] * len(pics)
        assert got == want, [len(a) == len(b) for a, b in zip(got, want)]
    assert world.enc.encode_pictures_resized(pics[1:2], (1, 513), quality) == world.enc.encode_pictures(pics[1:2], quality)   # its own size: the picture itself


@pytest.mark.gpu
def test_gpu_encode_resized_device(world):
    """three photos, one of them a crop view of a larger tensor, to one .nhw file each: the files, sizes and status of encode_device on the
    rule's 512 x 512 pictures"""
    import torch
    import nhwcodec_amd as na
    host = [np.ascontiguousarray(world.scene[40:40 + 1100, 100:100 + 1500]), np.ascontiguousarray(world.scene[900:900 + 333, 2000:2000 + 777])]
    large = torch.from_numpy(np.ascontiguousarray(world.scene[:1300, :1700])).cuda()
    view = large[211:211 + 1025, 307:307 + 1023]
    assert not view.is_contiguous()
    pictures = [torch.from_numpy(host[0]).cuda(), view, torch.from_numpy(host[1]).cuda()]
    ruled = np.stack([rule(p, 512, 512) for p in (host[0], view.cpu().numpy(), host[1])])
    want = world.enc.encode_device(torch.from_numpy(ruled).cuda(), 17)
    got = world.enc.encode_resized_device(pictures, 17)
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and not bool(got[2].any()) and same_files(got[0], want[0], want[1])
    out = world.enc.alloc_out(3)
    again = world.enc.encode_resized_device(pictures, 17, out=out)
    assert again[0].data_ptr() == out[0].data_ptr() and torch.equal(again[1], want[1]) and same_files(again[0], want[0], want[1])
    with pytest.raises(na.NhwError):
        world.enc.encode_resized_device(pictures * 9)                # 27 pictures for an encoder of max_batch 24
    with pytest.raises(na.NhwError):
        world.enc.encode_resized_device([large[:, :, :2]])           # no [H, W, 3] picture


@pytest.mark.gpu
def test_gpu_encode_resized_refusals_launch_nothing(world):
    import nhwcodec_amd as na
    L = world.enc.lib
    pic = np.ascontiguousarray(world.scene[:300, :200])
    blob = pic.reshape(-1)
    in_off = np.array([0, blob.size], np.uint64)
    arena = np.full(1 << 20, CANARY, np.uint8)
    off = np.full(2, 77, np.uint64)
    status = np.full(1, 99, np.int32)

    def call(w, h, out_w, out_h, quality=20):
        width, height = np.array([w], np.uint32), np.array([h], np.uint32)
        return L.nhw_enc_pictures_resized(world.enc.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, 1, out_w, out_h, quality,
                                          arena.ctypes.data, arena.size, off.ctypes.data, status.ctypes.data)
    for out_w, out_h in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert call(200, 300, out_w, out_h) == NHW_E_ARG and b"1 .. 4096" in L.nhw_last_error(), (out_w, out_h)
    for out_w, out_h in ((1, 8), (8, 2)):                            # 200 > 128 x 1, 300 > 128 x 2
        assert call(200, 300, out_w, out_h) == NHW_E_ARG and b"128 times" in L.nhw_last_error(), (out_w, out_h)
    assert call(0, 300, 8, 8) == NHW_E_ARG and call(200, 65536, 512, 512) == NHW_E_ARG
    assert call(200, 300, 8, 8, quality=24) != 0
    assert (arena == CANARY).all() and (off == 77).all() and (status == 99).all()
    for size in ((0, 8), (8, 4097), 8):
        with pytest.raises(na.NhwError):
            world.enc.encode_pictures_resized([pic], size)
    with pytest.raises(na.NhwError, match="limit"):
        world.enc.encode_pictures_resized([pic], (2, 8))
    assert call(200, 300, 2, 3) == 0 and status[0] == 0 and na.picture_info(bytes(arena[:int(off[1])])) == (2, 3)   # exactly at the limit: it runs


# ---------------------------------------------------------------- nhw-enc --resize
def _bmp(pic):
    """a 24-bit bottom-up BMP of pic (rows in file order), rows padded to 4 bytes"""
    h, w = pic.shape[:2]
    stride = (3 * w + 3) & ~3
    body = b"".join(r.tobytes() + b"\0" * (stride - 3 * w) for r in pic)
    return struct.pack("<2sIHHIIiiHHIIiiII", b"BM", 54 + len(body), 0, 0, 54, 40, w, h, 1, 24, 0, len(body), 0, 0, 0, 0) + body


@pytest.fixture(scope="module")
def cli():
    return built_cli("nhw-enc")


@pytest.mark.parametrize("args,message", [(("IN", "OUT", "--resize", "600x300"), "--resize works with --picture only"),
                                          (("--picture", "IN", "OUT", "--resize", "600"), "--resize wants <W>x<H>"),
                                          (("--picture", "IN", "OUT", "--resize", "600x4097"), "the sides must be 1..4096"),
                                          (("--picture", "IN", "OUT", "--resize", "1x300"), "more than 128 times")])
def test_cli_resize_misuse(cli, tmp_path, args, message):
    """each with its one line and exit code 1, before any work on a device: in.bmp is 129 x 2"""
    (tmp_path / "in.bmp").write_bytes(_bmp(np.zeros((2, 129, 3), np.uint8)))
    names = {"IN": str(tmp_path / "in.bmp"), "OUT": str(tmp_path / "out.nhwp")}
    rc, out, err = run(cli, "-q20", *[names.get(a, a) for a in args])
    assert rc == 1 and message in err and len(err.strip().splitlines()) == 1 and not (tmp_path / "out.nhwp").exists(), (rc, out, err)
    assert "--resize" in run(cli, "-h")[1]


@pytest.mark.gpu
def test_gpu_cli_resize(world, cli, tmp_path):
    pic = _enc_pictures(world)[0]
    (tmp_path / "in.bmp").write_bytes(_bmp(pic))
    rc, out, err = run(cli, "-q20", "--picture", str(tmp_path / "in.bmp"), str(tmp_path / "out.nhwp"), "--resize", "600x300")
    assert rc == 0 and "600 x 300" in out, err
    want = world.enc.encode_pictures([rule(pic, 600, 300)], 20)[0]
    assert (tmp_path / "out.nhwp").read_bytes() == want and parse_container(want)[:2] == (600, 300)
    rc, out, err = run(cli, "-q20", "--resize", "600x300", "--picture", str(tmp_path / "in.bmp"), str(tmp_path / "front.nhwp"))   # the option in front
    assert rc == 0 and (tmp_path / "front.nhwp").read_bytes() == want, err
