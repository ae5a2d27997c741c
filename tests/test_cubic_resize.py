"""The cubic filter: the rule, the kernel k_cubic_to_tensor behind nhw_resample_to_tensor_device, the host call
nhw_dec_crops_to_device_resample and the Python wrappers (resize_to_tensor_device, Decoder.decode_crops_device and
Encoder.encode_resized_device with filter="cubic").  The rule -- the Keys cubic with a = -1/2, its support widened with the reduction, in
integers -- is stated here in numpy's int64 with floor divisions and arithmetic shifts, and held against torch's CPU bicubic with antialias as
an outside yardstick.  Every comparison with the product is exact: bytes for uint8, bit patterns for the floats."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests.picture_cases import SIZES, Rect, World, expected_stats
from tests.support import CANARY, ROOT, load_lib, same_files
from tests.tensor_cases import ALL_FORMATS, expected_tensor, tensor_bits

NEW_SYMBOLS = ("nhw_resample_to_tensor_device", "nhw_dec_crops_to_device_resample")
PROTOTYPES = """
int nhw_resample_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                  const uint8_t *d_flags, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_to_device_resample(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                     uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const uint64_t *dst_addr,
                                     int *status, int filter);
"""
DEFINES = {"NHW_FILTER_CUBIC": 2, "NHW_CUBIC_MAX_REDUCTION": 32}
NHW_E_ARG = -4
CUBIC = 2
LIMIT = 32
GUARD = 4096                                                        # canary bytes kept in front of and behind a batch
SCALES = (1, 2, 4)
BIG = 2                                                             # 1023 x 1025: a 2 x 3 grid of tiles, odd sides

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
NEGATIVE = dict(scale=(-1 / 255, -0.5, -2.0), bias=(1.0, 127.5, 3.25))
BYTES = ("uint8", "HWC", "BGR", "file")
HALF = ("float16", "CHW", "RGB", "reversed")


def _fmt(dtype, layout, channels, rows, k=0):
    """the TensorFormat of a parameter tuple; the float types take the ImageNet constants and a set with negative scales in turn"""
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, channels, rows)
    return na.TensorFormat(dtype, layout, channels, rows, **(IMAGENET, NEGATIVE)[k % 2])


# ---------------------------------------------------------------- the rule, in the test's own words
def floor_div(a, b):
    return a // b                                                   # numpy's and Python's // floor, also below zero


def trunc_div(a, b):
    """C's division, toward zero: what the rule does NOT use"""
    a = np.asarray(a, dtype=np.int64)
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def raw(U):
    """the Keys cubic with a = -1/2 times 2^31 at U / 1024, int64, for 0 <= U < 2048"""
    U = np.asarray(U, dtype=np.int64)
    return np.where(U <= 1024, 3 * U**3 - 5120 * U**2 + (1 << 31), -U**3 + 5120 * U**2 - (8 << 20) * U + (1 << 32))


@functools.lru_cache(maxsize=None)
def runs(n, m, div=floor_div):
    """the taps of every output index of an axis of source length n and output length m -> [(first source index, weights int64)], straight
    from the definition: U of every source pixel near the output's centre, the taps those with U < 2048"""
    D = max(n, m)
    out = []
    for o in range(m):
        centre = (2 * o + 1) * n
        lo, hi = max((centre - 4 * D) // (2 * m) - 2, 0), min((centre + 4 * D) // (2 * m) + 2, n - 1)
        i = np.arange(lo, hi + 1, dtype=np.int64)
        N = np.abs((2 * i + 1) * m - centre)
        U = (N * 1024 + D) // (2 * D)
        assert N.max() < 1 << 31 and (U[0] >= 2048 or lo == 0) and (U[-1] >= 2048 or hi == n - 1)     # the candidates reach past the support
        inside = np.flatnonzero(U < 2048)
        assert len(inside) and (np.diff(inside) == 1).all() and N[inside].max() < 4 * D < 1 << 19, (n, m, o)   # one contiguous run
        r = raw(U[inside])
        R = int(r.sum())
        assert R > 0, (n, m, o)
        q = div(r * (1 << 15) + R, 2 * R)
        q[int(np.argmax(q))] += (1 << 14) - int(q.sum())             # argmax: the first of the largest
        out.append((int(i[inside[0]]), q))
    return out


def rule(P, out_w, out_h, flip=False, div=floor_div, limit=LIMIT):
    """P uint8 [h, w, 3] -> R uint8 [out_h, out_w, 3] under the cubic rule, mirrored left-right with `flip`.  (limit: the arithmetic
    itself does not need the reduction limit, and one CPU case below looks beyond it)"""
    h, w = P.shape[:2]
    assert 1 <= w <= 65535 and 1 <= h <= 65535 and w <= limit * out_w and h <= limit * out_h
    P = P.astype(np.int64)
    Hh = np.empty((h, out_w, 3), np.int64)
    for ox, (first, q) in enumerate(runs(w, out_w, div)):
        S = (P[:, first:first + len(q)] * q[None, :, None]).sum(axis=1)
        assert np.abs(S).max() < 1 << 23
        Hh[:, ox] = div(S + 128, 256)                                # for the floor: (S + 128) >> 8
    assert np.abs(Hh).max() < 1 << 15
    R = np.empty((out_h, out_w, 3), np.uint8)
    for oy, (first, q) in enumerate(runs(h, out_h, div)):
        V = (Hh[first:first + len(q)] * q[:, None, None]).sum(axis=0)
        assert np.abs(V).max() < 1 << 30
        R[oy] = np.clip(div(V + (1 << 19), 1 << 20), 0, 255)
    return np.ascontiguousarray(R[:, ::-1]) if flip else R


def row(v):
    return np.repeat(np.array(v, np.uint8)[None, :, None], 3, axis=2)


def line(v, m, c=0, **kw):
    return rule(row(v), m, 1, **kw)[0, :, c].tolist()


def weights(n, m, o):
    return runs(n, m)[o][1].tolist()


@pytest.fixture(scope="module")
def lib():
    return load_lib()


# ---------------------------------------------------------------- without a GPU
def test_cubic_symbols_prototypes_and_constants(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    text = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    hdr = squeeze(text)
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 2
    for decl in decls:
        assert squeeze(decl) in hdr, decl
    for name, value in DEFINES.items():
        assert re.search(rf"^#define {name} {value}$", text, re.M), name
    import nhwcodec_amd as na
    assert na.RESAMPLERS == {"two_tap": 0, "area": 1, "cubic": 2} and list(na.RESAMPLERS) == ["two_tap", "area", "cubic"]
    assert na.CUBIC_MAX_REDUCTION == LIMIT
    assert na.FILTERS == {"two_tap": 0, "area": 1} and na.AREA_MAX_REDUCTION == 128


def test_the_cubic_rule_by_hand():
    assert int(raw(0)) == 1 << 31 and int(raw(1024)) == 0 and int(raw(2047)) < 0 and int(raw(1025)) < 0 and int(raw(1023)) > 0
    assert int(-np.int64(2048)**3 + 5120 * np.int64(2048)**2 - (8 << 20) * np.int64(2048) + (1 << 32)) == 0       # r(2048) = 0
    assert line([100], 4) == [100, 100, 100, 100]
    assert line([0, 255], 3) == [0, 128, 255]
    assert [weights(2, 3, o) for o in range(3)] == [[17464, -1080], [8192, 8192], [-1080, 17464]]
    assert line([10, 20, 40], 2, 1) == [13, 33]
    assert weights(3, 2, 0) == [10650, 6392, -658] and weights(3, 2, 1) == [-658, 6392, 10650]
    assert line([0, 255, 0], 2, 2) == [99, 99]                                   # the area rule gives 85: the lobes sharpen
    assert line([10, 20, 40, 80, 160], 2) == [19, 99]
    assert weights(5, 2, 0) == [5688, 6811, 3922, 475, -512] and weights(5, 2, 1) == [-512, 475, 3922, 6811, 5688]
    assert line([0, 0, 255, 255], 8) == [0, 0, 0, 52, 203, 255, 255, 255]        # the undershoot and the overshoot are clamped
    assert rule(row([10, 20, 40, 80, 160]).transpose(1, 0, 2), 1, 2)[:, 0, 0].tolist() == [19, 99]   # the same down a column
    assert line([10, 20, 40, 80, 160], 2, flip=True) == [99, 19]                 # ... and mirrored
    assert line([10, 20, 40], 2, flip=True) == [33, 13]
    long = runs(65535, 2048)
    assert max(len(q) for _, q in long) == 128 and min(len(q) for _, q in long[64:-64]) >= 127


def test_identity_constants_and_negative_lobes():
    rng = np.random.default_rng(20)
    for w, h in [(1, 1), (1, 7), (9, 1), (11, 9), (64, 33)] + [(int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(6)]:
        P = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(rule(P, w, h), P), (w, h)
        assert all(sorted(q.tolist())[-1] == 16384 and not np.delete(np.sort(q), -1).any() for _, q in runs(w, w))   # one tap of 16384
    for v in (0, 1, 127, 254, 255):
        for (w, h), (ow, oh) in (((300, 200), (7, 300)), ((65535, 2), (2048, 1)), ((5, 5), (9, 2))):
            assert (rule(np.full((h, w, 3), v, np.uint8), ow, oh, limit=64) == v).all(), (v, w, h, ow, oh)   # (300 to 7 lies beyond the limit of 32)
    # a division that truncates toward zero: the weights of the negative lobes and the negative H differ, and so do bytes
    assert any((a[1] != b[1]).any() for a, b in zip(runs(5, 2), runs(5, 2, trunc_div)))
    assert [q.tolist() for _, q in runs(2, 3, trunc_div)][0] != [17464, -1080]
    P = np.random.default_rng(21).integers(0, 256, (9, 12, 3), dtype=np.uint8)
    P[:, :6] //= 16                                                                # a dark half beside a bright one: undershoot below zero
    S = np.stack([(P[:, first:first + len(q)].astype(np.int64) * q[None, :, None]).sum(axis=1) + 128 for first, q in runs(12, 24)])
    assert (S < 0).sum() >= 20 and (trunc_div(S, 256) != S >> 8).sum() >= 10       # negative numerators of H, and where the two divisions part
    assert not np.array_equal(rule(P, 24, 18), rule(P, 24, 18, div=trunc_div))


AXES = [(65535, 2048), (65535, 4096), (64, 2), (4097, 4096), (300, 130), (7, 3), (1, 5), (3, 4096)]
MOST_ABS = 20484                                                    # the largest sum |q| of the axes above (DESIGN.md section 20 records it)


def test_axis_checks():
    most_taps, most_abs = 0, 0
    for n, m in AXES:
        assert n <= LIMIT * m
        for o, (first, q) in enumerate(runs(n, m)):
            assert len(q) >= 1 and 0 <= first and first + len(q) <= n, (n, m, o)   # (that the run is contiguous and R positive: runs())
            assert int(q.sum()) == 16384, (n, m, o)
            most_taps, most_abs = max(most_taps, len(q)), max(most_abs, int(np.abs(q).sum()))
    assert most_taps <= 129
    assert most_abs < 1 << 15
    assert most_abs == MOST_ABS, most_abs


YARDSTICK = [((300, 200), (224, 224)), ((500, 375), (224, 224)), ((33, 17), (16, 16)), ((64, 48), (100, 75)), ((1000, 700), (96, 64)), ((7, 5), (4, 5)),
             ((256, 255), (32, 24))]


@pytest.mark.parametrize("src,out", YARDSTICK)
def test_the_rule_against_torch_bicubic_antialias(src, out):
    """the rule against an outside implementation of the same filter in float64: no byte is more than 1 from torch's rounded, clipped value.
    (Observed over these pairs, printed below and recorded, not gated: at most 0.666 from the clipped real value; 12.0 % of the bytes differ
    on the smooth 256 x 255 -> 32 x 24, elsewhere at most 2.7 %.)"""
    import torch
    import torch.nn.functional as F
    (w, h), (ow, oh) = src, out
    rng = np.random.default_rng(200 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), xx * 255 / max(w - 1, 1), yy * 255 / max(h - 1, 1)], -1).astype(np.uint8)
    for kind, P in (("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), ("smooth", smooth)):
        t = torch.from_numpy(P).permute(2, 0, 1)[None].double()
        T = F.interpolate(t, size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
        got = rule(P, ow, oh).astype(np.int64)
        d = np.abs(got - np.clip(np.floor(T + 0.5), 0, 255))
        print(f"{w} x {h} -> {ow} x {oh} {kind}: largest byte difference {int(d.max())}, share of differing bytes {(d > 0).mean():.4f}, "
              f"largest real difference {np.abs(got - np.clip(T, 0, 255)).max():.3f}")
        assert d.max() <= 1, (src, out, kind)


def test_cubic_refusals_before_any_device():
    import nhwcodec_amd as na
    fmt = _fmt(*BYTES)
    for bad in ("bicubic", "CUBIC", "", None, 2, b"cubic"):
        with pytest.raises(na.NhwError, match="'two_tap', 'area', 'cubic'"):
            na.resize_to_tensor_device(["not a tensor"], (8, 8), fmt, filter=bad)
        with pytest.raises(na.NhwError, match="'two_tap', 'area', 'cubic'"):
            na.Decoder.decode_crops_device(object.__new__(na.Decoder), [b""], [(0, 0, 0, 1, 1)], (8, 8), fmt, filter=bad)

    import torch
    for shape in ((2, 65, 3), (65, 2, 3)):                           # host tensors: the limit is looked at before where they live
        with pytest.raises(na.NhwError, match="cubic filter's limit"):
            na.resize_to_tensor_device([torch.zeros((1, 1, 3), dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8)], (2, 2), fmt, filter="cubic")
    with pytest.raises(na.NhwError, match="CUDA"):                   # ... and at the limit the next check speaks
        na.resize_to_tensor_device([torch.zeros((64, 64, 3), dtype=torch.uint8)], (2, 2), fmt, filter="cubic")
    dec = object.__new__(na.Decoder)                                 # no handle, no device: the limit raises before either is needed
    dec.torch = torch
    for crops, scale in (([(0, 0, 0, 10, 10), (0, 3, 3, 65, 2)], 1), ([(0, 0, 0, 2, 65)], 2), ([(0, 0, 0, 8, 8), (0, 0, 0, 300, 8)], None)):
        with pytest.raises(na.NhwError, match="cubic filter's limit"):
            dec.decode_crops_device([b"no container"], crops, (2, 2), fmt, scale=scale, filter="cubic")


# ---------------------------------------------------------------- on the MI355X: the kernel alone
SRC_SIZES = [(1, 1), (2, 2), (3, 1), (5, 3), (7, 1), (33, 17), (128, 128), (256, 255), (300, 200)]      # W, H
OUT_SIZES = [(1, 1), (3, 2), (16, 16), (100, 75), (224, 224), (299, 299), (4096, 1)]                    # W, H
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
        key = (k, out_w, out_h)
        if key not in self._cache:
            self._cache[key] = rule(self.own[k], out_w, out_h)
        R = self._cache[key]
        return np.ascontiguousarray(R[:, ::-1]) if flip else R


@pytest.fixture(scope="module")
def sources():
    return Sources(SRC_SIZES, 202)


def _guarded(n, per, fmt):
    """a canary-filled byte buffer with room for n tensors of `per` elements between two guards -> (buffer, the byte offset of tensor 0)"""
    import torch
    buf = torch.full((2 * GUARD + n * per * fmt.dtype.itemsize,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, GUARD


def _launch(table, out_w, out_h, fmt, flags=None, other_addr=None, filter=CUBIC, entry=None):
    """one launch of nhw_resample_to_tensor_device (or of the entry named, which takes no filter) over a host table into a guarded batch;
    other_addr: {entry: function of its slot's address} for the entries that get another address -> (rc, the batch's slots as byte arrays,
    guards intact)"""
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
    rest = (ctypes.byref(c), d_flags.data_ptr() if d_flags is not None else None, addr.data_ptr(), None)
    if entry is None:
        rc = L.nhw_resample_to_tensor_device(d_tab.data_ptr(), n, out_w, out_h, filter, *rest)
    else:
        rc = getattr(L, entry)(d_tab.data_ptr(), n, out_w, out_h, *rest)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:at] == CANARY).all() and (host[at + n * per * es:] == CANARY).all())
    return rc, [host[at + i * per * es: at + (i + 1) * per * es] for i in range(n)], intact


def _same(got, px, fmt):
    want = expected_tensor(px, fmt)
    return np.array_equal(got.view(want.dtype).reshape(want.shape), want)


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h", OUT_SIZES)
def test_gpu_cubic_kernel_on_random_bytes(sources, out_w, out_h):
    """every source within the limit in one launch, flags mixed, also with a null flag table: under all 32 formats for one output size, under
    two formats for the others; the batch between guards; then the wrapper"""
    import nhwcodec_amd as na
    ks = [k for k, s in enumerate(SRC_SIZES) if within(s, (out_w, out_h))]
    assert len(ks) >= 5 and (len(ks) < len(SRC_SIZES)) == (out_w < 16 or out_h < 16)
    flags = [FLAGS[k] for k in ks]
    formats = [_fmt(*four, k=i // 2) for i, four in enumerate(ALL_FORMATS)] if (out_w, out_h) == ALL_32 else [_fmt(*BYTES), _fmt(*HALF)]
    assert len(formats) in (2, 32)
    for i, fmt in enumerate(formats):
        for fl in ((flags, None) if i % 4 == 0 else (flags,)):
            rc, slots, intact = _launch(sources.table[ks], out_w, out_h, fmt, fl)
            assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
            for j, k in enumerate(ks):
                assert _same(slots[j], sources.rule(k, out_w, out_h, fl[j] if fl else 0), fmt), f"{fmt} source {SRC_SIZES[k]} to {out_w} x {out_h}, flags {fl}"
    fmt = _fmt(*HALF)
    views = [sources.views[k] for k in ks]
    got = na.resize_to_tensor_device(views, (out_h, out_w), fmt, flips=[bool(f) for f in flags], filter="cubic")
    assert got.dtype == fmt.dtype and tuple(got.shape) == (len(ks), 3, out_h, out_w)
    bits = tensor_bits(got)
    for j, k in enumerate(ks):
        assert np.array_equal(bits[j], expected_tensor(sources.rule(k, out_w, out_h, flags[j]), fmt))
    if len(ks) < len(SRC_SIZES):                                     # the wrapper knows the sizes: a picture beyond the limit raises
        with pytest.raises(na.NhwError, match="limit"):
            na.resize_to_tensor_device(sources.views, (out_h, out_w), fmt, filter="cubic")


@pytest.mark.gpu
def test_gpu_cubic_long_runs_and_chunks():
    """runs of 128 taps (15 columns a chunk); all 255 through them; a picture exactly at the limit on both axes (129 x 129 taps under a pixel);
    the widest output over a shrinking row axis (ten columns a chunk, 410 chunks); a band of 64 rows whose weights do not fit one chunk of
    rows"""
    cases = [((65535, 1), (2048, 1), None), ((65535, 3), (2048, 1), 255), ((64, 64), (2, 2), None), ((2048, 70), (4096, 3), None), ((3, 1040), (2, 130), None)]
    for j, (size, (out_w, out_h), fill) in enumerate(cases):
        src = Sources([size], 203 + j, fill)
        want = src.rule(0, out_w, out_h)
        if fill is not None:
            assert (want == fill).all()
        for four, flag in ((BYTES, 0), (HALF, 1)):
            fmt = _fmt(*four)
            rc, slots, intact = _launch(src.table, out_w, out_h, fmt, [flag])
            assert rc == 0 and intact and _same(slots[0], src.rule(0, out_w, out_h, flag), fmt), (size, out_w, out_h, fill, fmt)


@pytest.mark.gpu
def test_gpu_cubic_entries_that_store_nothing(sources):
    """an entry one pixel beyond the limit on either axis, a zero side, an oversize side, a zero address and a misaligned one: their slots keep
    the canary, the other entries of the same launch are right"""
    edge = Sources([(65, 1), (64, 1), (2, 33), (2, 32)], 208)
    for four in (BYTES, HALF):
        fmt = _fmt(*four)
        rc, slots, intact = _launch(edge.table, 2, 1, fmt)                       # 65 x 1 -> 2 x 1 and 2 x 33 -> 2 x 1 are beyond it
        assert rc == 0 and intact
        assert (slots[0] == CANARY).all() and (slots[2] == CANARY).all()
        assert _same(slots[1], edge.rule(1, 2, 1), fmt) and _same(slots[3], edge.rule(3, 2, 1), fmt)
    out_w, out_h = 9, 200
    picks = [8, 7, 5, 6, 7, 5, 6, 7]                                 # 300 x 200 -> 9 x 200 is beyond the limit (288), 256 x 255 within it
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
def test_gpu_cubic_many_entries_take_bands_of_64_rows():
    """4096 entries to 3 x 130: with so many a band has the most rows it can have, 64, so an entry is two full bands and one of two rows"""
    n, out_w, out_h = 4096, 3, 130
    src = Sources([(7, 300)] * 5, 209)
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


@pytest.mark.gpu
def test_gpu_resample_entry_filters(sources):
    """filters 0 and 1 are the two older entries, byte for byte; 3 and -1 are refused and nothing is written"""
    import nhwcodec_amd as na
    out_w, out_h = 16, 16
    for four in (BYTES, HALF):
        fmt = _fmt(*four)
        for filter, entry in ((0, "nhw_resize_to_tensor_device"), (1, "nhw_area_to_tensor_device")):
            new = _launch(sources.table, out_w, out_h, fmt, FLAGS, filter=filter)
            old = _launch(sources.table, out_w, out_h, fmt, FLAGS, entry=entry)
            assert new[0] == old[0] == 0 and new[2] and old[2]
            assert all(np.array_equal(a, b) and (a != CANARY).any() for a, b in zip(new[1], old[1])), (fmt, filter)
        for filter in (3, -1):
            rc, slots, intact = _launch(sources.table, out_w, out_h, fmt, FLAGS, filter=filter)
            assert rc == NHW_E_ARG and intact and all((s == CANARY).all() for s in slots) and b"filter" in na._library().nhw_last_error()


# ---------------------------------------------------------------- on the MI355X: the host paths
@pytest.fixture(scope="module")
def world():
    """the crops' pictures (SIZES: 1 x 700, 500 x 375, 1023 x 1025, crops of one seeded scene of generated images) as containers at q20, a
    decoder of 4 tiles a chunk, and the encoder and the scene for the encode test"""
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
def test_gpu_cubic_crops_equal_the_rule_on_decode_windows(world, scale, out_w, out_h, four):
    """40 seeded crops with flips in one call on a decoder of max_batch 4; the statistics are those of the two-tap call; then the crops
    shuffled, into a tensor of the caller's"""
    import torch
    fmt = _fmt(*four)
    rng = np.random.default_rng(2000 + 10 * scale + out_w)
    rects = seeded_windows(scale, 40, rng)
    flips = [bool(v) for v in rng.integers(0, 2, len(rects))]
    assert 8 < sum(flips) < 32 and all(within(r[3:], (out_w, out_h)) for r in rects)
    assert sum(r[3] > out_w or r[4] > out_h for r in rects) >= 5 and sum(r[3] < out_w or r[4] < out_h for r in rects) >= (5 if out_w > 32 else 1)
    wins = world.dec.decode_windows(world.containers, rects, scale)
    world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, flips=flips, scale=scale)
    stats = world.dec.region_stats()
    got, scales = world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, flips=flips, scale=scale, filter="cubic")
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
                                             filter="cubic")
    assert again.data_ptr() == mine.data_ptr() and world.dec.region_stats() == stats
    assert np.array_equal(tensor_bits(again), bits[perm])
    assert np.array_equal(tensor_bits(mine[len(rects) * per:]), before)


@pytest.mark.gpu
def test_gpu_cubic_crops_choose_their_scale_as_before(world):
    """full-resolution crops of the pictures to 64 x 48 with scale=None: the scales and windows are crop_scale's and crop_window's, all three
    scales in one call, and every crop is the rule on its window"""
    import nhwcodec_amd as na
    W, H = SIZES[BIG]
    out_w, out_h = 64, 48
    rng = np.random.default_rng(205)
    crops = [(BIG, 0, 0, W, H), (BIG, W - 256, H - 192, 256, 192), (BIG, W - 255, H - 192, 255, 192), (BIG, 511, 513, 128, 96), (BIG, 300, 1, 127, 96),
             (BIG, W - 31, H - 17, 31, 17), (BIG, 5, 7, 64, 48), (1, 0, 0, 500, 375), (1, 100, 100, 200, 97), (0, 0, 100, 1, 500), (BIG, 0, 300, W, 60)]
    for _ in range(25):
        w, h = int(rng.integers(8, 600)), int(rng.integers(8, 600))
        crops.append((BIG, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    flips = [bool(v) for v in rng.integers(0, 2, len(crops))]
    fmt = _fmt("float32", "CHW", "RGB", "reversed", k=1)
    got, scales = world.dec.decode_crops_device(world.containers, crops, (out_h, out_w), fmt, flips=flips, filter="cubic")
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
        world.dec.decode_crops_device(world.containers, [(1, 0, 0, 10, 10), (0, 0, 0, 1, 700)], (5, 5), fmt, filter="cubic")
    assert world.dec.region_stats() == stats


def _call_crops(dec, containers, rects, scale, out_w, out_h, fmt, flags, addrs, filter, entry="nhw_dec_crops_to_device_resample"):
    """nhw_dec_crops_to_device_resample or nhw_dec_crops_to_device_filter by ctypes -> (rc, status)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    addr = np.array(addrs, np.uint64)
    f = np.array(flags, np.uint8) if flags is not None else None
    c = fmt.c_struct()
    rc = getattr(dec.lib, entry)(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out_w, out_h, ctypes.byref(c),
                                 f.ctypes.data if f is not None else None, addr.ctypes.data, status.ctypes.data, filter)
    return rc, status


@pytest.mark.gpu
def test_gpu_crops_resample_argument(world):
    """filters 0 and 1 are nhw_dec_crops_to_device_filter byte for byte and status for status; with filter 2 a rect beyond the limit is
    NHW_E_ARG, selects no tile and keeps its slot's canary while its neighbours are right; other filters are refused at call level"""
    import torch
    rng = np.random.default_rng(206)
    fmt = _fmt(*HALF)
    out_w, out_h = 32, 24
    per, es = 3 * out_w * out_h, 2
    rects = seeded_windows(2, 12, rng) + [(BIG, 0, 0, 0, 5)]          # the last: an empty rect, NHW_E_ARG for every filter
    flips = [i % 3 == 0 for i in range(len(rects))]
    for filter in (0, 1):
        results = []
        for entry in ("nhw_dec_crops_to_device_filter", "nhw_dec_crops_to_device_resample"):
            buf, at = _guarded(len(rects), per, fmt)
            rc, status = _call_crops(world.dec, world.containers, rects, 2, out_w, out_h, fmt, flips, [buf.data_ptr() + at + i * per * es for i in range(len(rects))], filter, entry)
            torch.cuda.synchronize()
            assert rc == 0 and status.tolist() == [0] * 12 + [NHW_E_ARG]
            results.append((buf.cpu().numpy(), status.tolist(), world.dec.region_stats()))
        assert np.array_equal(results[0][0], results[1][0]) and results[0][1:] == results[1][1:]
        assert results[0][2] == expected_stats(world.containers, rects[:12], 2, unique=True) and (results[0][0][GUARD:-GUARD] != CANARY).any()
    # beyond the limit: 65 columns to 2.  Rect 1 alone selects tile (ty 2, tx 1) of the large picture, which no other rect touches
    out_w, out_h = 2, 2
    per = 3 * out_w * out_h
    rects = [(BIG, 0, 0, 60, 50), (BIG, 600, 1024, 65, 1), (1, 10, 10, 64, 64), (BIG, 0, 0, 65, 5), (1, 0, 0, 5, 65), (BIG, 3, 3, 30, 30)]
    bad = [False, True, False, True, True, False]
    ok = [r for r, b in zip(rects, bad) if not b]
    buf, at = _guarded(len(rects), per, fmt)
    addrs = [buf.data_ptr() + at + i * per * es for i in range(len(rects))]
    rc, status = _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, fmt, None, addrs, CUBIC)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_ARG if b else 0 for b in bad]
    assert world.dec.region_stats() == expected_stats(world.containers, ok, 1, unique=True)
    assert expected_stats(world.containers, ok + rects[1:2], 1, unique=True)[0] == world.dec.region_stats()[0] + 1   # rect 1 would have brought a tile of its own
    host = buf.cpu().numpy()
    wins = iter(world.dec.decode_windows(world.containers, ok, 1))
    for i, b in enumerate(bad):
        got = host[at + i * per * es: at + (i + 1) * per * es]
        if b:
            assert (got == CANARY).all(), rects[i]
        else:
            assert _same(got, rule(next(wins), out_w, out_h), fmt), rects[i]
    assert (host[:at] == CANARY).all() and (host[at + len(rects) * per * es:] == CANARY).all()
    rc, status = _call_crops(world.dec, world.containers, rects, 1, out_w, out_h, fmt, None, addrs, 1)
    assert rc == 0 and not status.any()                              # the area filter's limit is 128
    # an unknown filter
    stats = world.dec.region_stats()
    buf.fill_(CANARY)
    for filter in (3, -1, 256):
        rc, status = _call_crops(world.dec, world.containers, ok, 1, out_w, out_h, fmt, None, addrs[:len(ok)], filter)
        assert rc == NHW_E_ARG and (status == 99).all() and b"filter" in world.dec.lib.nhw_dec_last_error()
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and world.dec.region_stats() == stats


@pytest.mark.gpu
def test_gpu_encode_resized_device_cubic(world):
    """two photos, one of them a crop view of a larger tensor, to one .nhw file each under the cubic rule: the files, sizes and status of
    encode_device on the rule's 512 x 512 pictures; the default is the area filter's call as before"""
    import torch
    import nhwcodec_amd as na
    large = torch.from_numpy(np.ascontiguousarray(world.scene[:1300, :1700])).cuda()
    view = large[211:211 + 1025, 307:307 + 1023]
    assert not view.is_contiguous()
    small = np.ascontiguousarray(world.scene[900:900 + 333, 2000:2000 + 777])
    pictures = [view, torch.from_numpy(small).cuda()]
    ruled = np.stack([rule(p, 512, 512) for p in (view.cpu().numpy(), small)])
    want = world.enc.encode_device(torch.from_numpy(ruled).cuda(), 17)
    got = world.enc.encode_resized_device(pictures, 17, filter="cubic")
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and not bool(got[2].any()) and same_files(got[0], want[0], want[1])
    area = na.resize_to_tensor_device(pictures, (512, 512), na.TensorFormat(*BYTES), filter="area")
    assert not torch.equal(area, torch.from_numpy(ruled).cuda())
    today = world.enc.encode_device(area, 17)
    for again in (world.enc.encode_resized_device(pictures, 17), world.enc.encode_resized_device(pictures, 17, filter="area")):
        assert torch.equal(again[1], today[1]) and torch.equal(again[2], today[2]) and same_files(again[0], today[0], today[1])
    with pytest.raises(na.NhwError, match="'two_tap', 'area', 'cubic'"):
        world.enc.encode_resized_device(pictures, 17, filter="lanczos")


@pytest.mark.gpu
def test_gpu_one_handle_serves_every_filter_in_turn(world):
    rng = np.random.default_rng(207)
    rects = seeded_windows(2, 10, rng)
    fmt = _fmt(*HALF)
    before = world.dec.decode_windows(world.containers, rects, 2)
    got = {f: tensor_bits(world.dec.decode_crops_device(world.containers, rects, (24, 32), fmt, scale=2, filter=f)[0]).copy() for f in ("two_tap", "area", "cubic", "two_tap")}
    after = world.dec.decode_windows(world.containers, rects, 2)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    for i, P in enumerate(before):
        assert np.array_equal(got["cubic"][i], expected_tensor(rule(P, 32, 24), fmt)), rects[i]
    assert not np.array_equal(got["cubic"], got["area"]) and not np.array_equal(got["cubic"], got["two_tap"])
