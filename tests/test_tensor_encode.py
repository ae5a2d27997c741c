"""Encode straight from training tensors: nhw_tensor_to_bytes_device (k_tensor_to_bytes), nhw_enc_batch_device_tensor,
nhw_tile_tensors_device (k_tile_pad_tensor) and their Python faces.

The expected bytes come from the specification (include/nhw_hip.h), computed exactly on the CPU by rule_bytes: t = float64(x) * float64(scale) +
float64(bias); where t is farther than 2^-12 from every k + 0.5 the byte is clip(rint(t), 0, 255) -- the float64 error and the float32 rounding of
the fma are both far below 2^-12 for |t| < 512, and outside that range the clamp decides; every element inside such a zone is recomputed with
fractions.Fraction: the exact product and sum, ONE rounding of the rational to float32 (half-even), then rint (half-even) and the clamp.  No
element is left out of a comparison.  test_rule_helper_on_hand_worked_cases pins the helper itself.

Shapes: a 512 x 512 picture is the codec's unit, so n = 3 is the small batch.  A reference is computed once per element type and shared: layout,
channel order and row direction only permute it."""
import ctypes
import fractions
import math
import os
import re

import numpy as np
import pytest

from oracle.harness import class_image
from tests.support import ROOT, device_arena, golden, load_lib
from tests.tensor_cases import ALL_FORMATS, CONSTANTS, DTYPES, SENTINEL, binade, expected_tensor, round_to_binary

NHW_E_ARG, NHW_E_QUALITY = -4, -1
IMG = 786432
GUARD = 4096
FOUR_FORMATS = [("float32", "CHW", "RGB", "reversed"), ("float16", "HWC", "BGR", "file"), ("bfloat16", "CHW", "BGR", "reversed"), ("uint8", "CHW", "RGB", "reversed")]
FOUR_CONSTANTS = ["imagenet", "unit", "imagenet", None]          # the decode constants whose inverse each of the four encodes under
ROUND_TRIP = [(d, c) for d in ("float32", "float16", "bfloat16") for c in ("imagenet", "unit")]
PICTURE_FORMATS = [("float32", "CHW", "RGB", "reversed"), ("float16", "HWC", "BGR", "file"), ("uint8", "CHW", "RGB", "file")]
PICTURE_SIZES = [(1, 1), (513, 7), (600, 515)]                  # W, H: one pixel; past a tile's width by one, odd; two tile rows and columns, no multiple of 4


# ---------------------------------------------------------------- the specification on the CPU
def _round_to_f32(q):
    """a rational, rounded once to float32 (normal range), half-even -> the rational that float32 holds"""
    if q == 0:
        return q
    assert binade(abs(q)) >= -126
    r = round_to_binary(abs(q), "float32")       # tensor_cases' rounder, which also knows the subnormals and the overflow
    assert r != math.inf
    return r if q > 0 else -r


def _exact_byte(x, scale, bias):
    y = _round_to_f32(fractions.Fraction(float(x)) * fractions.Fraction(float(scale)) + fractions.Fraction(float(bias)))
    return min(255, max(0, round(y)))            # round(Fraction): half-even


def rule_bytes(x, scale, bias, count=None):
    """x: float64 [..., 3], the elements widened exactly, tensor channel last; scale, bias: the format's float32 constants by tensor channel
    -> the byte of every element, uint8 [..., 3].  count: a list that receives the number of elements that took the exact route"""
    sc, bi = np.array(scale, np.float32).astype(np.float64), np.array(bias, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = x * sc + bi
        out = np.clip(np.rint(np.where(np.isnan(t), 0.0, t)), 0, 255).astype(np.uint8)
        zone = np.isfinite(t) & (t > -1) & (t < 257) & (np.abs(t - (np.floor(t) + 0.5)) <= 2.0 ** -12)
    idx = np.argwhere(zone)
    memo = {}
    for i in idx:
        i = tuple(i)
        key = (float(x[i]), i[-1])
        if key not in memo:
            memo[key] = _exact_byte(x[i], sc[i[-1]], bi[i[-1]])
        out[i] = memo[key]
    if count is not None:
        count.append(len(idx))
    return out


def widen(bits, dtype):
    """bit patterns (unsigned integers of the element's size) -> the values, exactly, as float64"""
    if dtype == "uint8":
        return bits.astype(np.float64)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float32).astype(np.float64)


def byte_picture(t, fmt):
    """t: the bytes by tensor channel, [..., H, W, 3] in tensor row order -> the byte path's picture(s): B, G, R a pixel, rows in file order"""
    if fmt.channels == "RGB":
        t = t[..., ::-1]
    if fmt.rows == "reversed":
        t = t[..., ::-1, :, :]
    return np.ascontiguousarray(t)


def expected_bytes(bits_hwc, fmt, count=None):
    """bits_hwc: bit patterns [..., H, W, 3], tensor channel last, tensor row order"""
    t = bits_hwc if fmt.dtype_name == "uint8" else rule_bytes(widen(bits_hwc, fmt.dtype_name), fmt.scale, fmt.bias, count)
    return byte_picture(t, fmt)


NP_BITS = {"uint8": np.uint8, "float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}


def to_bits(values32, dtype):
    """float32 values rounded to the element type (uint8: truncated integers) -> its bit patterns"""
    import torch
    if dtype == "uint8":
        return values32.astype(np.uint8)
    if dtype == "float32":
        return np.ascontiguousarray(values32, np.float32).view(np.uint32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return values32.astype(np.float16).view(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(values32, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def to_device(bits, dtype):
    """bit patterns -> a CUDA tensor of the element type with those bits"""
    import torch
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}[bits.dtype]
    return torch.from_numpy(np.array(bits, order="C").view(signed)).cuda().view(getattr(torch, dtype))


def in_layout(bits_hwc, fmt):
    """[..., H, W, 3] -> the tensor's own layout"""
    return np.ascontiguousarray(np.moveaxis(bits_hwc, -1, -3)) if fmt.layout == "CHW" else bits_hwc


RANDOM_SCALE, RANDOM_BIAS = (255.0, 270.0, 240.0), (0.0, -10.0, 5.0)     # on x in -0.15 .. 1.25: about -40 .. 300 and more, so both clamps fire
_RANDOM = {}


def random_batch(dtype):
    """three pictures of random elements, [3, 512, 512, 3] bit patterns, and the bytes by tensor channel the rule makes of them under the
    RANDOM constants; computed once per type, never written to"""
    if dtype not in _RANDOM:
        rng = np.random.default_rng(1234 + DTYPES.index(dtype))
        if dtype == "uint8":
            bits = rng.integers(0, 256, (3, 512, 512, 3), dtype=np.uint8)
            t = bits
        else:
            bits = to_bits((rng.random((3, 512, 512, 3), dtype=np.float32) * np.float32(1.4) - np.float32(0.15)), dtype)
            t = rule_bytes(widen(bits, dtype), RANDOM_SCALE, RANDOM_BIAS)
            assert (t == 0).mean() > 0.02 and (t == 255).mean() > 0.02
        bits.setflags(write=False)
        t.setflags(write=False)
        _RANDOM[dtype] = (bits, t)
    return _RANDOM[dtype]


def _format(dtype, layout, channels, rows, **kw):
    import nhwcodec_amd as na
    return na.TensorFormat(dtype, layout, channels, rows, **({} if dtype == "uint8" else kw))


def _random_format(four):
    return _format(*four, scale=RANDOM_SCALE, bias=RANDOM_BIAS)


# ---------------------------------------------------------------- without a GPU
def test_rule_helper_on_hand_worked_cases():
    one = lambda x, s=1.0, b=0.0: int(rule_bytes(np.full((1, 3), float(x)), (s,) * 3, (b,) * 3)[0, 0])
    assert [one(v) for v in (0.5, 1.5, 2.5, 3.5, 254.5, 255.5, 255.49, 255.51, 256.0, 1e30)] == [0, 2, 2, 4, 254, 255, 255, 255, 255, 255]
    assert [one(v) for v in (-0.5, -0.0, 0.0, -1e30, 0.4999, 0.5001, float("inf"), float("-inf"), float("nan"), -float("nan"))] == [0, 0, 0, 0, 0, 1, 255, 0, 0, 0]
    assert one(0.0, 0.0, 254.5) == 254 and one(float("inf"), 0.0, 7.0) == 0 and one(2.0 ** -24, 2.0 ** 25) == 2 and one(2.0 ** -127, 2.0 ** 127) == 1
    # one rounding, not two: 2 * 1 + (0.5 + 2^-24) -- the exact sum 2.5 + 2^-24 lies above the tie, float32 holds 2.5: the
    # fma gives the float 2.5 and rint(2.5) = 2, where rint of the exact sum would be 3
    x, b = float(np.float32(2.0)), float(np.float32(0.5 + 2.0 ** -24))
    assert b != 0.5 and one(x, 1.0, b) == 2
    # ... and the other way: the exact sum lies below a tie the float32 rounding reaches
    assert one(float(np.float32(1.0 - 2.0 ** -24)), 1.0, 0.5) == 2 and float(np.float32(1.5 - 2.0 ** -24)) == 1.5
    # _round_to_f32 itself: ties to even at 24 bits
    f = fractions.Fraction
    assert _round_to_f32(f(2 ** 24 + 1)) == 2 ** 24 and _round_to_f32(f(2 ** 24 + 3)) == 2 ** 24 + 4 and _round_to_f32(f(3, 2)) == f(3, 2)
    assert _round_to_f32(f(1, 3)) == f(float(np.float32(1 / 3)))
    count = []
    rule_bytes(np.array([[0.5, 0.25, 1.5 + 2.0 ** -13]]), (1.0,) * 3, (0.0,) * 3, count)
    assert count == [2]
    assert np.array_equal(widen(np.array([0x3C00, 0x0001, 0xFBFF], np.uint16), "float16"), [1.0, 2.0 ** -24, -65504.0])
    assert np.array_equal(widen(np.array([0x3F80, 0x0001, 0xC000], np.uint16), "bfloat16"), [1.0, 2.0 ** -133, -2.0])


def test_header_declares_the_entry_points_and_the_picture_struct():
    import nhwcodec_amd as na
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "nhw_hip.h")).read())
    assert "int nhw_tensor_to_bytes_device(const void *d_in, int n, const nhw_tensor_format *fmt, void *d_bgr, void *stream);" in hdr
    assert ("int nhw_enc_batch_device_tensor(nhw_enc *e, const void *d_in, int n, const nhw_tensor_format *fmt, int quality, void *d_out, "
            "int32_t *d_sizes, int32_t *d_status, void *stream);") in hdr
    assert ("int nhw_tile_tensors_device(const nhw_tensor_picture *d_pics, int n_pics, int tile0, int m, const nhw_tensor_format *fmt, "
            "void *d_tiles, void *stream);") in hdr
    assert "typedef struct { uint64_t addr, pitch, plane; uint32_t width, height, first_tile, reserved; } nhw_tensor_picture;" in hdr
    assert np.dtype(na.TENSOR_PICTURE_DTYPE).itemsize == 40
    assert [n for n, _ in na.TENSOR_PICTURE_DTYPE] == ["addr", "pitch", "plane", "width", "height", "first_tile", "reserved"]
    lib = load_lib()
    for name in ("nhw_tensor_to_bytes_device", "nhw_enc_batch_device_tensor", "nhw_tile_tensors_device"):
        assert hasattr(lib, name), name


def test_inverted_arithmetic_and_refusals():
    import nhwcodec_amd as na
    f = na.TensorFormat("float16", "HWC", "BGR", "file", **CONSTANTS["imagenet"])
    g = f.inverted()
    assert (g.dtype_name, g.layout, g.channels, g.rows) == ("float16", "HWC", "BGR", "file")
    for c in range(3):
        s, b = np.float32(f.scale[c]), np.float32(f.bias[c])
        assert np.float32(g.scale[c]) == np.float32(1) / s and np.float32(g.bias[c]) == -b / s
        assert g.scale[c] == float(np.float32(g.scale[c])) and g.bias[c] == float(np.float32(g.bias[c]))
    h = na.TensorFormat("float32", scale=(0.5, 4, -2), bias=(1, 0, 3)).inverted()
    assert h.scale == (2.0, 0.25, -0.5) and h.bias == (-2.0, 0.0, 1.5)
    u = na.TensorFormat("uint8", "CHW", "RGB", "file").inverted()
    assert u.scale == (1.0,) * 3 and u.bias == (0.0,) * 3 and u.dtype_name == "uint8"
    for kw in (dict(scale=0), dict(scale=(1, 0, 1)), dict(scale=1e-39), dict(scale=(1, 1, 1e-30), bias=(0, 0, 1e30))):
        with pytest.raises(na.NhwError):
            na.TensorFormat("float32", **kw).inverted()


@pytest.mark.parametrize("dtype,constants", ROUND_TRIP)
def test_round_trip_condition(dtype, constants):
    """what the GPU round-trip test rests on: for every byte b and channel, the element a decode under fmt stores for b, encoded under
    fmt.inverted(), is b again: rint(fma(decode(b), scale', bias')) == b, the unrounded value within 0.5 of b"""
    import nhwcodec_amd as na
    fmt = na.TensorFormat(dtype, "HWC", "BGR", "file", **CONSTANTS[constants])
    inv = fmt.inverted()
    px = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1).reshape(1, 256, 3)
    elems = widen(expected_tensor(px, fmt), dtype)                        # [1, 256, 3] float64: what the decoder stores
    assert np.array_equal(rule_bytes(elems, inv.scale, inv.bias), px)
    err = np.abs(elems * np.array(inv.scale) + np.array(inv.bias) - px)
    assert err.max() < 0.5, err.max()


def test_python_argument_errors_without_a_device():
    import torch
    import nhwcodec_amd as na
    fmt = na.TensorFormat("float32", "CHW", "RGB", "reversed")
    x = torch.zeros((1, 3, 512, 512), dtype=torch.float32)
    for call in (lambda: na.tensor_to_bytes_device(x, "float32"), lambda: na.tensor_to_bytes_device(x, None),       # fmt is no TensorFormat
                 lambda: na.tensor_to_bytes_device(x, fmt),                                                             # the batch is on the CPU
                 lambda: na.tensor_to_bytes_device(x.to(torch.float16), fmt),                                           # the wrong dtype
                 lambda: na.tensor_to_bytes_device(x.permute(0, 2, 3, 1), fmt), lambda: na.tensor_to_bytes_device(x[0], fmt),   # the wrong shape
                 lambda: na.tensor_to_bytes_device(x.numpy(), fmt),
                 lambda: na.tile_tensors_device([], fmt), lambda: na.tile_tensors_device(x[0], fmt), lambda: na.tile_tensors_device([x[0]], fmt),
                 lambda: na.tile_tensors_device([x[0]], "CHW")):
        with pytest.raises(na.NhwError):
            call()


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _guarded(nbytes):
    """a 16-byte aligned view of nbytes between two sentinel-filled guards -> (the whole buffer, the view)"""
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + nbytes:] == SENTINEL).all())


def _to_bytes_guarded(lib, x, fmt):
    """nhw_tensor_to_bytes_device into a guarded buffer -> uint8 [n, 512, 512, 3] on the host"""
    import torch
    n = x.shape[0]
    buf, out = _guarded(n * IMG)
    c = fmt.c_struct()
    assert lib.nhw_tensor_to_bytes_device(x.data_ptr(), n, ctypes.byref(c), out.data_ptr(), None) == 0, lib.nhw_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(buf, n * IMG), f"{fmt}: bytes outside n * 786432 were written"
    return out.cpu().numpy().reshape(n, 512, 512, 3)


def _differ(got, want, what):
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} bytes differ, first at {tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {want[bad][0]}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout,channels,rows", ALL_FORMATS)
def test_gpu_every_format(lib, dtype, layout, channels, rows):
    """all 32 formats on three pictures of random elements that reach about -40 .. 300 behind the affine, byte for byte, between guards"""
    import torch
    import nhwcodec_amd as na
    fmt = _random_format((dtype, layout, channels, rows))
    bits, t = random_batch(dtype)
    x = to_device(in_layout(bits, fmt), dtype)
    assert tuple(x.shape) == (3,) + fmt.shape(512, 512)
    got = _to_bytes_guarded(lib, x, fmt)
    _differ(got, byte_picture(t, fmt), f"{fmt}")
    py = na.tensor_to_bytes_device(x, fmt)
    torch.cuda.synchronize()
    assert py.dtype == torch.uint8 and tuple(py.shape) == (3, 512, 512, 3) and np.array_equal(py.cpu().numpy(), got)


def _special_picture(dtype):
    """float32 values [512, 512, 3], tensor channel last, that `dtype` holds exactly, and the hand-worked bytes at some of their places, for the
    constants scale = (256, 1, 2^25 or 2^127), bias = 0.  Channel 0: the ties (k + 0.5) / 256; channel 1: the ties k + 0.5 and the special values;
    channel 2: the smallest denormals"""
    import torch
    t = getattr(torch, dtype)
    fin = float(torch.finfo(t).max)
    holds = lambda v: np.array_equal(widen(to_bits(np.array([v], np.float32), dtype), dtype), np.array([v], np.float64))
    x = np.zeros((512, 512, 3), np.float32)
    hand = {}                                                            # (row, column, channel) -> byte
    for k in range(256):
        tie = min(255, k + (k & 1))                                      # k + 0.5 to the even neighbour; 255.5 clamps
        if holds((k + 0.5) / 256):
            x[0, k, 0] = (k + 0.5) / 256
            hand[(0, k, 0)] = tie
        if holds(k + 0.5):
            x[0, k, 1] = k + 0.5
            hand[(0, k, 1)] = tie
    for k, want in ((0, 0), (1, 2), (2, 2)) + (((254, 254), (255, 255)) if dtype != "bfloat16" else ()):
        assert hand[(0, k, 1)] == want and hand[(0, k, 0)] == want       # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254, 255.5 -> 255
    eps = float(torch.finfo(t).eps)
    below, above = 255.5 * (1 - eps), 255.5 * (1 + eps)                  # 255.49.. and 255.51.. to the type's precision (rounded to it below)
    specials = [(-0.5, 0), (-0.0, 0), (float("nan"), 0), (-float("nan"), 0), (float("inf"), 255), (float("-inf"), 0), (fin, 255), (-fin, 0),
                (below, 255 if dtype != "bfloat16" else None), (above, 255 if dtype != "bfloat16" else None),    # (bfloat16 holds neither 255.5 nor a neighbour of it)
                (254.5 * (1 + eps), 255 if dtype != "bfloat16" else None), (0.5 * (1 + eps), 1), (0.5 * (1 - eps), 0)]
    for j, (v, want) in enumerate(specials):
        x[1, j, 1] = v
        if want is not None:
            hand[(1, j, 1)] = want
    if dtype == "float16":
        x[2, 0, 2] = 2.0 ** -24                                          # the smallest float16 denormal, times 2^25
        hand[(2, 0, 2)] = 2
        big = 2.0 ** 25
    else:
        x[2, 0, 2] = 2.0 ** -127                                         # a float32 (and bfloat16) denormal, times 2^127
        hand[(2, 0, 2)] = 1
        big = 2.0 ** 127
    x[3:, :, :] = np.random.default_rng(5).random((509, 512, 3), dtype=np.float32) * (1, 300, 0) - (0, 20, 0)
    return x, hand, (256.0, 1.0, big)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_gpu_special_values(lib, dtype, layout):
    """exact ties (power-of-two constants: the arithmetic is exact), signed zeros, NaNs, infinities, the largest finite values, denormals, and
    a bias alone behind scale 0"""
    import torch
    x32, hand, scale = _special_picture(dtype)
    bits = to_bits(x32, dtype)
    top = 8 * bits.itemsize - 1                                          # -0.0 and the NaNs of both signs as bit patterns: a cast may not keep a sign
    quiet = {"float16": 0x7E00, "bfloat16": 0x7FC0, "float32": 0x7FC00000}[dtype]
    bits[1, 1, 1], bits[1, 2, 1], bits[1, 3, 1] = 1 << top, quiet, quiet | 1 << top
    assert np.isnan(widen(bits[1, 2:4, 1], dtype)).all() and np.signbit(widen(bits[1, 1:4, 1], dtype)).tolist() == [True, False, True]
    fmt = _format(dtype, layout, "BGR", "file", scale=scale, bias=0)
    want = expected_bytes(bits[None], fmt)
    for (r, c, ch), b in hand.items():
        assert want[0, r, c, ch] == b, (r, c, ch, x32[r, c, ch])         # the reference agrees with the hand-worked values ...
    got = _to_bytes_guarded(lib, to_device(in_layout(bits[None], fmt), dtype), fmt)
    for (r, c, ch), b in hand.items():
        assert got[0, r, c, ch] == b, (r, c, ch, x32[r, c, ch], int(got[0, r, c, ch]))
    _differ(got, want, f"{fmt}")                                         # ... and the kernel with the reference, everywhere
    # a bias alone: x = 0 and scale = 0 (and, elsewhere in the picture, x finite: 0 * x + bias)
    fmt0 = _format(dtype, layout, "RGB", "reversed", scale=0, bias=(0.5, 7.0, 254.5))
    zero = np.zeros((1, 512, 512, 3), NP_BITS[dtype])
    got0 = _to_bytes_guarded(lib, to_device(in_layout(zero, fmt0), dtype), fmt0)
    assert (got0[..., 2] == 0).all() and (got0[..., 1] == 7).all() and (got0[..., 0] == 254).all()      # RGB: tensor channel 0 is byte 2


def _encode(enc, call, *a):
    """-> (files or None where the status is not 0, sizes, status) on the host"""
    import torch
    out, sizes, status = call(*a)
    torch.cuda.synchronize()
    sizes, status = sizes.cpu().numpy(), status.cpu().numpy()
    return [out[i, :int(sizes[i])].cpu().numpy().tobytes() if status[i] == 0 else None for i in range(len(sizes))], sizes.tolist(), status.tolist()


@pytest.fixture(scope="module")
def enc():
    import nhwcodec_amd as na
    e = na.Encoder(0, max_batch=3, device_only=True)
    yield e
    e.close()


def _class_pictures():
    px = np.stack([class_image("blocks", 1), class_image("gradient", 2), class_image("tiles", 3)])
    px[1, :256, :, 0] = 255                                              # ... with saturated and black stretches in one of them
    px[1, 256:, :, 2] = 0
    return px


def _decoded_form(px, fmt):
    """what a decode under fmt stores for the byte pictures px [n, 512, 512, 3]: bit patterns in fmt's layout (tests/tensor_cases.py)"""
    return np.stack([expected_tensor(p, fmt) for p in px])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(4))
def test_gpu_encode_is_the_byte_encode(enc, oracle, k):
    """encode_tensor_device equals encode_device of the expected bytes: sizes, status and files, at q20 (fused front), q23 (plain front) and q10
    (the low path); at q20 the files are the oracle encoder's of those bytes"""
    import torch
    import nhwcodec_amd as na
    four, constants = FOUR_FORMATS[k], FOUR_CONSTANTS[k]
    px = _class_pictures()
    dec_fmt = _format(*four, **(CONSTANTS[constants] if constants else {}))
    fmt = dec_fmt.inverted()
    bits = _decoded_form(px, dec_fmt)                                    # the tensor a decode of these pictures would have stored
    hwc = np.moveaxis(bits, 1, -1) if fmt.layout == "CHW" else bits
    want_px = expected_bytes(hwc, fmt)
    assert np.array_equal(want_px, px)                                   # (the round-trip condition, on these pictures)
    x = to_device(bits, fmt.dtype_name)
    d_px = torch.from_numpy(want_px).cuda()
    for q in (20, 23, 10):
        got = _encode(enc, enc.encode_tensor_device, x, fmt, q)
        want = _encode(enc, enc.encode_device, d_px, q)
        assert got == want, (fmt, q, got[1:], want[1:])
        assert want[2] == [0, 0, 0]
        if q == 20:
            for i in range(3):
                assert got[0][i] == oracle.encode(want_px[i], 20), (fmt, i)


@pytest.mark.gpu
def test_gpu_byte_format_is_encode_device(enc):
    import torch
    import nhwcodec_amd as na
    d_px = torch.from_numpy(_class_pictures()).cuda()
    fmt = na.TensorFormat("uint8", "HWC", "BGR", "file")
    assert _encode(enc, enc.encode_tensor_device, d_px, fmt, 20) == _encode(enc, enc.encode_device, d_px, 20)
    assert np.array_equal(na.tensor_to_bytes_device(d_px, fmt).cpu().numpy(), d_px.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,constants", ROUND_TRIP)
def test_gpu_round_trip(enc, dtype, constants):
    """decode_tensor_device(fmt) of three committed files, then encode_tensor_device(fmt.inverted()): the files of decode_device + encode_device"""
    import torch
    import nhwcodec_amd as na
    files = [golden("q20_0.nhw"), golden("q10_0.nhw"), golden("q23_0.nhw")]
    fmt = na.TensorFormat(dtype, "CHW", "RGB", "reversed", **CONSTANTS[constants])
    dec = na.Decoder(0, max_batch=3)
    try:
        t, st, _ = dec.decode_tensor_device(*device_arena(files), fmt)
        px, st2, _ = dec.decode_device(*device_arena(files))
        torch.cuda.synchronize()
        assert not bool(st.any()) and not bool(st2.any())
        got = _encode(enc, enc.encode_tensor_device, t, fmt.inverted(), 20)
        want = _encode(enc, enc.encode_device, px.contiguous(), 20)
    finally:
        dec.close()
    assert got == want and all(f is not None for f in want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("device_only", [True, False])
def test_gpu_one_handle_bytes_and_tensors_in_any_order(device_only):
    """bytes, tensor, bytes, another tensor format on ONE handle (the first tensor call allocates the scratch), on torch's default stream and on
    another; n = max_batch works, n = max_batch + 1 is refused"""
    import torch
    import nhwcodec_amd as na
    px = _class_pictures()
    d_px = torch.from_numpy(px).cuda()
    f32 = na.TensorFormat("float32", "CHW", "RGB", "reversed", **CONSTANTS["imagenet"])
    f16 = na.TensorFormat("float16", "HWC", "BGR", "file", **CONSTANTS["unit"])
    tensors = {f: to_device(_decoded_form(px, f), f.dtype_name) for f in (f32, f16)}
    fresh = na.Encoder(0, max_batch=3, device_only=True)
    want = {q: _encode(fresh, fresh.encode_device, d_px, q) for q in (20, 12)}
    want2 = _encode(fresh, fresh.encode_device, d_px[:2], 20)
    fresh.close()
    e = na.Encoder(0, max_batch=3, device_only=device_only)
    try:
        for stream in (None, torch.cuda.Stream()):
            with torch.cuda.stream(stream):
                assert _encode(e, e.encode_device, d_px, 20) == want[20]
                assert _encode(e, e.encode_tensor_device, tensors[f32], f32.inverted(), 12) == want[12]      # n = max_batch
                assert _encode(e, e.encode_device, d_px, 12) == want[12]
                assert _encode(e, e.encode_tensor_device, tensors[f16][:2], f16.inverted(), 20) == want2
                if not device_only:
                    assert e.encode(px[:2], 20) == want2[0]                                                  # the host path, whose staging the scratch is not
                assert _encode(e, e.encode_tensor_device, tensors[f32], f32.inverted(), 20) == want[20]
        four = torch.cat([tensors[f32], tensors[f32][:1]])
        with pytest.raises(na.NhwError, match="max_batch"):
            e.encode_tensor_device(four, f32.inverted())
        out, sizes, status = e.alloc_out(4)
        c = f32.inverted().c_struct()
        assert e.lib.nhw_enc_batch_device_tensor(e.h, four.data_ptr(), 4, ctypes.byref(c), 20, out.data_ptr(), sizes.data_ptr(), status.data_ptr(), None) == NHW_E_ARG
        assert _encode(e, e.encode_device, d_px, 20) == want[20]
    finally:
        e.close()


# ---------------------------------------------------------------- pictures of any size
def _picture_sources(fmt, fill_seed):
    """the three pictures as views of one device buffer of fmt's element type -> (views, their bit patterns [H, W, 3] tensor channel last, in
    tensor row order).  The pictures' own elements depend on fmt only; everything else in the buffer on fill_seed (NaNs included).  CHW: crop
    views x[:, y0:y1, x0:x1] of larger tensors that start at an odd element offset, x0 odd; HWC: rows with a padded pitch, odd in elements"""
    import torch
    dtype = fmt.dtype_name
    rng = np.random.default_rng(99)
    own = []
    for w, h in PICTURE_SIZES:
        if dtype == "uint8":
            own.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        else:
            own.append(to_bits(rng.random((h, w, 3), dtype=np.float32) * np.float32(1.4) - np.float32(0.15), dtype))
    frng = np.random.default_rng(fill_seed)
    total = 3 << 20
    if dtype == "uint8":
        host = frng.integers(0, 256, total, dtype=np.uint8)
    else:
        fill = frng.random(total, dtype=np.float32) * np.float32(4) - np.float32(2)
        fill[frng.random(total) < 0.25] = np.nan
        host = to_bits(fill, dtype)
    at, places = 1, []                                                   # (offset, strides) in elements
    for (w, h), bits in zip(PICTURE_SIZES, own):
        if fmt.layout == "CHW":
            big_w, big_h = w + 11, h + 5
            off = at + 1 + 2 * big_w + 3                                 # row 2, column 3 of a [3, big_h, big_w] tensor at the even offset at + 1
            strides = (big_h * big_w, big_w, 1)
            for c in range(3):
                for r in range(h):
                    host[off + c * strides[0] + r * big_w: off + c * strides[0] + r * big_w + w] = bits[r, :, c]
            at = (at + 1 + 3 * big_h * big_w + 8) | 1
        else:
            pitch = 3 * w + 7 + 2 * len(places)                          # odd
            off, strides = at, (pitch, 3, 1)
            for r in range(h):
                host[off + r * pitch: off + r * pitch + 3 * w] = bits[r].reshape(-1)
            at = (at + h * pitch + 8) | 1
        assert off % 2 == 1
        places.append((off, strides))
    assert at <= total
    buf = to_device(host, dtype)
    views = [buf.as_strided((3, h, w) if fmt.layout == "CHW" else (h, w, 3), st, off) for (off, st), (w, h) in zip(places, PICTURE_SIZES)]
    return views, own


def _tiles_of(px):
    """the numpy reference of the padding rule: a byte picture [H, W, 3] -> its tiles [T, 512, 512, 3]"""
    h, w = px.shape[:2]
    ny, nx = -(-h // 512), -(-w // 512)
    p = np.pad(px, ((0, 512 * ny - h), (0, 512 * nx - w), (0, 0)), mode="edge")
    return p.reshape(ny, 512, nx, 512, 3).transpose(0, 2, 1, 3, 4).reshape(ny * nx, 512, 512, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout,channels,rows", PICTURE_FORMATS)
def test_gpu_tile_tensors(lib, dtype, layout, channels, rows):
    """1 x 1, 513 x 7 and 600 x 515 as crop views (CHW) or with padded pitches (HWC): the tiles are tile_pictures_device's of the expected byte
    pictures and numpy's edge padding of them; what is not picture in the source buffers plays no part; the tile buffer's guards stay"""
    import torch
    import nhwcodec_amd as na
    fmt = _random_format((dtype, layout, channels, rows))
    views, own = _picture_sources(fmt, 1)
    other, own2 = _picture_sources(fmt, 2)
    assert all(np.array_equal(a, b) for a, b in zip(own, own2))
    want_px = [expected_bytes(b, fmt) for b in own]
    want = np.concatenate([_tiles_of(p) for p in want_px])
    assert len(want) == 1 + 2 + 4

    def run(v):
        table, tiles, _ = na._tensor_picture_table(v, fmt, "test")
        assert tiles == len(want)
        buf, out = _guarded(tiles * IMG)
        c = fmt.c_struct()
        assert lib.nhw_tile_tensors_device(table.data_ptr(), len(v), 0, tiles, ctypes.byref(c), out.data_ptr(), None) == 0, lib.nhw_last_error()
        torch.cuda.synchronize()
        assert _guards_intact(buf, tiles * IMG)
        return out.cpu().numpy().reshape(tiles, 512, 512, 3)

    got = run(views)
    _differ(got, want, f"{fmt}")
    byte_tiles = na.tile_pictures_device([torch.from_numpy(p).cuda() for p in want_px])
    py = na.tile_tensors_device(views, fmt)
    torch.cuda.synchronize()
    assert np.array_equal(byte_tiles.cpu().numpy(), got) and np.array_equal(py.cpu().numpy(), got)
    _differ(run(other), want, f"{fmt}, the other filling")
    # a range of tiles in the middle (tile0, m), and bad entries passed over: their tiles stay as they were
    table, tiles, _ = na._tensor_picture_table(views, fmt, "test")
    c = fmt.c_struct()
    buf, out = _guarded(3 * IMG)
    assert lib.nhw_tile_tensors_device(table.data_ptr(), 3, 2, 3, ctypes.byref(c), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert _guards_intact(buf, 3 * IMG) and np.array_equal(out.cpu().numpy().reshape(3, 512, 512, 3), want[2:5])
    bad = table.cpu().numpy().view(np.dtype(na.TENSOR_PICTURE_DTYPE)).copy()
    bad[0]["width"] = 0
    bad[1]["height"] = 65536
    if fmt.dtype.itemsize > 1:
        bad[2]["pitch"] += 1
    d_bad = torch.from_numpy(bad.view(np.int64).copy()).cuda()
    buf, out = _guarded(7 * IMG)
    assert lib.nhw_tile_tensors_device(d_bad.data_ptr(), 3, 0, 7, ctypes.byref(c), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    res = out.cpu().numpy().reshape(7, 512, 512, 3)
    assert (res[:3] == SENTINEL).all() and _guards_intact(buf, 7 * IMG)
    if fmt.dtype.itemsize > 1:
        assert (res[3:] == SENTINEL).all()
    else:
        assert np.array_equal(res[3:], want[3:])


@pytest.mark.gpu
def test_gpu_tiles_feed_the_encoder(enc):
    """tile_tensors_device -> encode_device: the files of the byte pictures' tiles"""
    import torch
    import nhwcodec_amd as na
    fmt = na.TensorFormat("float32", "CHW", "RGB", "reversed", **CONSTANTS["unit"])
    px = np.ascontiguousarray(class_image("blocks", 4)[:300, :400])
    x = to_device(expected_tensor(px, fmt), "float32")
    tiles = na.tile_tensors_device([x], fmt.inverted())
    want = na.tile_pictures_device([torch.from_numpy(px).cuda()])
    torch.cuda.synchronize()
    assert torch.equal(tiles, want)
    assert _encode(enc, enc.encode_device, tiles, 20) == _encode(enc, enc.encode_device, want, 20)


# ---------------------------------------------------------------- refusals
def _c_format(base=("float32", "CHW", "RGB", "reversed"), **kw):
    import nhwcodec_amd as na
    c = na.TensorFormat(*base).c_struct()
    for k, v in kw.items():
        if k in ("scale", "bias"):
            getattr(c, k)[1] = v
        else:
            setattr(c, k, v)
    return c


REFUSED_FORMATS = [dict(scale=float("inf")), dict(scale=float("nan")), dict(bias=float("-inf")), dict(bias=float("nan")),
                   dict(dtype=4), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(channels=2), dict(channels=-1), dict(rows=2), dict(rows=-1),
                   dict(reserved=1), dict(dtype=0, scale=2.0), dict(dtype=0, bias=1.0)]


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(enc):
    """every NHW_E_ARG case of the three entry points returns before any launch: files, sizes, status, bytes and tiles stay at their sentinels, and
    the handle encodes bytes as before"""
    import torch
    import nhwcodec_amd as na
    lib = enc.lib
    px = _class_pictures()
    d_px = torch.from_numpy(px).cuda()
    before = _encode(enc, enc.encode_device, d_px, 20)
    x = torch.zeros((3 * 3 * 512 * 512 + 8,), dtype=torch.float32, device="cuda")
    out = torch.full((3 * (512 << 10),), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    status = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bgr = torch.full((3 * IMG + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    views, _ = _picture_sources(_random_format(PICTURE_FORMATS[0]), 3)
    table, tiles, _ = na._tensor_picture_table(views, _random_format(PICTURE_FORMATS[0]), "test")
    assert x.data_ptr() % 16 == 0 and bgr.data_ptr() % 16 == 0

    def enc_call(c, shift=0, n=3, q=20, h=enc.h, o=out, s=sizes, t=status):
        return lib.nhw_enc_batch_device_tensor(h, x.data_ptr() + shift, n, ctypes.byref(c) if c is not None else None, q,
                                               o.data_ptr() if o is not None else None, s.data_ptr() if s is not None else None, t.data_ptr() if t is not None else None, None)

    def bytes_call(c, shift=0, oshift=0, n=3):
        return lib.nhw_tensor_to_bytes_device(x.data_ptr() + shift, n, ctypes.byref(c) if c is not None else None, bgr.data_ptr() + oshift, None)

    def tile_call(c, n_pics=3, tile0=0, m=3, oshift=0, t=table):
        return lib.nhw_tile_tensors_device(t.data_ptr() if t is not None else None, n_pics, tile0, m, ctypes.byref(c) if c is not None else None, bgr.data_ptr() + oshift, None)

    def untouched():
        torch.cuda.synchronize()
        return (bool((out == SENTINEL).all()) and bool((sizes == 0x5A5A5A5A).all()) and bool((status == 0x5A5A5A5A).all()) and bool((bgr == SENTINEL).all()))

    good = _c_format()
    byte_format = _c_format(base=("uint8", "HWC", "BGR", "file"))
    for kw in REFUSED_FORMATS:
        c = _c_format(**kw)
        assert enc_call(c) == NHW_E_ARG and bytes_call(c) == NHW_E_ARG and tile_call(c) == NHW_E_ARG, kw
        assert lib.nhw_last_error()
    assert enc_call(None) == NHW_E_ARG and bytes_call(None) == NHW_E_ARG and tile_call(None) == NHW_E_ARG
    for shift in (1, 2, 4, 8):                                          # a misaligned batch pointer, the byte format too
        assert enc_call(good, shift=shift) == NHW_E_ARG and enc_call(byte_format, shift=shift) == NHW_E_ARG, shift
        assert bytes_call(good, shift=shift) == NHW_E_ARG and bytes_call(good, oshift=shift) == NHW_E_ARG and tile_call(good, oshift=shift) == NHW_E_ARG, shift
    for n in (0, -1, 4):                                                # n outside 1 .. max_batch
        assert enc_call(good, n=n) == NHW_E_ARG and enc_call(byte_format, n=n) == NHW_E_ARG, n
    assert bytes_call(good, n=0) == NHW_E_ARG and bytes_call(good, n=-1) == NHW_E_ARG and bytes_call(good, n=(1 << 22) + 1) == NHW_E_ARG
    assert lib.nhw_tensor_to_bytes_device(None, 3, ctypes.byref(good), bgr.data_ptr(), None) == NHW_E_ARG
    assert lib.nhw_tensor_to_bytes_device(x.data_ptr(), 3, ctypes.byref(good), None, None) == NHW_E_ARG
    # what nhw_enc_batch_device and nhw_tile_pictures_device refuse for the shared arguments
    assert enc_call(good, h=None) == NHW_E_ARG and enc_call(good, o=None) == NHW_E_ARG and enc_call(good, s=None) == NHW_E_ARG and enc_call(good, t=None) == NHW_E_ARG
    assert lib.nhw_enc_batch_device_tensor(enc.h, None, 3, ctypes.byref(good), 20, out.data_ptr(), sizes.data_ptr(), status.data_ptr(), None) == NHW_E_ARG
    assert enc_call(good, q=0) == NHW_E_QUALITY and enc_call(good, q=24) == NHW_E_QUALITY
    assert tile_call(good, t=None) == NHW_E_ARG and tile_call(good, n_pics=0) == NHW_E_ARG and tile_call(good, m=0) == NHW_E_ARG and tile_call(good, tile0=-1) == NHW_E_ARG
    assert untouched()
    assert _encode(enc, enc.encode_device, d_px, 20) == before          # the handle still encodes bytes as it did
    assert enc_call(good) == 0 and not untouched()                      # ... and the same call with nothing wrong does run


@pytest.mark.gpu
def test_gpu_python_argument_errors(enc):
    import torch
    import nhwcodec_amd as na
    fmt = na.TensorFormat("float32", "CHW", "RGB", "reversed")
    x = torch.zeros((2, 3, 512, 512), dtype=torch.float32, device="cuda")
    flat = torch.zeros((2 * 3 * 512 * 512 + 4,), dtype=torch.float32, device="cuda")
    for call in (lambda: enc.encode_tensor_device(x, "float32"), lambda: enc.encode_tensor_device(x.half(), fmt), lambda: enc.encode_tensor_device(x.cpu(), fmt),
                 lambda: enc.encode_tensor_device(x.permute(0, 2, 3, 1), fmt), lambda: enc.encode_tensor_device(x.flip(0).transpose(2, 3), fmt),
                 lambda: enc.encode_tensor_device(flat[1:-3].view(2, 3, 512, 512), fmt),                          # 4 bytes off
                 lambda: na.tensor_to_bytes_device(x.transpose(2, 3), fmt), lambda: na.tensor_to_bytes_device(flat[1:-3].view(2, 3, 512, 512), fmt),
                 lambda: na.tile_tensors_device([x[0], x[1].cpu()], fmt), lambda: na.tile_tensors_device([x[0].half()], fmt),
                 lambda: na.tile_tensors_device([x[0].transpose(1, 2)], fmt), lambda: na.tile_tensors_device([x[0, :, :, ::2]], fmt),
                 lambda: na.tile_tensors_device([x[0].permute(1, 2, 0)], na.TensorFormat("float32", "HWC", "RGB", "reversed")),
                 lambda: na.tile_tensors_device([torch.zeros((3, 1, 65536), dtype=torch.float32, device="cuda")], fmt)):
        with pytest.raises(na.NhwError):
            call()
    with pytest.raises(ValueError):
        enc.encode_tensor_device(x, fmt, out=enc.alloc_out(2)[:2])
