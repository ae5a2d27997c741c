"""What a decode must produce, as bytes and as tensors, shared by test_scaled_decode.py, test_tensor_decode.py, test_tensor_values.py,
test_tensor_encode.py, test_crops.py, test_decode_values.py and test_decode_surgery.py: section 14's half- and quarter-scale pictures built from the oracle decoder's intermediate
planes, section 16's tensors made on the CPU from the specification in exact arithmetic, and the decode calls into guarded buffers that are held against them.
Each module's own docstring says why these are the expected values."""
import ctypes
import fractions
import functools
import hashlib
import itertools
import math
import struct

import numpy as np

from tests.support import CANARY, device_arena

SENTINEL = 0xA5
TAIL = 4096                                     # sentinel bytes kept behind every output

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CONSTANTS = {                                   # name -> TensorFormat keywords
    "imagenet": dict(mean=IMAGENET_MEAN, std=IMAGENET_STD),
    "unit": dict(scale=1 / 255, bias=0),
    "negative": dict(scale=(-1 / 255, -0.5, -2.0), bias=(1.0, 127.5, 3.25)),
    "identity": dict(scale=1, bias=0),
}
DTYPES = ("uint8", "float16", "bfloat16", "float32")
ALL_FORMATS = list(itertools.product(DTYPES, ("HWC", "CHW"), ("BGR", "RGB"), ("file", "reversed")))      # 32


# ---------------------------------------------------------------- the scaled pictures: probes -> planes -> nhwo_dec_color
def _probe16(oracle, nhw, pid, stride):
    return np.frombuffer(oracle.decode_probe(nhw, pid), np.int16).reshape(-1, stride)


def expected_planes(oracle, nhw, scale):
    """(Y, U, V) uint8 [T, T] of section 14's definition, and the file's quality"""
    clip = lambda a: np.clip(a, 0, 255).astype(np.uint8)
    q = oracle.decode(nhw)[1]
    if scale == 2:
        y = clip(_probe16(oracle, nhw, 6, 512)[:256, :256])
        u, v = (clip(_probe16(oracle, nhw, 46 + c, 256)[:256, :256]) for c in (0, 1))
    else:
        y = clip(_probe16(oracle, nhw, 4, 512)[:128, :128].T)
        u, v = (clip(_probe16(oracle, nhw, 42 + c, 256)[:128, :128]) for c in (0, 1))
    return np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v), q


def oracle_colour(oracle, y, u, v, q):
    """the file's own quality branch of nhwo_dec_color on small planes: the function walks 262144 pixels, so the planes sit at the front of
    zero-padded arrays and the first T * T pixels come back"""
    t = y.shape[0]
    fn = oracle.lib.nhwo_dec_color
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    fn.restype = None
    pad = [np.zeros(4 * 65536, np.uint8) for _ in range(3)]
    for p, a in zip(pad, (y, u, v)):
        p[:t * t] = a.reshape(-1)
    out = np.empty(12 * 65536, np.uint8)
    fn(pad[0].ctypes.data, pad[1].ctypes.data, pad[2].ctypes.data, q, out.ctypes.data)
    return out[:3 * t * t].reshape(t, t, 3).copy()


_EXPECTED = {}


def expected(oracle, nhw, scale):
    """the expected scaled picture of a file, uint8 [T, T, 3]; computed once a (file, scale) and never written to"""
    key = (hashlib.sha1(nhw).digest(), scale)
    if key not in _EXPECTED:
        y, u, v, q = expected_planes(oracle, nhw, scale)
        px = oracle_colour(oracle, y, u, v, q)
        px.setflags(write=False)
        _EXPECTED[key] = px
    return _EXPECTED[key]


_BYTES = {}


def expected_bytes(oracle, nhw, scale):
    """the byte path's picture of a file, uint8 [S, S, 3]: the oracle decoder's at scale 1, section 14's at 2 and 4; computed once, never written to"""
    if scale != 1:
        return expected(oracle, nhw, scale)
    if nhw not in _BYTES:
        px = np.array(oracle.decode(nhw)[0], np.uint8).reshape(512, 512, 3)
        px.setflags(write=False)
        _BYTES[nhw] = px
    return _BYTES[nhw]


def decode_scaled(dec, files, scale):
    """one decode_scaled_device call into a canary-backed buffer -> (pixels, status, quality) on the host; the canary is checked"""
    import torch
    n, t = len(files), 512 // scale
    room = n * 3 * t * t
    buf = torch.full((room + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    px, st, qq = dec.decode_scaled_device(*device_arena(files), scale, out=buf)
    torch.cuda.synchronize()
    assert tuple(px.shape) == (n, t, t, 3) and px.data_ptr() == buf.data_ptr()
    assert bool((buf[room:] == CANARY).all()), "bytes behind n * 3 T T were written"
    return px.cpu().numpy(), st.cpu().numpy(), qq.cpu().numpy()


# ---------------------------------------------------------------- the tensors
def tensor_format(dtype, layout, channels, rows, constants=None):
    """the TensorFormat of a parameter tuple; the float types walk through CONSTANTS so that every set meets every dtype"""
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, channels, rows)
    if constants is None:
        constants = list(CONSTANTS)[ALL_FORMATS.index((dtype, layout, channels, rows)) % len(CONSTANTS)]
    return na.TensorFormat(dtype, layout, channels, rows, **CONSTANTS[constants])


def check_constants(fmt):
    """a remark, no longer a gate: the condition under which the float64 shortcut (product and sum in double, one astype(float32)) IS the
    single-precision fma.  expected_tensor does not take the shortcut any more; test_tensor_values.py holds exact_elements against it on
    every set of CONSTANTS, which all meet this condition"""
    for s, b in zip(fmt.scale, fmt.bias):
        assert np.float32(s) == s and np.float32(b) == b and np.isfinite(s) and np.isfinite(b) and s != 0
        assert b == 0 or abs(int(np.frexp(s)[1]) - int(np.frexp(b)[1])) <= 20, (s, b)


# the value rule of a decode in exact arithmetic.  A binary format here: (significand bits with the hidden one, exponent of the smallest subnormal,
# exponent of the largest binade, width in bits)
BINARY = {"float32": (24, -149, 127, 32), "float16": (11, -24, 15, 16), "bfloat16": (8, -133, 127, 16), "float64": (53, -1074, 1023, 64)}
NP_BITS = {"uint8": np.uint8, "float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}


def binade(a):
    """the e with 2^e <= a < 2^(e + 1), for a rational a > 0"""
    e = a.numerator.bit_length() - a.denominator.bit_length()
    return e if a >= fractions.Fraction(2) ** e else e - 1


def quantum(a, dtype_name):
    """the spacing of the format's values around the rational a > 0 (as if the exponent had no upper end): a power of two"""
    p, low, _, _ = BINARY[dtype_name]
    return fractions.Fraction(2) ** max(binade(a) - (p - 1), low)


def round_to_binary(a, dtype_name):
    """a rational a >= 0 rounded once to the format, to nearest, ties to even -> the rational the format holds (0 where a underflows), or
    math.inf where the rounded value lies above the largest finite one (float16: from 65520 on).  Subnormals are values like any other"""
    if a == 0:
        return a
    p, _, top, _ = BINARY[dtype_name]
    q = quantum(a, dtype_name)
    r = round(a / q) * q                         # round(Fraction): half to even
    return r if r <= (2 ** p - 1) * fractions.Fraction(2) ** (top - p + 1) else math.inf


def is_tie(a, dtype_name):
    """the rational a > 0 lies exactly midway between two neighbouring values of the format (or between the largest and the next power of two)"""
    return (a / quantum(a, dtype_name)).denominator == 2


def binary_bits(negative, a, dtype_name):
    """the bit pattern of (-1)^negative * a, a a value of the format or math.inf"""
    p, low, top, width = BINARY[dtype_name]
    sign = int(bool(negative)) << (width - 1)
    if a == math.inf:
        return sign | (2 ** (width - p) - 1) << (p - 1)
    m = a / fractions.Fraction(2) ** low
    assert m.denominator == 1
    m = int(m)
    if m < 1 << (p - 1):                         # zero and the subnormals: exponent field 0
        return sign | m
    e = m.bit_length() - p                       # a = (m >> e) * 2^(low + e), m >> e a full significand
    assert m == (m >> e) << e and low + e + p - 1 <= top
    return sign | (e + 1) << (p - 1) | ((m >> e) - (1 << (p - 1)))


def _f32_key(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@functools.lru_cache(maxsize=None)
def _exact_elements(scale_bits, bias_bits, dtype_name):
    scale, bias = (struct.unpack("<f", struct.pack("<I", v))[0] for v in (scale_bits, bias_bits))
    assert math.isfinite(scale) and math.isfinite(bias)
    s, c = fractions.Fraction(scale), fractions.Fraction(bias)
    out = np.empty(256, NP_BITS[dtype_name])
    for b in range(256):
        v = b * s + c
        if v != 0:
            negative = v < 0
        else:                                    # -0 only as (-0) + (-0): a zero product takes the scale's sign, a sum that cancels is +0
            negative = b * s == 0 and math.copysign(1.0, scale) < 0 and math.copysign(1.0, bias) < 0
        a = round_to_binary(abs(v), "float32")
        if dtype_name != "float32" and a != math.inf:
            a = round_to_binary(a, dtype_name)
        out[b] = binary_bits(negative, a, dtype_name)
    out.setflags(write=False)
    return out


def exact_elements(scale, bias, dtype_name):
    """DESIGN.md section 16's value rule in rationals: the 256 bit patterns (uint32 or uint16, read-only) that bytes 0 .. 255 give under the
    float32 constants scale and bias.  The exact b * scale + bias is rounded once to float32 (24 bits, subnormals down to 2^-149, infinity
    above FLT_MAX) -- the fma -- and that value once more to the type (float16: 11 bits, subnormals down to 2^-24, infinity from 65520 on;
    bfloat16: 8 bits, float32's exponents); both to nearest, ties to even.  Signs: a value that is not zero keeps its sign through both
    roundings, also where it rounds to zero; an exact sum of zero is +0, unless the product b * scale and the bias are both negative zeros
    (b = 0 or scale = -0 with scale < 0 or -0, bias -0), which give -0"""
    assert dtype_name in ("float32", "float16", "bfloat16") and float(np.float32(scale)) == scale and float(np.float32(bias)) == bias, (scale, bias, dtype_name)
    return _exact_elements(_f32_key(scale), _f32_key(bias), dtype_name)


def expected_tensor(px, fmt):
    """the specification on the CPU: px uint8 [H, W, 3] as the byte path writes it -> the bit patterns of the tensor, [H, W, 3] or [3, H, W]:
    a lookup in one table of exact_elements per output channel"""
    b = px[..., ::-1] if fmt.channels == "RGB" else px
    if fmt.dtype_name == "uint8":
        bits = b.copy()
    else:
        bits = np.stack([exact_elements(fmt.scale[c], fmt.bias[c], fmt.dtype_name)[b[..., c]] for c in range(3)], axis=-1)
    if fmt.rows == "reversed":
        bits = bits[::-1]
    if fmt.layout == "CHW":
        bits = bits.transpose(2, 0, 1)
    return np.ascontiguousarray(bits)


def first_difference(got, px, fmt):
    """got: a tensor's bit patterns in fmt's own layout, px: the bytes uint8 [H, W, 3] it was made of -> None where got is expected_tensor(px,
    fmt), else a sentence naming the first differing (byte, output channel, constant pair)"""
    want = expected_tensor(px, fmt)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = got != want
    if not bad.any():
        return None
    hwc = lambda a: (a.transpose(1, 2, 0) if fmt.layout == "CHW" else a)[::-1 if fmt.rows == "reversed" else 1]
    y, x, c = (int(v) for v in np.argwhere(hwc(bad))[0])
    b = int(px[y, x, 2 - c if fmt.channels == "RGB" else c])
    return (f"{int(bad.sum())} of {bad.size} elements differ; the first: byte {b} in output channel {c} under scale {float(fmt.scale[c]).hex()}, bias "
            f"{float(fmt.bias[c]).hex()} as {fmt.dtype_name} gives {int(hwc(got)[y, x, c]):#x}, the rule {int(hwc(want)[y, x, c]):#x} (row {y}, column {x} of the byte picture)")


def tensor_bits(t):
    """a tensor's bit patterns on the host, as unsigned integers"""
    import torch
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def decode_tensor(dec, files, fmt, scale):
    """one decode_tensor_device call into a sentinel-filled buffer -> (the tensor's bit patterns, status, quality) on the host; what lies behind
    n * 3 * S * S elements is checked"""
    import torch
    n, s = len(files), 512 // scale
    room = n * 3 * s * s * fmt.dtype.itemsize
    buf = torch.full((room + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[:room].view(fmt.dtype)
    t, st, qq = dec.decode_tensor_device(*device_arena(files), fmt, scale=scale, out=out)
    torch.cuda.synchronize()
    assert t.dtype == fmt.dtype and tuple(t.shape) == (n,) + fmt.shape(s, s) and t.data_ptr() == buf.data_ptr()
    assert bool((buf[room:] == SENTINEL).all()), "elements behind n * 3 * S * S were written"
    return tensor_bits(t), st.cpu().numpy(), qq.cpu().numpy()


def assert_tensor(oracle, got, files, status, fmt, scale, what=""):
    for i, f in enumerate(files):
        if status[i]:
            assert (got[i].view(np.uint8) == SENTINEL).all(), f"{what}: refused file {i}: its slot was written"
            continue
        want = expected_tensor(expected_bytes(oracle, f, scale), fmt)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape
        bad = got[i] != want
        assert not bad.any(), f"{what} {fmt} scale {scale} file {i}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"
