"""The value rule of a decode (nhw_tensor_elem in nhw_tensor.h) on every byte, at the edges of the number formats: ties of
float16 and bfloat16 (among the subnormals too), float16's overflow threshold, float32 subnormals of both signs, the fma's single rounding where
a separate product overflows, infinities, the carry of the integer bfloat16 rounding into infinity, the sign of zero, and the pairs on which
"fma to float32, then round to the type" (the rule) differs from one rounding of the exact value.

The expected values are tests/tensor_cases.py's exact_elements: the rule in rationals, hand-checked below.  The table PAIRS names what each
(scale, bias) is there for; test_every_pair_hits_its_edges recomputes the count of bytes in each class on the CPU, so an edit cannot quietly lose
an edge.  The mutants of test_restated_mutants_are_caught_by_the_table are the mistakes the table is there to catch, restated in Python.

On the GPU every storing kernel meets every byte under every pair as every float type, bit for bit: k_bytes_to_tensor, k_resize_to_tensor,
k_area_to_tensor and k_cubic_to_tensor on two small pictures whose channels each hold all 256 values (the three resampling kernels at the
source's own size, where they reproduce it -- asserted first under the byte format), the pairs rotated through the three channel slots; and the
decoder's last kernels at scales 1, 2 and 4 on seven files whose expected bytes, by the oracle, hold every value in every channel at every
scale."""
import ctypes
import fractions
import itertools
import math

import numpy as np
import pytest

from oracle.harness import class_image
from tests.support import CANARY
from tests.tensor_cases import (BINARY, CONSTANTS, NP_BITS, binary_bits, check_constants, decode_tensor, exact_elements, expected_bytes, expected_tensor,
                                first_difference, is_tie, round_to_binary, tensor_bits, tensor_format)

F = fractions.Fraction
FLOATS = ("float16", "bfloat16", "float32")
FLT_MAX = float.fromhex("0x1.fffffep+127")
GUARD = 4096
# TensorFormat(mean=IMAGENET_MEAN, std=IMAGENET_STD)'s float32 constants (test_tensor_decode.py holds them against the arithmetic)
IMAGENET_SCALE32 = (0.017124753445386887, 0.017507001757621765, 0.01742919348180294)
IMAGENET_BIAS32 = (-2.1179039478302, -2.0357141494750977, -1.804444432258606)

# name -> (scale, bias, {class: the number of bytes 0 .. 255 in it}); the classes are those of classify()
PAIRS = {
    "f16 ties": (1 + 2.0 ** -11, 0.0, {"f16 tie": 8}),                                  # b = 2^k: b + b 2^-11 lies midway
    "f16 ties, half the bytes": (3 * 2.0 ** -11, 1.0, {"f16 tie": 128, "bf16 tie": 16}),
    "bf16 ties": (1 + 2.0 ** -8, 0.0, {"bf16 tie": 8, "f16 tie": 20}),
    "f16 subnormals": (2.0 ** -22, 0.0, {"f16 subnormal": 255}),
    "f16 subnormal ties": (3 * 2.0 ** -26, 0.0, {"f16 subnormal tie": 64, "f16 subnormal": 255}),
    "f16 overflow at 255": (257.0, 0.0, {"f16 inf": 1}),
    "f16 largest finite": (256.0, 239.0, {"f16 inf": 0}),                              # 65519 stays 65504
    "f32 subnormals": (2.0 ** -149, 0.0, {"f32 subnormal": 255, "f16 zero of a nonzero": 255, "bf16 zero of a nonzero": 255}),
    "f32 subnormals, both signs": (2.0 ** -133, -2.0 ** -127, {"f32 subnormal": 191, "f32 negative subnormal": 64, "bf16 subnormal": 191, "f16 -0 of a nonzero": 64}),
    "FLT_MAX": (FLT_MAX, -FLT_MAX, {"f32 inf": 253, "product overflows, fma finite": 1, "bf16 inf": 2, "f16 inf": 2}),
    "f32 overflow": (2.0 ** 121, 0.0, {"f32 inf": 128, "f16 inf": 127}),
    "-0 at byte 0": (-1.0, -0.0, {"-0": 1}),
    "f16 negative underflow": (-2.0 ** -30, 0.0, {"f16 -0 of a nonzero": 32, "f16 subnormal": 223, "f16 subnormal tie": 4}),
    "f16 -0 for every byte above 0": (-2.0 ** -33, 0.0, {"f16 -0 of a nonzero": 255}),
    "+0 from 0 b + -0": (0.0, -0.0, {"-0": 0}),
    "the bias alone": (0.0, 254.5, {"bf16 tie": 256}),
    "f16 two-step": (1 + 2.0 ** -11, 2.0 ** -40, {"f16 two-step": 8, "f16 tie": 8}),
    "bf16 two-step": (1 + 2.0 ** -8, 2.0 ** -40, {"bf16 two-step": 8, "bf16 tie": 8}),
    "float64 shortcut fails at 130": (float.fromhex("0x1.f81f82p-32"), 1.0, {"float64 shortcut differs": 1}),
    "float64 shortcut fails at 205": (float.fromhex("0x1.3fb014p-32"), 1.0, {"float64 shortcut differs": 1}),
    "imagenet 0": (IMAGENET_SCALE32[0], IMAGENET_BIAS32[0], {"fma differs": 133}),
    "imagenet 1": (IMAGENET_SCALE32[1], IMAGENET_BIAS32[1], {"fma differs": 120}),
    "imagenet 2": (IMAGENET_SCALE32[2], IMAGENET_BIAS32[2], {"fma differs": 124}),
    "negative bf16 ties": (-2.0, 3.25, {"bf16 tie": 32}),
}
NAMES = list(PAIRS)
TRIPLES = [NAMES[k:k + 3] for k in range(0, len(NAMES), 3)]
SHAPES = list(itertools.product(("HWC", "CHW"), ("BGR", "RGB"), ("file", "reversed")))      # layout, channels, rows


def _f32(x):
    return float(np.float32(x)) == x


def _float64_form(scale, bias, dtype_name):
    """what expected_tensor was before: product and sum in float64, astype(float32), then the type's own rounding (numpy's, torch's)"""
    import torch
    with np.errstate(over="ignore"):
        x = (np.arange(256).astype(np.float64) * np.float64(scale) + np.float64(bias)).astype(np.float32)
    if dtype_name == "float32":
        return x.view(np.uint32)
    if dtype_name == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _fma(b, scale, bias):
    """the fma of the rule in rationals -> (the exact value, the magnitude float32 holds or math.inf)"""
    v = b * F(scale) + F(bias)
    return v, round_to_binary(abs(v), "float32")


def classify(scale, bias):
    """{class: [bytes]} of a pair, from the exact arithmetic alone"""
    out = {}
    add = lambda k, b: out.setdefault(k, []).append(b)
    short = _float64_form(scale, bias, "float32")
    for b in range(256):
        v, x = _fma(b, scale, bias)
        if v == 0 and exact_elements(scale, bias, "float32")[b] >> 31:
            add("-0", b)
        if int(short[b]) != int(exact_elements(scale, bias, "float32")[b]):
            add("float64 shortcut differs", b)
        prod = round_to_binary(abs(b * F(scale)), "float32")
        if prod == math.inf:
            add("product overflows" + (", fma finite" if x != math.inf else ""), b)
        elif round_to_binary(abs((prod if scale >= 0 else -prod) + F(bias)), "float32") != x:
            add("fma differs", b)
        if x == math.inf:
            add("f32 inf", b)
            continue
        if 0 < x < F(2) ** -126:
            add("f32 subnormal", b)
            if v < 0:
                add("f32 negative subnormal", b)
        for dt, tag in (("float16", "f16"), ("bfloat16", "bf16")):
            if x == 0:
                continue
            normal = F(2) ** (BINARY[dt][1] + BINARY[dt][0] - 1)                          # the smallest normal value
            r = round_to_binary(x, dt)
            if is_tie(x, dt):
                add(tag + " tie", b)
                if x < normal:
                    add(tag + " subnormal tie", b)
            if r == math.inf:
                add(tag + " inf", b)
                continue
            if 0 < r < normal:
                add(tag + " subnormal", b)
            if r == 0:
                add(tag + " zero of a nonzero", b)
                if v < 0:
                    add(tag + " -0 of a nonzero", b)
            if round_to_binary(abs(v), dt) != r:
                add(tag + " two-step", b)
    return out


# ---------------------------------------------------------------- without a GPU
def test_the_constants_are_float32_and_fill_the_triples():
    assert len(NAMES) == 24 and all(len(t) == 3 for t in TRIPLES)
    for name, (scale, bias, _) in PAIRS.items():
        assert _f32(scale) and _f32(bias) and math.isfinite(scale) and math.isfinite(bias), name
    import nhwcodec_amd as na
    f = na.TensorFormat("float16", scale=(-1.0, 2.0 ** -149, FLT_MAX), bias=(-0.0, -2.0 ** -127, -FLT_MAX))     # the constants reach the C struct as they are
    c = f.c_struct()
    assert [float(v).hex() for v in c.scale] == [(-1.0).hex(), (2.0 ** -149).hex(), FLT_MAX.hex()]
    assert [float(v).hex() for v in c.bias] == [(-0.0).hex(), (-2.0 ** -127).hex(), (-FLT_MAX).hex()]
    im = na.TensorFormat("float32", mean=CONSTANTS["imagenet"]["mean"], std=CONSTANTS["imagenet"]["std"])
    assert im.scale == IMAGENET_SCALE32 and im.bias == IMAGENET_BIAS32


def test_hand_worked_values():
    """the reference itself, on values worked by hand, before any device is asked"""
    e = exact_elements
    # the rounder alone
    assert round_to_binary(F(65519), "float16") == 65504 and round_to_binary(F(65520), "float16") == math.inf and is_tie(F(65520), "float16")
    assert round_to_binary(F(2) ** -25, "float16") == 0 and round_to_binary(F(3, 2 ** 25), "float16") == F(2) ** -23      # ties among the smallest: to even
    assert round_to_binary(F(2) ** -150, "float32") == 0 and round_to_binary(F(3, 2 ** 150), "float32") == F(2) ** -148
    assert round_to_binary(F(2) ** 128 - F(2) ** 103, "float32") == math.inf and round_to_binary(F(2) ** 128 - F(2) ** 103 - 1, "float32") == F(FLT_MAX)
    assert round_to_binary(F(FLT_MAX), "bfloat16") == math.inf and round_to_binary(F(FLT_MAX), "float16") == math.inf
    assert [binary_bits(0, F(1), dt) for dt in FLOATS] == [0x3C00, 0x3F80, 0x3F800000]
    assert [binary_bits(1, math.inf, dt) for dt in FLOATS] == [0xFC00, 0xFF80, 0xFF800000]
    assert binary_bits(0, F(2) ** -24, "float16") == 1 and binary_bits(0, F(2) ** -14, "float16") == 0x0400 and binary_bits(0, F(65504), "float16") == 0x7BFF
    assert binary_bits(1, F(2) ** -149, "float32") == 0x80000001 and binary_bits(0, F(FLT_MAX), "float32") == 0x7F7FFFFF
    # 257 * 255 = 65535 is infinity in float16, 257 * 254 = 65278 rounds to 65280
    assert e(257.0, 0.0, "float16")[255] == 0x7C00 and e(257.0, 0.0, "float16")[254] == 0x7BF8 and e(257.0, 0.0, "float32")[255] == 0x477FFF00
    assert (e(257.0, 0.0, "float16")[:255] < 0x7C00).all()
    # 256 * 255 + 239 = 65519, one below the threshold
    assert e(256.0, 239.0, "float16")[255] == 0x7BFF and e(256.0, 239.0, "float32")[255] == 0x477FEF00 and e(256.0, 239.0, "bfloat16")[255] == 0x4780
    # FLT_MAX b - FLT_MAX: -FLT_MAX, +0, FLT_MAX (the product 2 FLT_MAX is not a float), then infinity
    assert e(FLT_MAX, -FLT_MAX, "float32")[:4].tolist() == [0xFF7FFFFF, 0, 0x7F7FFFFF, 0x7F800000] and (e(FLT_MAX, -FLT_MAX, "float32")[3:] == 0x7F800000).all()
    assert e(FLT_MAX, -FLT_MAX, "bfloat16")[:4].tolist() == [0xFF80, 0, 0x7F80, 0x7F80]                 # 0x7F7FFFFF + 0x7FFF + 1 carries into the exponent
    assert e(FLT_MAX, -FLT_MAX, "float16")[:4].tolist() == [0xFC00, 0, 0x7C00, 0x7C00]
    # 3 b 2^-26 in units of 2^-24: 0.75, 1.5, 2.25 -> 1, 2, 2; b = 6: 4.5 -> 4, b = 10: 7.5 -> 8
    assert e(3 * 2.0 ** -26, 0.0, "float16")[[1, 2, 3, 6, 10]].tolist() == [1, 2, 2, 4, 8]
    # the signs of zero
    for dt, sign in (("float16", 0x8000), ("bfloat16", 0x8000), ("float32", 0x80000000)):
        assert e(-1.0, -0.0, dt)[0] == sign and e(-1.0, 0.0, dt)[0] == 0 and e(1.0, -0.0, dt)[0] == 0             # (-0) + (-0); (-0) + (+0); (+0) + (-0)
        assert (e(0.0, -0.0, dt) == 0).all() and (e(-0.0, -0.0, dt) == sign).all() and (e(-0.0, 0.0, dt) == 0).all()
        assert e(-1.0, 1.0, dt)[1] == 0 and e(1.0, -1.0, dt)[1] == 0                                              # a sum that cancels
    assert (e(-2.0 ** -33, 0.0, "float16")[1:] == 0x8000).all() and e(-2.0 ** -33, 0.0, "float16")[0] == 0        # what underflows keeps its sign
    assert e(-2.0 ** -30, 0.0, "float16")[[1, 32, 33, 96]].tolist() == [0x8000, 0x8000, 0x8001, 0x8002]             # 32: the tie 0.5 to even; 96: 1.5 to 2
    assert (e(-2.0 ** -149, 0.0, "bfloat16")[1:] == 0x8000).all() and e(-2.0 ** -149, 0.0, "float32")[255] == 0x800000FF
    # the two roundings: 1 + 2^-11 + 2^-40 lies above float16's midpoint, its float32 on it
    assert e(1 + 2.0 ** -11, 2.0 ** -40, "float32")[1] == 0x3F801000 and e(1 + 2.0 ** -11, 2.0 ** -40, "float16")[1] == 0x3C00
    assert binary_bits(0, round_to_binary(F(1 + 2.0 ** -11) + F(2) ** -40, "float16"), "float16") == 0x3C01
    assert e(1 + 2.0 ** -8, 2.0 ** -40, "bfloat16")[1] == 0x3F80 and binary_bits(0, round_to_binary(F(1 + 2.0 ** -8) + F(2) ** -40, "bfloat16"), "bfloat16") == 0x3F81
    # where float64 is not enough: 130 * 0x1.f81f82p-32 lies 2^-54 above 2^-24: the float64 sum drops that quarter of its last place
    # and lands on float32's midpoint
    s = float.fromhex("0x1.f81f82p-32")
    assert 130 * F(s) - F(2) ** -24 == F(2) ** -54 and e(s, 1.0, "float32")[130] == 0x3F800001 and _float64_form(s, 1.0, "float32")[130] == 0x3F800000


@pytest.mark.parametrize("dtype", FLOATS)
def test_exact_tables_equal_the_float64_form_on_the_suites_constants(dtype):
    """every expectation of the older tensor tests is what it was: on the four sets of CONSTANTS the lookup tables are the float64 form, bit
    for bit"""
    for name in CONSTANTS:
        fmt = tensor_format(dtype, "HWC", "BGR", "file", name)
        check_constants(fmt)
        for c in range(3):
            assert np.array_equal(exact_elements(fmt.scale[c], fmt.bias[c], dtype), _float64_form(fmt.scale[c], fmt.bias[c], dtype)), (name, c)
        px = np.random.default_rng(5).integers(0, 256, (5, 7, 3), dtype=np.uint8)
        for layout, channels, rows in SHAPES:
            f = tensor_format(dtype, layout, channels, rows, name)
            b = (px[..., ::-1] if channels == "RGB" else px)[::-1 if rows == "reversed" else 1]
            want = np.stack([_float64_form(f.scale[c], f.bias[c], dtype)[b[..., c]] for c in range(3)], -1)
            assert np.array_equal(expected_tensor(px, f), want.transpose(2, 0, 1) if layout == "CHW" else want)


@pytest.mark.parametrize("name", NAMES)
def test_every_pair_hits_its_edges(name):
    scale, bias, counts = PAIRS[name]
    got = classify(scale, bias)
    print(name, {k: len(v) for k, v in got.items()})
    for cls, n in counts.items():
        assert len(got.get(cls, [])) == n, (name, cls, got.get(cls))
    if name == "f16 overflow at 255":
        assert got["f16 inf"] == [255]
    if name == "FLT_MAX":
        assert got["product overflows, fma finite"] == [2] and got["bf16 inf"] == got["f16 inf"] == [0, 2] and got["f32 inf"] == list(range(3, 256))
    if name == "f32 overflow":
        assert got["f32 inf"] == list(range(128, 256))
    if name.startswith("float64 shortcut"):
        assert got["float64 shortcut differs"] == [int(name[-3:])]
    if name == "f16 ties":
        assert got["f16 tie"] == [1, 2, 4, 8, 16, 32, 64, 128] and "f16 two-step" not in got


def test_what_the_suites_constants_leave_out():
    """the four older sets hold bfloat16 ties and fma-against-product bytes, one float16 subnormal, and none of the other classes: why PAIRS exists"""
    seen = {}
    for name in CONSTANTS:
        fmt = tensor_format("float32", "HWC", "BGR", "file", name)
        for c in range(3):
            for cls, bs in classify(fmt.scale[c], fmt.bias[c]).items():
                seen[cls] = seen.get(cls, 0) + len(bs)
    assert set(seen) == {"bf16 tie", "fma differs", "f16 subnormal"} and seen["f16 subnormal"] == 1, seen


# ---- the mistakes the table is there to catch, restated
def _mutant(kind, scale, bias):
    """(dtype, the 256 bit patterns a wrong nhw_tensor_elem of that kind would give)"""
    u32 = exact_elements(scale, bias, "float32").astype(np.uint64)
    if kind == "bf16 truncates":
        return "bfloat16", (u32 >> 16).astype(np.uint16)
    if kind == "bf16 without the tie term":                            # (u + 0x7FFF) >> 16: a tie goes down
        return "bfloat16", ((u32 + 0x7FFF) >> 16).astype(np.uint16)
    if kind == "bf16 ties away":                                       # (u + 0x8000) >> 16
        return "bfloat16", ((u32 + 0x8000) >> 16).astype(np.uint16)
    dt = "float16" if "f16" in kind else "float32"
    out = exact_elements(scale, bias, dt).copy()
    flush = lambda c: 0.0 if abs(c) < 2.0 ** -126 else c
    for b in range(256):
        v, x = _fma(b, scale, bias)
        if kind == "product, then sum":
            prod = round_to_binary(abs(b * F(scale)), "float32")
            if prod == math.inf:
                out[b] = binary_bits(scale < 0, math.inf, dt)
                continue
            w = (prod if scale >= 0 else -prod) + F(bias)
            if w != 0:
                out[b] = binary_bits(w < 0, round_to_binary(abs(w), "float32"), dt)
        elif kind == "f16 straight from a double" and v != 0:
            out[b] = binary_bits(v < 0, round_to_binary(round_to_binary(abs(v), "float64"), dt), dt)
        elif kind == "f32 denormals flushed":
            w = b * F(flush(scale)) + F(flush(bias))
            r = round_to_binary(abs(w), "float32")
            out[b] = binary_bits(w < 0 or (w == 0 and out[b] >> 31), 0 if r < F(2) ** -126 else r, dt)
        elif kind == "f16 denormals flushed" and x != math.inf and round_to_binary(x, dt) < F(2) ** -14:
            out[b] = out[b] & 0x8000
    return dt, out


MUTANTS = {                                                            # kind -> the pairs that must catch it (others may too)
    "bf16 truncates": ["bf16 ties", "FLT_MAX", "negative bf16 ties", "imagenet 0"],
    "bf16 without the tie term": ["f16 ties, half the bytes", "negative bf16 ties", "f16 largest finite"],      # ties whose upper half is odd: they go up
    "bf16 ties away": ["bf16 ties", "the bias alone", "bf16 two-step"],                                        # ... and ties that stay: upper half even
    "product, then sum": ["FLT_MAX", "imagenet 0", "imagenet 1", "imagenet 2", "float64 shortcut fails at 130", "float64 shortcut fails at 205"],
    "f16 straight from a double": ["f16 two-step", "bf16 two-step"],
    "f32 denormals flushed": ["f32 subnormals", "f32 subnormals, both signs"],
    "f16 denormals flushed": ["f16 subnormals", "f16 subnormal ties", "f16 negative underflow"],
}


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_restated_mutants_are_caught_by_the_table(kind):
    caught = {}
    for name, (scale, bias, _) in PAIRS.items():
        dt, bits = _mutant(kind, scale, bias)
        n = int((bits != exact_elements(scale, bias, dt)).sum())
        if n:
            caught[name] = n
    print(kind, "is caught by", caught)
    assert all(name in caught for name in MUTANTS[kind]), (kind, caught)


# ---- the formats of the GPU tests
def formats(dtype, turn=None):
    """[(the three pair names by output channel, TensorFormat)]: every triple of PAIRS in all three rotations (or, with turn, in one rotation
    a triple, which varies with it), layouts, channel orders and row directions taken in turn"""
    import nhwcodec_amd as na
    out = []
    for t, names in enumerate(TRIPLES):
        for r in range(3) if turn is None else [(t + turn) % 3]:
            rot = names[r:] + names[:r]
            layout, channels, rows = SHAPES[(len(out) + 3 * FLOATS.index(dtype) + (turn or 0)) % len(SHAPES)]
            out.append((rot, na.TensorFormat(dtype, layout, channels, rows, scale=[PAIRS[n][0] for n in rot], bias=[PAIRS[n][1] for n in rot])))
    return out


def test_the_formats_rotate_every_pair_through_every_slot():
    for dtype in FLOATS:
        full = formats(dtype)
        assert len(full) == 24 and {(n, c) for rot, _ in full for c, n in enumerate(rot)} == set(itertools.product(NAMES, range(3)))
        assert {(f.layout, f.channels, f.rows) for _, f in full} == set(SHAPES)
        for rot, f in full:
            assert f.dtype_name == dtype and [float(v).hex() for v in f.scale] == [float(PAIRS[n][0]).hex() for n in rot]
            assert [float(v).hex() for v in f.bias] == [float(PAIRS[n][1]).hex() for n in rot]                      # -0.0 and the subnormals arrive
        for turn in range(9):
            some = formats(dtype, turn)
            assert len(some) == 8 and sorted(n for rot, _ in some for n in rot) == sorted(NAMES)
    assert len({(f.layout, f.channels, f.rows) for k in range(3) for _, f in formats(FLOATS[k], k)}) >= 6


class Coverage:
    """which (pair, byte) met a comparison"""

    def __init__(self):
        self.seen = {n: np.zeros(256, bool) for n in NAMES}

    def add(self, rot, px, fmt):
        b = px[..., ::-1] if fmt.channels == "RGB" else px
        for c, n in enumerate(rot):
            self.seen[n][np.unique(b[..., c])] = True

    def complete(self):
        return all(v.all() for v in self.seen.values())


# ---------------------------------------------------------------- on the MI355X: the pointwise kernels
def _all_bytes(i):
    return np.stack([i, 255 - i, (7 * i + 3) % 256], -1).astype(np.uint8)       # B, G, R: all 256 values in each (7 is odd)


class Pictures:
    """16 x 16 (pixel i holds byte i) and 256 x 3 (one value a column, the rows shifted by 85) as views of one device buffer of random bytes:
    odd addresses, a gap behind every row"""

    def __init__(self):
        import torch
        self.own = [_all_bytes(np.arange(256).reshape(16, 16)), _all_bytes((np.arange(256)[None, :] + 85 * np.arange(3)[:, None]) % 256)]
        for px in self.own:
            assert all(len(np.unique(px[..., c])) == 256 for c in range(3))
        host = np.random.default_rng(77).integers(0, 256, 8192, dtype=np.uint8)
        at, places = 1, []
        for k, px in enumerate(self.own):
            h, w = px.shape[:2]
            pitch = 3 * w + 5 + 2 * k
            places.append((at, pitch))
            for r in range(h):
                host[at + r * pitch: at + r * pitch + 3 * w] = px[r].reshape(-1)
            at = (at + h * pitch + 7) | 1
        assert at < len(host)
        self.buf = torch.from_numpy(host).cuda()
        self.views = [self.buf.as_strided(px.shape, (pitch, 3, 1), off) for (off, pitch), px in zip(places, self.own)]
        assert all(v.data_ptr() % 2 == 1 for v in self.views)
        for v, px in zip(self.views, self.own):
            assert np.array_equal(v.cpu().numpy(), px)


@pytest.fixture(scope="module")
def pictures():
    return Pictures()


KERNELS = {"bytes": None, "two_tap": 0, "area": 1, "cubic": 2}         # the name of the path -> nhw_resample_to_tensor_device's filter


def _guarded_launch(kernel, view, fmt):
    """one picture through the C entry of a path into a canary-filled buffer -> (the tensor's bit patterns in fmt's layout, guards intact)"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    h, w = int(view.shape[0]), int(view.shape[1])
    room = 3 * h * w * fmt.dtype.itemsize
    buf = torch.full((2 * GUARD + room,), CANARY, dtype=torch.uint8, device="cuda")
    addr = torch.tensor([buf.data_ptr() + GUARD], dtype=torch.int64, device="cuda")
    table = na._picture_table([view], "test")[0]
    c = fmt.c_struct()
    if KERNELS[kernel] is None:
        rc = L.nhw_bytes_to_tensor_device(table.data_ptr(), 1, ctypes.byref(c), addr.data_ptr(), None)
    else:
        rc = L.nhw_resample_to_tensor_device(table.data_ptr(), 1, w, h, KERNELS[kernel], ctypes.byref(c), None, addr.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, L.nhw_last_error()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == CANARY).all() and (host[GUARD + room:] == CANARY).all())
    return host[GUARD:GUARD + room].view(NP_BITS[fmt.dtype_name]).reshape(fmt.shape(h, w)), intact


def _wrapper(kernel, view, fmt):
    import nhwcodec_amd as na
    if kernel == "bytes":
        return tensor_bits(na.pictures_to_tensor_device([view], fmt)[0])
    return tensor_bits(na.resize_to_tensor_device([view], tuple(view.shape[:2]), fmt, filter=kernel))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [k for k in KERNELS if k != "bytes"])
def test_gpu_filters_reproduce_the_source_at_its_own_size(pictures, kernel):
    """under the plain byte format: what differs in the value tests below is then the value rule, not the resampling"""
    import nhwcodec_amd as na
    fmt = na.TensorFormat("uint8", "HWC", "BGR", "file")
    for view, px in zip(pictures.views, pictures.own):
        got, intact = _guarded_launch(kernel, view, fmt)
        assert intact and np.array_equal(got, px), (kernel, px.shape)
        assert np.array_equal(_wrapper(kernel, view, fmt), px), (kernel, px.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gpu_every_byte_under_every_pair_pointwise(pictures, kernel, dtype):
    """24 formats (every pair in every channel slot) on both pictures, through the C entry between guards and through the Python wrapper: bit
    patterns equal the exact rule's"""
    cover, compared = Coverage(), 0
    for rot, fmt in formats(dtype):
        for view, px in zip(pictures.views, pictures.own):
            got, intact = _guarded_launch(kernel, view, fmt)
            assert intact, f"{kernel} {fmt}: a byte outside the tensor was written"
            for what, bits in (("C entry", got), ("wrapper", _wrapper(kernel, view, fmt))):
                diff = first_difference(bits, px, fmt)
                assert diff is None, f"{kernel}, {what}, {px.shape[1]} x {px.shape[0]}, pairs {rot}: {diff}"
                compared += bits.size
            cover.add(rot, px, fmt)
    assert cover.complete()
    print(f"{kernel} {dtype}: {compared} elements compared; every byte under each of {len(NAMES)} pairs in each of the three channel slots")


# ---------------------------------------------------------------- on the MI355X: the decoder's last kernels
QUALITY = 23


def _ramps(kinds):
    x, y = np.meshgrid(np.arange(512), np.arange(512))
    d = {"x": x // 2, "y": y // 2, "d": (x + y) // 4}
    return np.stack([d[k] for k in kinds], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def files(oracle):
    """seven files at quality 23: black, white, the grey gradient, white noise, a ramp in each channel in three directions, its negative, and
    the ramps with the directions exchanged"""
    images = [class_image(k) for k in ("black", "white", "gradient", "noise")] + [_ramps("xyd"), 255 - _ramps("xyd"), _ramps("ydx")]
    return [oracle.encode(img, QUALITY) for img in images]


def test_the_files_hold_every_byte_in_every_channel_at_every_scale(oracle, files):
    """from the oracle alone: the union of the expected bytes of the files, a channel and a scale, is 0 .. 255"""
    assert len(files) <= 24
    for scale in (1, 2, 4):
        seen = np.zeros((3, 256), bool)
        for f in files:
            px = expected_bytes(oracle, f, scale)
            assert px.shape == (512 // scale, 512 // scale, 3)
            for c in range(3):
                seen[c, np.unique(px[..., c])] = True
        assert seen.all(), (scale, [np.flatnonzero(~seen[c]).tolist() for c in range(3)])


@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=16)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("scale", [1, 2, 4])
def test_gpu_every_byte_under_every_pair_decoded(dec, oracle, files, scale, dtype):
    """the store of k_dec_final and k_dec_scaled<2> / <4>: the seven files under eight formats that hold every pair once, the rotation moving
    with scale and type; every element equals the exact rule on the oracle's bytes, and nothing behind the batch is written"""
    cover, compared = Coverage(), 0
    for rot, fmt in formats(dtype, turn=3 * (scale // 2) + FLOATS.index(dtype)):
        bits, st, qq = decode_tensor(dec, files, fmt, scale)
        assert st.tolist() == [0] * len(files) and qq.tolist() == [QUALITY] * len(files)
        for i, f in enumerate(files):
            px = expected_bytes(oracle, f, scale)
            diff = first_difference(bits[i], px, fmt)
            assert diff is None, f"scale {scale}, file {i}, pairs {rot}: {diff}"
            compared += bits[i].size
            cover.add(rot, px, fmt)
    assert cover.complete()
    print(f"decoder scale {scale} {dtype}: {compared} elements compared; every byte under each of {len(NAMES)} pairs")
