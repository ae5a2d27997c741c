"""The blur rule without a GPU: the per-pixel functions and the predicate of nhwcodec_amd/csrc/nhw_blur.h held by a
stand-alone program (tests/blur/check.cpp, plain and under AddressSanitizer + UBSan; nothing is preloaded) against a 64-bit model and against the
numpy restatement of blur_cases on crafted pictures; the header alone; hand-worked values of the numpy model; the builders blur_taps,
blur_gaussian, blur_box and blur_fixed and their refusals; the integer rule's fidelity to the float64 convolution; the struct and the limits as the
header declares them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.blur_cases import BLUR, MAX_MIX, MIX_ONE, ONE, REFLECT, REPLICATE, blur_model, check_cases, check_text, gaussian, int_taps, ix, model_of, one_tap, record
from tests.nhw_surgery import can_sanitize
from tests.support import ROOT

CSRC = os.path.join(ROOT, "nhwcodec_amd", "csrc")
HEADER = os.path.join(CSRC, "nhw_blur.h")


def _build_check(tmp_path, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1"] if sanitize else ["-O2"]
    obj, exe = str(tmp_path / "check.o"), str(tmp_path / "blur_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-c", os.path.join(ROOT, "tests", "blur", "check.cpp"), "-o", obj])
    subprocess.check_call(["g++", *flags, obj, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_rule_matches_the_model_on_crafted_pictures(tmp_path, sanitize):
    if sanitize and not can_sanitize():
        pytest.skip("this machine's compiler cannot link and run a sanitized program")
    cases = check_cases()
    table = tmp_path / "cases.txt"
    table.write_text(check_text(cases))
    p = subprocess.run([_build_check(tmp_path, sanitize), str(table)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    n = len(cases)
    assert n >= 200 and f"cases {n}\n" in p.stdout and f"checked {sum(w * h * c for w, h, c, _, _ in cases)}\n" in p.stdout, p.stdout[-2000:]
    assert "\nmismatches 0\n" in p.stdout and "file mismatches 0\n" in p.stdout and "predicate errors 0\n" in p.stdout, p.stdout[-2000:]
    assert f"mix checked {15 * 65536}\n" in p.stdout and "mix mismatches 0\n" in p.stdout, p.stdout[-2000:]
    # the crafted cases do reach the extremes: a byte of 255 under radius 15, and a mix of +-16 against a difference of +-255
    assert any(int(r["rx"]) == 15 and int(r["ry"]) == 15 and px.min() == 255 for _, _, _, r, px in cases)
    for mix in (MAX_MIX, -MAX_MIX):
        diffs = [blur_model(px, r["wx"][:3], r["wy"][:1], MIX_ONE, int(r["border"])).astype(int) - px for _, _, _, r, px in cases if int(r["mix"]) == mix and int(r["rx"]) == 1]
        assert diffs and diffs[0].max() == 255 and diffs[0].min() == -255


def test_header_stands_alone():
    """g++ takes nhw_blur.h with no HIP header in front of it"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "hip/hip_runtime.h" not in open(HEADER).read()


def test_hand_worked_values_of_the_numpy_model():
    row = lambda *v: np.array([v], np.uint8)
    assert blur_model(row(0, 1), [16384, 16384, 0], [ONE], MIX_ONE, REPLICATE).tolist() == [[0, 1]]
    # pixel 1: 16384 x 0 + 16384 x 1 = 16384 -> h = (16384 + 64) >> 7 = 128, half a level -> b = (32768 x 128 + 2^22) >> 23 = 1: the half goes up
    assert blur_model(row(0, 1), [16384, 16384, 0], [ONE], MIX_ONE, REPLICATE)[0, 1] == 1
    assert blur_model(row(1, 0), [0, 16384, 16384], [ONE], MIX_ONE, REPLICATE)[0, 0] == 1
    mixed = lambda p, b, mix: int(np.clip(p + np.floor_divide(mix * (b - p) + 32768, 65536), 0, 255))
    assert mixed(250, 240, -MIX_ONE) == 255 and mixed(5, 20, -MIX_ONE) == 0                            # 260 and -10, clamped
    assert mixed(100, 101, 32768) == 101 and mixed(100, 99, 32768) == 100                              # +1/2 -> +1, -1/2 -> 0: halves go up
    # ... and through the model itself, a picture whose neighbour is the blurred byte (all of the weight in tap 0: b(x) = p(x - 1))
    left = lambda mix, *v: blur_model(row(*v), one_tap(1, 0), [ONE], mix, REPLICATE)[0].tolist()
    assert left(-MIX_ONE, 240, 250) == [240, 255] and left(-MIX_ONE, 20, 5) == [20, 0]
    assert left(32768, 101, 100) == [101, 101] and left(32768, 99, 100) == [99, 100]
    assert ix(np.arange(-3, 7), 4, REFLECT).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0]
    assert ix(np.arange(-3, 7), 4, REPLICATE).tolist() == [0, 0, 0, 0, 1, 2, 3, 3, 3, 3]
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for mix in (0, 1, -1, MIX_ONE, -MAX_MIX, MAX_MIX):                                                 # rx = ry = 0: z = p for every mix
        assert np.array_equal(blur_model(px, [ONE], [ONE], mix), px)
    g = int_taps(gaussian(1.3, 4))
    b = blur_model(px, g, g, MIX_ONE)
    assert np.array_equal(blur_model(px, g, g, 0), px) and not np.array_equal(b, px)                   # mix 0 keeps the picture, mix 1 gives b
    for v in (0, 1, 127, 255):                                                                         # a constant picture stays constant
        for mix in (MIX_ONE, -MAX_MIX, 12345):
            assert (blur_model(np.full((5, 6), v, np.uint8), g, int_taps([1.0] * 31), mix, REPLICATE) == v).all()
    assert np.array_equal(blur_model(px[..., 0], one_tap(2, 0), [ONE], MIX_ONE, REPLICATE)[:, 2:], px[:, :-2, 0])      # tap 0 is the pixel rx to the left


def test_builders():
    import nhwcodec_amd as na
    assert (na.BLUR_MAX_RADIUS, na.BLUR_ONE, na.BLUR_MAX_MIX) == (15, ONE, 16)
    for w in ([1.0], [1, 2, 1], [0.2, 0.2, 0.2, 0.2, 0.2], np.ones(31), [1e-9, 1, 1e-9], [3, 0, 0], [0, 0, 5.5]):
        t = na.blur_taps(w)
        assert sum(t) == ONE and len(t) == len(w) and all(type(v) is int and v >= 0 for v in t), w
        assert list(t) == int_taps(w), w
    assert na.blur_taps([1, 1, 1]) == (10923, 10922, 10923)                                            # 3 x 10923 = 32769: the centre gives one back
    assert na.blur_taps([1.0] * 7) == (4681, 4681, 4681, 4682, 4681, 4681, 4681)                       # 7 x 4681 = 32767: the centre takes the one that lacks
    for bad in ([], [1, 1], np.ones(33), [1, -1, 1], [0, 0, 0], [1, float("nan"), 1], [1, float("inf"), 1], "abc", None, [[1, 2, 1]], 1.0):
        with pytest.raises(na.NhwError):
            na.blur_taps(bad)
    for sigma in (0.1, 0.5, 1.0, 2.0, 5.0):
        for r in (0, 1, 5, 11, 15):
            t = na.blur_gaussian(sigma, r)
            assert len(t) == 2 * r + 1 and sum(t) == ONE and t == t[::-1] and list(t) == int_taps(gaussian(sigma, r)), (sigma, r)
        assert len(na.blur_gaussian(sigma)) == 2 * max(1, min(15, int(np.ceil(3 * sigma)))) + 1
    assert len(na.blur_gaussian(0.1)) == 3 and len(na.blur_gaussian(2.0)) == 13 and len(na.blur_gaussian(100.0)) == 31
    for bad in (dict(sigma=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma="x"), dict(sigma=1.0, radius=16), dict(sigma=1.0, radius=-1),
                dict(sigma=1.0, radius=1.5), dict(sigma=1.0, radius=True)):
        with pytest.raises(na.NhwError):
            na.blur_gaussian(**bad)
    for r in range(16):
        t = na.blur_box(r)
        assert len(t) == 2 * r + 1 and sum(t) == ONE and t == t[::-1] and list(t) == int_taps([1.0] * (2 * r + 1)) and len(set(t[:r])) <= 1
    for bad in (16, -1, 1.0, None):
        with pytest.raises(na.NhwError):
            na.blur_box(bad)


def test_blur_fixed():
    import nhwcodec_amd as na
    r = na.blur_fixed([1, 2, 1])
    assert r.dtype == BLUR and (int(r["rx"]), int(r["ry"]), int(r["mix"]), int(r["border"])) == (1, 1, MIX_ONE, REFLECT)
    assert r["wx"].tolist() == [8192, 16384, 8192] + [0] * 29 and r["wy"].tolist() == r["wx"].tolist() and not r["reserved"].any() and not r["reserved8"]
    r = na.blur_fixed(na.blur_gaussian(2.0, 11), [ONE], mix=-0.5, border="replicate")
    assert (int(r["rx"]), int(r["ry"]), int(r["mix"]), int(r["border"])) == (11, 0, -32768, REPLICATE) and r["wy"].tolist() == [ONE] + [0] * 31
    assert r["wx"][:23].tolist() == int_taps(gaussian(2.0, 11))
    asym = [1000, 2000, ONE - 3000]
    assert na.blur_fixed(asym)["wx"][:3].tolist() == asym                                              # integers that sum to 32768 are taken as they are
    assert na.blur_fixed(np.array(asym, np.uint16), one_tap(15, 30))["wy"][30] == ONE
    tie = lambda v: int(na.blur_fixed([1.0], mix=v)["mix"])
    assert (tie(0.5 / MIX_ONE), tie(1.5 / MIX_ONE), tie(2.5 / MIX_ONE), tie(-0.5 / MIX_ONE), tie(-1.5 / MIX_ONE)) == (0, 2, 2, 0, -2)      # ties to even
    assert tie(16.0) == MAX_MIX and tie(-16.0) == -MAX_MIX
    for bad in (dict(mix=16.0 + 1.0 / MIX_ONE), dict(mix=-16.0 - 1.0 / MIX_ONE), dict(mix=float("nan")), dict(mix=float("inf")), dict(mix="1"), dict(mix=None),
                dict(border="wrap"), dict(border=0), dict(taps_y=[1, 1]), dict(taps_y=[1, float("nan"), 1]), dict(taps_y=np.ones(33))):
        with pytest.raises(na.NhwError):
            na.blur_fixed(**{"taps_x": [1, 2, 1], **bad})
    for bad in ([], [1, -2, 1], "x", None, [0, 0, 0]):
        with pytest.raises(na.NhwError):
            na.blur_fixed(bad)
    mine = record(int_taps(gaussian(2.0, 11)), [ONE], -32768, REPLICATE)
    assert mine.tobytes() == r.tobytes()


def _header_struct(text):
    """nhw_blur as the header declares it, as a ctypes.Structure: the C layout rules applied to the header's own fields"""
    body = re.search(r"typedef struct nhw_blur \{(.*?)\} nhw_blur;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint16_t": ctypes.c_uint16, "uint8_t": ctypes.c_uint8}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            kind, names = decl.split(None, 1)
            for name in (v.strip() for v in names.split(",")):
                t = kinds[kind]
                for d in reversed([int(v) for v in re.findall(r"\[(\d+)\]", name)]):
                    t = t * d
                fields.append((re.match(r"\w+", name).group(0), t))
    return type("HeaderBlur", (ctypes.Structure,), {"_fields_": fields})


def test_struct_and_limits_as_the_header_declares_them():
    import nhwcodec_amd as na
    text = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    assert re.search(r"^#define NHW_BLUR_MAX_RADIUS\s+15\b", text, re.M) and re.search(r"^#define NHW_BLUR_ONE\s+32768\b", text, re.M)
    assert re.search(r"^#define NHW_BLUR_MAX_MIX\s+16\b", text, re.M) and re.search(r"enum \{ NHW_BLUR_REFLECT = 0, NHW_BLUR_REPLICATE = 1 \};", text)
    S = _header_struct(text)
    assert ctypes.sizeof(S) == 144 and ctypes.alignment(S) == 4
    assert {n: (getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_} == dict(wx=(0, 64), wy=(64, 64), mix=(128, 4), rx=(132, 1), ry=(133, 1), border=(134, 1),
                                                                                         reserved8=(135, 1), reserved=(136, 8))
    mine = np.dtype(na.BLUR_DTYPE)
    assert mine == BLUR and mine.itemsize == 144
    for n, _ in S._fields_:
        assert getattr(S, n).offset == mine.fields[n][1], n
    rec = na.blur_fixed([1, 2, 1], [1.0], mix=0.25, border="replicate")                                # blur_fixed's bytes, read through the header's struct
    s = S.from_buffer_copy(rec.tobytes())
    assert (list(s.wx[:3]), s.wy[0], s.mix, s.rx, s.ry, s.border) == ([8192, 16384, 8192], ONE, 16384, 1, 0, 1)
    assert na.BLUR_BORDERS == {"reflect": REFLECT, "replicate": REPLICATE}
    px = np.random.default_rng(7).integers(0, 256, (6, 7, 3), dtype=np.uint8)                          # ... and the record means to the model what its builder was given
    assert np.array_equal(model_of(px, rec), blur_model(px, [8192, 16384, 8192], [ONE], 16384, REPLICATE))


# ---------------------------------------------------------------- fidelity: the integer rule against the float64 convolution
def _float_blur(px, sigma, r):
    """the float64 convolution with the unquantised weights and the reflect border: px uint8 [H, W] -> float64 [H, W]"""
    w = gaussian(sigma, r)
    w = w / w.sum()
    p = np.pad(px.astype(np.float64), r, mode="reflect")
    H, W = px.shape
    rows = sum(w[j] * p[:, j:j + W] for j in range(2 * r + 1))
    return sum(w[j] * rows[j:j + H, :] for j in range(2 * r + 1))


@pytest.mark.parametrize("r", (1, 5, 11, 15))
@pytest.mark.parametrize("sigma", (0.1, 0.5, 1.0, 2.0, 5.0))
def test_fidelity_to_the_float_convolution(sigma, r):
    """The integer rule differs from the ROUNDED float64 result by one level at the most.  The bound is derived: rounding a tap moves it by at most
    1/2 in 32768 and the deficit, at most 31/2, goes to one tap, so a pass moves a pixel by less than 31 x 255 / 32768 = 0.24 levels; h's rounding
    adds 1/512; the last rounding adds 1/2: |integer - float| < 0.24 + 0.24 + 0.002 + 0.5 < 1, and the float's own rounding to a level adds at
    most 1/2 more, which leaves the two integers at most 1 apart (measured: a worst |integer - float| of 0.507)."""
    import nhwcodec_amd as na
    rng = np.random.default_rng(2611)
    taps = na.blur_gaussian(sigma, r)
    board = (((np.arange(40)[:, None] + np.arange(36)[None, :]) & 1) * 255).astype(np.uint8)
    worst = 0.0
    for name, px in (("random", rng.integers(0, 256, (40, 36), dtype=np.uint8)), ("checkerboard", board), ("constant", np.full((40, 36), 255, np.uint8))):
        got = blur_model(px, taps, taps, MIX_ONE, REFLECT).astype(np.int64)
        want = _float_blur(px, sigma, r)
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - np.rint(want).astype(np.int64)).max() <= 1, (name, sigma, r)
        if name == "constant":
            assert (got == 255).all(), (sigma, r)
    print(f"sigma {sigma}, radius {r}: worst |integer - float| {worst:.4f}")
    assert worst < 1.0
