"""The colour rule without a GPU: nhw_colour_apply and nhw_colour_within of nhwcodec_amd/csrc/nhw_colour.h held by a
stand-alone program (tests/colour/check.cpp, plain and under AddressSanitizer + UBSan; nothing is preloaded) against a 64-bit model on all 2^24
byte triples under every map of colour_cases.MAPS; the header alone; the Python face -- colour_matrix, colour_compose, colour_fixed, the
`colours` keyword's refusals before any device is touched --; the exported symbols and the struct as the header declares it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.colour_cases import COLOUR, GAIN, MAPS, OFFSET, ONE, SYMBOLS, apply_grey, apply_map, maps_text
from tests.nhw_surgery import can_sanitize
from tests.support import ROOT, load_lib

CSRC = os.path.join(ROOT, "nhwcodec_amd", "csrc")
HEADER = os.path.join(CSRC, "nhw_colour.h")
PROTOTYPES = """
int nhw_resample_mapped_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                         const uint8_t *d_flags, const nhw_colour_map *d_maps, const uint64_t *d_out_addr, void *stream);
int nhw_warp_mapped_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                     const nhw_warp *d_warps, const nhw_colour_map *d_maps, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_mapped_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const nhw_colour_map *maps,
                                   const uint64_t *dst_addr, int32_t *status, int filter);
int nhw_dec_warps_mapped_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                   uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const nhw_colour_map *maps,
                                   const uint64_t *dst_addr, int32_t *status);
"""


def _build_check(tmp_path, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1"] if sanitize else ["-O2"]
    obj, exe = str(tmp_path / "check.o"), str(tmp_path / "colour_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, "-I", CSRC, "-c", os.path.join(ROOT, "tests", "colour", "check.cpp"), "-o", obj])
    subprocess.check_call(["g++", *flags, "-pthread", obj, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_rule_matches_the_model_on_every_triple(tmp_path, sanitize):
    if sanitize and not can_sanitize():
        pytest.skip("this machine's compiler cannot link and run a sanitized program")
    table = tmp_path / "maps.txt"
    table.write_text(maps_text())
    p = subprocess.run([_build_check(tmp_path, sanitize), str(table)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    n = len(MAPS)
    assert n >= 12 and f"maps {n}\n" in p.stdout and f"checked {n * ((1 << 24) + 256)}\n" in p.stdout, p.stdout[-2000:]
    assert "mismatches 0\n" in p.stdout and "predicate errors 0\n" in p.stdout, p.stdout[-2000:]


def test_the_table_and_the_numpy_rule():
    """the table holds what the issue names, and the numpy rule the GPU tests use agrees with the rule's words on hand-worked values"""
    every = np.arange(256, dtype=np.uint8)
    px = np.stack([every, every[::-1], every], axis=1)
    assert np.array_equal(apply_map(px, MAPS["identity"]), px) and np.array_equal(apply_map(px, MAPS["inversion"]), 255 - px)
    assert apply_map(np.array([[1, 3, 255]], np.uint8), MAPS["half"]).tolist() == [[1, 2, 128]]                 # 0.5 -> 1, 1.5 -> 2: halves go up
    assert apply_map(np.array([[1, 3, 255]], np.uint8), MAPS["minus half"]).tolist() == [[200, 199, 73]]         # 199.5 -> 200, 198.5 -> 199, 72.5 -> 73
    assert apply_map(np.array([[1, 3, 255]], np.uint8), MAPS["minus half below zero"]).tolist() == [[3, 0, 0]]   # 2.5 -> 3; -1.5 -> -1 and -128 -> clamped
    assert apply_map(np.array([[10, 20, 30]], np.uint8), MAPS["rotation"]).tolist() == [[20, 30, 10]]
    assert apply_map(np.array([[255, 255, 255]], np.uint8), MAPS["luma mix"]).tolist() == [[255, 255, 255]]
    assert apply_map(np.array([[255, 255, 255], [0, 0, 0]], np.uint8), MAPS["corner +++"]).tolist() == [[255] * 3] * 2
    assert apply_map(np.array([[255, 255, 255], [0, 0, 0]], np.uint8), MAPS["corner ---"]).tolist() == [[0] * 3] * 2
    assert apply_grey(every, MAPS["inversion"]).tolist() == (255 - every).tolist() and apply_grey(np.array([3], np.uint8), MAPS["half"]).tolist() == [2]
    for m in MAPS.values():
        assert all(abs(v) <= GAIN for v in m[:9]) and all(abs(v) <= OFFSET for v in m[9:])
    corners = [m for k, m in MAPS.items() if k.startswith("corner")]
    assert len(corners) == 8 and all(abs(v) == GAIN for m in corners for v in m[:9]) and all(abs(v) == OFFSET for m in corners for v in m[9:])


def test_header_stands_alone():
    """g++ takes nhw_colour.h with no HIP header in front of it"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "hip/hip_runtime.h" not in open(HEADER).read()


def _header_struct(text):
    """nhw_colour_map as the header declares it, as a ctypes.Structure: the C layout rules applied to the header's own fields"""
    body = re.search(r"typedef struct nhw_colour_map \{(.*?)\} nhw_colour_map;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            kind, name = decl.split(None, 1)
            dims = [int(v) for v in re.findall(r"\[(\d+)\]", name)]
            t = kinds[kind]
            for d in reversed(dims):
                t = t * d
            fields.append((re.match(r"\w+", name).group(0), t))
    return type("HeaderColourMap", (ctypes.Structure,), {"_fields_": fields})


def test_symbols_prototypes_and_struct():
    lib = load_lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    text = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 4
    for decl in decls:
        assert squeeze(decl) in squeeze(text), decl
    assert re.search(r"^#define NHW_COLOUR_MAX_GAIN\s+16\b", text, re.M) and re.search(r"^#define NHW_COLOUR_MAX_OFFSET\s+4096\b", text, re.M)
    S = _header_struct(text)
    assert ctypes.sizeof(S) == 64 and ctypes.alignment(S) == 4
    assert {n: (getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_} == dict(m=(0, 36), o=(36, 12), reserved=(48, 16))
    import nhwcodec_amd as na
    mine = np.dtype(na.COLOUR_DTYPE)
    assert mine == COLOUR and mine.itemsize == 64
    for n, _ in S._fields_:
        assert getattr(S, n).offset == mine.fields[n][1], n
    assert na.COLOUR_MAX_GAIN == 16 and na.COLOUR_MAX_OFFSET == 4096
    import inspect
    for f in (na.resize_to_tensor_device, na.resize_grey_to_tensor_device, na.warp_to_tensor_device, na.warp_grey_to_tensor_device, na.Decoder.decode_crops_device,
              na.Decoder.decode_crops_grey_device, na.Decoder.decode_warps_device, na.Decoder.decode_warps_grey_device):
        assert inspect.signature(f).parameters["colours"].default is None, f


def test_colour_matrix():
    import nhwcodec_amd as na
    eye = np.eye(3, 4)
    assert np.array_equal(na.colour_matrix(), eye) and na.colour_matrix().dtype == np.float64
    assert np.allclose(na.colour_matrix(saturation=0), [[0.299, 0.587, 0.114, 0]] * 3, rtol=0, atol=1e-15)
    assert np.allclose(na.colour_matrix(contrast=0), [[0, 0, 0, 128]] * 3, rtol=0, atol=1e-12)
    assert np.allclose(na.colour_matrix(contrast=0, centre=100.5), [[0, 0, 0, 100.5]] * 3, rtol=0, atol=1e-12)
    assert np.array_equal(na.colour_matrix(brightness=1.5), 1.5 * eye)
    for h in (0.05, 0.25, -0.4, 0.5):
        assert np.abs(na.colour_compose(na.colour_matrix(hue=h), na.colour_matrix(hue=-h)) - eye).max() < 1e-9, h
    grey = np.array([77.0, 77.0, 77.0, 1.0])
    for kw in (dict(saturation=0.3), dict(saturation=1.8), dict(hue=0.1), dict(hue=-0.37), dict(saturation=0.5, hue=0.2)):
        assert np.abs(na.colour_matrix(**kw) @ grey - 77.0).max() < 1e-9, kw
    y = np.array([0.299, 0.587, 0.114])
    assert np.abs(y @ na.colour_matrix(hue=0.3)[:, :3] - y).max() < 1e-9                       # the turn keeps Y
    # the order: brightness, then contrast, then saturation, then hue
    want = na.colour_compose(na.colour_compose(na.colour_compose(na.colour_matrix(brightness=1.2), na.colour_matrix(contrast=0.7)), na.colour_matrix(saturation=1.4)),
                             na.colour_matrix(hue=0.1))
    assert np.abs(na.colour_matrix(1.2, 0.7, 1.4, 0.1) - want).max() < 1e-12
    assert np.allclose(na.colour_matrix(brightness=2, contrast=0.5)[:, :], np.hstack([np.eye(3), np.full((3, 1), 64.0)]), rtol=0, atol=1e-12)   # 0.5 (2 x) + 64
    a, b = np.arange(12.0).reshape(3, 4) / 7, np.arange(12.0)[::-1].reshape(3, 4) / 5
    x = np.array([3.0, 5.0, 7.0, 1.0])
    assert np.allclose(na.colour_compose(a, b) @ x, b @ np.append(a @ x, 1.0))
    for bad in (dict(hue=float("nan")), dict(brightness=float("inf")), dict(contrast="x"), dict(centre=None)):
        with pytest.raises(na.NhwError):
            na.colour_matrix(**bad)


def test_colour_fixed():
    import nhwcodec_amd as na
    assert na.colour_fixed(np.eye(3, 4)) == MAPS["identity"] and all(type(v) is int for v in na.colour_fixed(np.eye(3, 4)))
    # twelve distinct entries on (R, G, B, 1): the struct's row i makes byte i of B, G, R and its column j reads byte j
    m = np.array([[1, 2, 3, 10], [4, 5, 6, 11], [7, 8, 9, 12]], np.float64)
    assert na.colour_fixed(m) == tuple(ONE * v for v in (9, 8, 7, 6, 5, 4, 3, 2, 1, 12, 11, 10))
    tie = lambda v: na.colour_fixed(np.array([[v, 0, 0, v], [0, 0, 0, 0], [0, 0, 0, 0]]))
    assert (tie(0.5 / ONE)[8], tie(1.5 / ONE)[8], tie(2.5 / ONE)[8], tie(-0.5 / ONE)[8], tie(-1.5 / ONE)[8]) == (0, 2, 2, 0, -2)      # ties to even
    assert (tie(0.5 / ONE)[11], tie(1.5 / ONE)[11], tie(-2.5 / ONE)[11]) == (0, 2, -2)
    at = lambda i, j, v: np.array([[v if (i, j) == (r, c) else 0.0 for c in range(4)] for r in range(3)])
    for i in range(3):
        for j in range(4):
            limit = 16.0 if j < 3 else 4096.0
            for sign in (1, -1):
                assert max(abs(v) for v in na.colour_fixed(at(i, j, sign * limit))) == (GAIN if j < 3 else OFFSET)
                with pytest.raises(na.NhwError):
                    na.colour_fixed(at(i, j, sign * (limit + 1.0 / ONE)))
            for bad in (float("nan"), float("inf"), -float("inf")):
                with pytest.raises(na.NhwError):
                    na.colour_fixed(at(i, j, bad))
    for bad in (np.eye(3), np.eye(4), [1, 2, 3], "x", None, np.eye(3, 4).astype(object)):
        with pytest.raises(na.NhwError):
            na.colour_fixed(bad)
    assert na.colour_fixed(na.colour_matrix(saturation=0))[:3] == MAPS["luma mix"][:3]


def test_python_refusals_before_any_device(monkeypatch):
    """a wrong count, a wrong shape, a map beyond the limits and a NaN raise before a picture, a container or a device is looked at: the
    pictures here are no tensors at all, and the decoder is no decoder"""
    import nhwcodec_amd as na
    fmt, grey = na.TensorFormat("float16", "CHW", "RGB"), na.TensorFormat("float16", "CHW", "GREY")
    eye = np.eye(3, 4)
    nan = eye.copy()
    nan[1, 3] = float("nan")
    colour_bad = ([eye], [eye, eye, eye], [eye, np.eye(3)], [eye, 17 * eye], [eye, nan], [eye, (1.0, 0.0)], eye, "xx", [eye, list(range(11))],
                  [eye, np.array([GAIN + 1] + [0] * 11)], [eye, np.array([0] * 9 + [0, -OFFSET - 1, 0])])
    grey_bad = ([(1, 0)], [(1, 0), (1, 0), (1, 0)], [(1, 0), (16.001, 0)], [(1, 0), (1, -4096.5)], [(1, 0), (float("nan"), 0)], [(1, 0), (1, float("inf"))], [(1, 0), eye], [(1, 0), (1, 2, 3)])
    pics = ["no tensor", "no tensor"]
    mats = [[[1, 0, 0], [0, 1, 0]]] * 2
    dec = na.Decoder.__new__(na.Decoder)                               # no handle, no device: the refusals come first
    crops = [(0, 0, 0, 8, 8), (0, 1, 1, 8, 8)]
    for bad in colour_bad:
        with pytest.raises(na.NhwError, match="colour|`colours`"):
            na.resize_to_tensor_device(pics, (4, 4), fmt, colours=bad)
        with pytest.raises(na.NhwError, match="colour|`colours`"):
            na.warp_to_tensor_device(pics, mats, (4, 4), fmt, colours=bad)
        with pytest.raises(na.NhwError, match="colour|`colours`"):
            dec.decode_crops_device(["no container"], crops, (4, 4), fmt, colours=bad)
        with pytest.raises(na.NhwError, match="colour|`colours`"):
            dec.decode_warps_device(["no container"], [0, 0], mats, (4, 4), fmt, colours=bad)
    for bad in grey_bad:
        with pytest.raises(na.NhwError, match="colour|`colours`|grey"):
            na.resize_grey_to_tensor_device(pics, (4, 4), grey, colours=bad)
        with pytest.raises(na.NhwError, match="colour|`colours`|grey"):
            na.warp_grey_to_tensor_device(pics, mats, (4, 4), grey, colours=bad)
        with pytest.raises(na.NhwError, match="colour|`colours`|grey"):
            dec.decode_crops_grey_device(["no container"], crops, (4, 4), grey, colours=bad)
        with pytest.raises(na.NhwError, match="colour|`colours`|grey"):
            dec.decode_warps_grey_device(["no container"], [0, 0], mats, (4, 4), grey, colours=bad)
    t = na._colour_table([eye, np.array(MAPS["minus half"])], 2, "test")
    assert t.dtype == COLOUR and t["m"][0].tolist() == np.array(MAPS["identity"][:9]).reshape(3, 3).tolist() and t["o"][1].tolist() == [200 * ONE] * 3 and not t["reserved"].any()
    g = na._colour_table([(1.5, -64), (-0.5, 200.25)], 2, "test", channels=1)
    assert g["m"][:, 0, 0].tolist() == [3 * ONE // 2, -ONE // 2] and g["o"][:, 0].tolist() == [-64 * ONE, 200 * ONE + ONE // 4] and g["m"].reshape(2, 9)[:, 1:].any() == False  # noqa: E712
