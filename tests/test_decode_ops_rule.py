"""Per-sample flip, colour map and tone table in the full-file decode without a GPU: the two entries as the header
declares them, as the library exports them and as the Python face offers them; the packed-dword pixel reversal and the destination column
rule of nhwcodec_amd/csrc/nhw_reverse.h held by a stand-alone program (tests/decode_ops/check.cpp, plain and under AddressSanitizer + UBSan;
nothing is preloaded) against a reversal written a second way; the keywords' refusals before any device is touched; and the numpy model of
tests/decode_ops_cases.py on hand-worked values."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import colour_cases, tone_cases
from tests.decode_ops_cases import FLAGS, FORMATS8, GREY_FORMATS, SYMBOLS, maps_for, python_colours, python_tones, tables_for
from tests.nhw_surgery import can_sanitize
from tests.support import ROOT, load_lib

CSRC = os.path.join(ROOT, "nhwcodec_amd", "csrc")
HEADER = os.path.join(CSRC, "nhw_reverse.h")
PROTOTYPES = """
int nhw_dec_batch_device_tensor_ops(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale,
                                    const nhw_tensor_format *fmt, const uint8_t *d_flags, const nhw_colour_map *d_maps,
                                    const nhw_tone_table *d_tones, void *d_out, int32_t *d_status, int32_t *d_quality, void *stream);
int nhw_dec_batch_device_grey_ops(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale,
                                  const nhw_tensor_format *fmt, const uint8_t *d_flags, const nhw_colour_map *d_maps,
                                  const nhw_tone_table *d_tones, void *d_out, int32_t *d_status, int32_t *d_quality, void *stream);
"""


def test_header_library_and_python_have_the_entries():
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    text = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 2
    for decl in decls:
        assert squeeze(decl) in squeeze(text), decl
    lib = load_lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    plain = lib.nhw_dec_batch_device_tensor.argtypes
    for name in SYMBOLS:
        a = getattr(lib, name).argtypes
        assert len(a) == len(plain) + 3 and list(a[:7]) == list(plain[:7]) and list(a[10:]) == list(plain[7:]), name
    import nhwcodec_amd as na
    for f in (na.Decoder.decode_tensor_device, na.Decoder.decode_grey_device):
        p = inspect.signature(f).parameters
        for k in ("flips", "colours", "tones"):
            assert k in p and p[k].default is None, (f, k)
        assert "mirror, colour map, tone table" in re.sub(r"\s+", " ", f.__doc__) or "mirror, map, table" in re.sub(r"\s+", " ", f.__doc__)


def test_the_rule_reads_the_same_in_header_and_design():
    """the four steps, in their order, in both texts"""
    for path, start in ((os.path.join(ROOT, "include", "nhw_hip.h"), "(DESIGN.md section 28) ----"), (os.path.join(ROOT, "DESIGN.md"), "\n## 28. ")):
        text = open(path).read()
        assert text.count(start) == 1, (path, start)
        text = re.sub(r"[\s*`]+", " ", text[text.index(start):])
        at = [text.find(s) for s in ("c' = S - 1 - c", "nhw_colour_apply<3>(d_maps[i], b)", "nhw_tone_apply<3>(d_tones[i].t, b)", "value rule, channel order, layout and row rule")]
        assert all(a >= 0 for a in at) and at == sorted(at), (path, at)


def _build_check(tmp_path, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1"] if sanitize else ["-O2"]
    obj, exe = str(tmp_path / "check.o"), str(tmp_path / "decode_ops_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-c", os.path.join(ROOT, "tests", "decode_ops", "check.cpp"), "-o", obj])
    subprocess.check_call(["g++", *flags, obj, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_reversal_and_column_rule(tmp_path, sanitize):
    if sanitize and not can_sanitize():
        pytest.skip("this machine's compiler cannot link and run a sanitized program")
    p = subprocess.run([_build_check(tmp_path, sanitize)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    assert "reversals 148\n" in p.stdout and "pieces 392\n" in p.stdout and "mismatches 0\n" in p.stdout, p.stdout[-2000:]


def test_header_stands_alone():
    """g++ takes nhw_reverse.h with no HIP header in front of it"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "hip/hip_runtime.h" not in open(HEADER).read()


def test_the_cases_hold_what_they_should():
    """every enum value in the eight formats, the byte format among them; both thread shapes mirrored; different maps and tables a file, a
    clamping corner among the maps"""
    for k, values in enumerate((("uint8", "float16", "bfloat16", "float32"), ("HWC", "CHW"), ("BGR", "RGB"), ("file", "reversed"))):
        assert {f[k] for f in FORMATS8} == set(values)
    assert len({f[:2] for f in FORMATS8}) == 8 and FORMATS8[0] == ("uint8", "HWC", "BGR", "file")
    assert GREY_FORMATS[0] is None and {f[0] for f in GREY_FORMATS[1:]} == {"uint8", "float16", "bfloat16", "float32"}
    assert {f[0] for f in FLAGS} == {0, 1} and {f[1] for f in FLAGS} == {0, 1}
    corners = {m for k, m in colour_cases.MAPS.items() if k.startswith("corner")}
    for first in (0, 3):
        m = maps_for(3, first)
        assert len(set(m)) == 3 and corners & set(m)
    t = tables_for(3, 1)
    assert len({x.tobytes() for x in t}) == 3 and all(x.shape == (3, 256) and x.dtype == np.uint8 for x in t)
    assert np.array_equal(python_tones(t)[1], t[1][::-1]) and np.array_equal(python_tones(t, grey=True)[2], t[2][0])
    assert python_colours(m)[2].tolist() == list(m[2])


def test_the_numpy_model_on_hand_worked_values():
    """mirror, then map, then table: a 1 x 2 picture through each order-sensitive pair"""
    px = np.array([[[10, 20, 30], [200, 100, 0]]], np.uint8)
    flipped = px[:, ::-1]
    assert flipped.tolist() == [[[200, 100, 0], [10, 20, 30]]]
    rot = colour_cases.apply_map(flipped, colour_cases.MAPS["rotation"])            # B <- G, G <- R, R <- B
    assert rot.tolist() == [[[100, 0, 200], [20, 30, 10]]]
    consts = tone_cases.TABLES["constants"]
    assert tone_cases.apply_tone(rot, consts).tolist() == [[[3, 141, 250]] * 2]
    post = tone_cases.TABLES["posterize 1"]
    assert tone_cases.apply_tone(rot, post).tolist() == [[[0, 0, 128], [0, 0, 0]]]
    # the table acts BEHIND the map: posterize(contrast(x)) is not contrast(posterize(x))
    x = np.array([[[120, 120, 120]]], np.uint8)
    con = colour_cases.MAPS["contrast"]                                              # 1.5 x - 64: 120 -> 116
    assert tone_cases.apply_tone(colour_cases.apply_map(x, con), post).tolist() == [[[0, 0, 0]]]
    assert colour_cases.apply_map(tone_cases.apply_tone(np.array([[[130, 130, 130]]], np.uint8), post), con).tolist() == [[[128, 128, 128]]]
    assert colour_cases.apply_grey(np.array([3], np.uint8), colour_cases.MAPS["half"]).tolist() == [2]
    assert tone_cases.apply_tone_grey(np.array([5], np.uint8), consts).tolist() == [3]


def test_python_refusals_before_any_device():
    """wrong lengths, a map beyond the limits and a malformed tone table raise before a file, a device or the library is looked at: the arena is
    no tensor, and the decoder is no decoder"""
    import nhwcodec_amd as na
    fmt, grey = na.TensorFormat("float16", "CHW", "RGB"), na.TensorFormat("float16", "CHW", "GREY")
    dec = na.Decoder.__new__(na.Decoder)                               # no handle, no device: the refusals come first
    files = ("no arena", "no offsets", np.zeros(2, np.int32))          # two files, by the lengths' shape
    eye, ident = np.eye(3, 4), na.tone_identity()
    nan = eye.copy()
    nan[0, 0] = float("nan")
    G, O = colour_cases.GAIN, colour_cases.OFFSET
    bad_flips = ([True], [0, 1, 0], [0.5, 0.5], "ab", [[0, 1]])
    bad_colours = ([eye], [eye, eye, eye], 17 * eye, [eye, 17 * eye], nan, [eye, nan], np.eye(3), "xx", [eye, list(range(11))], np.array([G + 1] + [0] * 11),
                   [eye, np.array([0] * 9 + [0, -O - 1, 0])], (1.0, 0.0))
    bad_tones = ([ident], [ident] * 3, [ident, ident[:2]], [ident, ident.astype(np.float64)], [ident, ident.astype(np.int64) + 1], ident, "x", [ident, np.arange(256)])
    for bad in bad_flips:
        with pytest.raises(na.NhwError, match="flips"):
            dec.decode_tensor_device(*files, fmt, flips=bad)
        with pytest.raises(na.NhwError, match="flips"):
            dec.decode_grey_device(*files, fmt=grey, flips=bad)
    for bad in bad_colours:
        with pytest.raises(na.NhwError, match="colour|`colours`"):
            dec.decode_tensor_device(*files, fmt, colours=bad)
    for bad in ([(1, 0)], [(1, 0)] * 3, (16.001, 0), [(1, 0), (1, -4096.5)], (float("nan"), 0), [(1, 0), eye], eye, [(1, 0), (1, 2, 3)]):
        with pytest.raises(na.NhwError, match="colour|`colours`|grey"):
            dec.decode_grey_device(*files, colours=bad)
    for bad in bad_tones:
        with pytest.raises(na.NhwError, match="tone"):
            dec.decode_tensor_device(*files, fmt, tones=bad)
    for bad in ([ident[0]], [ident[0]] * 3, [ident[0], ident], [ident[0], ident[0].astype(np.int64) - 1], "x"):
        with pytest.raises(na.NhwError, match="tone"):
            dec.decode_grey_device(*files, fmt=grey, tones=bad)
    # what passes: one map for all files or one a file, in either spelling
    f, m, t = na._decode_ops(2, [True, False], eye, [ident, ident[::-1]], "test")
    assert f.tolist() == [1, 0] and m.dtype == colour_cases.COLOUR and len(m) == 2 and m["m"][1].tolist() == m["m"][0].tolist() == (np.eye(3, dtype=np.int64) * colour_cases.ONE).tolist()
    assert t.shape == (2, 768) and np.array_equal(t[0], na.tone_fixed(ident))
    _, m, _ = na._decode_ops(2, None, np.array(colour_cases.MAPS["minus half"]), None, "test")
    assert m["o"].tolist() == [[200 * colour_cases.ONE] * 3] * 2
    _, m, _ = na._decode_ops(2, None, [np.array(colour_cases.MAPS["half"]), eye], None, "test")
    assert m["m"][0][0][0] == colour_cases.ONE // 2 and m["m"][1][0][0] == colour_cases.ONE
    _, g, gt = na._decode_ops(2, None, (1.5, -64), [ident[0], ident[0][::-1]], "test", channels=1)
    assert g["m"][:, 0, 0].tolist() == [3 * colour_cases.ONE // 2] * 2 and g["o"][:, 0].tolist() == [-64 * colour_cases.ONE] * 2
    assert gt.shape == (2, 768) and gt[1, :256].tolist() == list(range(255, -1, -1)) and not gt[:, 256:].any()
    assert na._decode_ops(2, None, None, None, "test") == (None, None, None)
