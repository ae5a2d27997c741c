"""The tone table's rules without a GPU: nhw_tone_equalize, nhw_tone_autocontrast and nhw_tone_apply of
nhwcodec_amd/csrc/nhw_tone.h held by a stand-alone program (tests/tone/check.cpp, plain and under AddressSanitizer + UBSan; nothing is preloaded)
against a straightforward 128-bit model on the crafted histograms of tone_cases.HISTS and on seeded random ones, and the rows it prints against
tone_cases' numpy restatement; the header alone; the Python builders against hand-written tables; the `tones` keyword's refusals before any
device is touched; the exported symbols, their prototypes and the struct as the header declares it."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests.nhw_surgery import can_sanitize
from tests.support import ROOT, load_lib
from tests.tone_cases import HISTS, SYMBOLS, TABLES, apply_tone, apply_tone_grey, autocontrast_row, equalize_row, hists_text, random_hists

CSRC = os.path.join(ROOT, "nhwcodec_amd", "csrc")
HEADER = os.path.join(CSRC, "nhw_tone.h")
PROTOTYPES = """
int nhw_resample_toned_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, int filter, const nhw_tensor_format *fmt,
                                        const uint8_t *d_flags, const nhw_colour_map *d_maps, const nhw_tone_table *d_tones, const uint64_t *d_out_addr, void *stream);
int nhw_warp_toned_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                                    const nhw_warp *d_warps, const nhw_colour_map *d_maps, const nhw_tone_table *d_tones, const uint64_t *d_out_addr, void *stream);
int nhw_dec_crops_toned_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                  uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const uint8_t *flags, const nhw_colour_map *maps,
                                  const nhw_tone_table *tones, const uint64_t *dst_addr, int32_t *status, int filter);
int nhw_dec_warps_toned_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                                  uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const nhw_colour_map *maps,
                                  const nhw_tone_table *tones, const uint64_t *dst_addr, int32_t *status);
int nhw_hist_device(const nhw_picture *d_pics, int n, int channels, uint32_t *d_hist, void *stream);
int nhw_tone_from_hist_device(const uint32_t *d_hist, int n, int channels, const uint8_t *d_ops, nhw_tone_table *d_tones, void *stream);
"""


def _build_check(tmp_path, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1"] if sanitize else ["-O2"]
    obj, exe = str(tmp_path / "check.o"), str(tmp_path / "tone_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-c", os.path.join(ROOT, "tests", "tone", "check.cpp"), "-o", obj])
    subprocess.check_call(["g++", *flags, obj, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_rules_match_the_model_and_the_numpy_restatement(tmp_path, sanitize):
    if sanitize and not can_sanitize():
        pytest.skip("this machine's compiler cannot link and run a sanitized program")
    hists = list(HISTS.values()) + random_hists(40, 2502)
    text = tmp_path / "hists.txt"
    text.write_text(hists_text(hists))
    p = subprocess.run([_build_check(tmp_path, sanitize), str(text)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-2000:]
    assert f"file {len(hists)}\n" in p.stdout and "random 400\n" in p.stdout and "mismatches 0\n" in p.stdout, p.stdout[-300:]
    rows = [(kind, np.frombuffer(bytes.fromhex(digits), np.uint8)) for kind, digits in re.findall(r"^(eq|ac) ([0-9a-f]{512})$", p.stdout, re.M)]
    assert len(rows) == 2 * len(hists)
    names = list(HISTS) + [f"random {i}" for i in range(40)]
    for i, h in enumerate(hists):
        assert rows[2 * i][0] == "eq" and np.array_equal(rows[2 * i][1], equalize_row(h)), names[i]
        assert rows[2 * i + 1][0] == "ac" and np.array_equal(rows[2 * i + 1][1], autocontrast_row(h)), names[i]


def test_the_numpy_restatement_on_hand_worked_histograms():
    """tone_cases' two rules agree with the rule's words where a row can be written down"""
    ident = np.arange(256, dtype=np.uint8)
    for name in ("empty", "one bin", "one bin at 0", "total - last = 254", "one bin of 65535^2"):
        assert np.array_equal(equalize_row(HISTS[name]), ident), name          # step 0
    for name in ("empty", "one bin", "one bin at 0", "one bin of 65535^2"):
        assert np.array_equal(autocontrast_row(HISTS[name]), ident), name      # lo >= hi, or nothing counted
    # flat, 100 a bin: step = 25500 / 255 = 100, row[x] = (100 x + 50) / 100 = x
    assert np.array_equal(equalize_row(HISTS["flat"]), ident) and np.array_equal(autocontrast_row(HISTS["flat"]), ident)
    # step exactly 1: bins 0 .. 254 hold 1 each: row[x] = x
    assert np.array_equal(equalize_row(HISTS["step exactly 1"]), ident)
    # two bins at 0 and 255, 40000 and 60000: step = 40000 / 255 = 156; row[0] = 0, every other x has 40000 in front: (40000 + 78) / 156 = 256 -> 255
    eq = equalize_row(HISTS["two bins at 0 and 255"])
    assert eq[0] == 0 and (eq[1:] == 255).all()
    # two adjacent bins 100 (300) and 101 (700): step = 1; nothing in front up to 100, 300 in front of 101, 1000 beyond
    eq = equalize_row(HISTS["two adjacent bins"])
    assert (eq[:101] == 0).all() and (eq[101:] == 255).all()
    ac = autocontrast_row(HISTS["two adjacent bins"])
    assert (ac[:101] == 0).all() and (ac[101:] == 255).all()
    # a narrow band 90 .. 140: floor(255 (x - 90) / 50)
    ac = autocontrast_row(HISTS["a narrow band"])
    assert ac[89] == 0 and ac[90] == 0 and ac[91] == 5 and ac[100] == 51 and ac[115] == 127 and ac[139] == 249 and ac[140] == 255 and ac[255] == 255
    # the running sum plus step / 2 above 2^32: the last entry still comes out as (2^32 - 1001 + 8421502) / 16843005 = 255
    h = HISTS["2^32 - 1 spread"]
    step = (int(h.sum()) - 1000) // 255
    assert step == 16843005 and int(h[:255].sum()) + step // 2 >= 1 << 32 and equalize_row(h)[255] == 255 and equalize_row(h)[128] == (128 * 16843005 + 127 + step // 2) // step


def test_header_stands_alone():
    """g++ takes nhw_tone.h with no HIP header in front of it, under -Wall -Wextra -Werror"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-x", "c++", HEADER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    text = open(HEADER).read()
    assert "hip/hip_runtime.h" not in text and "float32" in text                # (the note on torchvision's autocontrast)


def test_symbols_prototypes_and_struct():
    lib = load_lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    text = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 6
    for decl in decls:
        assert squeeze(decl) in squeeze(text), decl
    m = re.search(r"typedef struct nhw_tone_table \{\s*uint8_t t\[(\d+)\]\[(\d+)\];\s*\} nhw_tone_table;", text)
    assert m and int(m.group(1)) * int(m.group(2)) == 768 and (int(m.group(1)), int(m.group(2))) == (3, 256)      # sizeof: bytes only, no padding
    for name, value in (("KEEP", 0), ("EQUALIZE", 1), ("AUTOCONTRAST", 2)):
        assert re.search(rf"^#define NHW_TONE_{name}\s+{value}\b", text, re.M), name
    import nhwcodec_amd as na
    assert na.TONE_OPS == {"keep": 0, "equalize": 1, "autocontrast": 2}
    for f in (na.resize_to_tensor_device, na.resize_grey_to_tensor_device, na.warp_to_tensor_device, na.warp_grey_to_tensor_device, na.Decoder.decode_crops_device,
              na.Decoder.decode_crops_grey_device, na.Decoder.decode_warps_device, na.Decoder.decode_warps_grey_device):
        assert inspect.signature(f).parameters["tones"].default is None, f
    assert "hist_device" in na.tone_from_hist_device.__doc__ and "resize_to_tensor_device" in na.tone_from_hist_device.__doc__     # the Equalize recipe


def test_builders_against_hand_written_tables():
    import nhwcodec_amd as na
    x = np.arange(256)
    ident = np.tile(x.astype(np.uint8), (3, 1))
    t = na.tone_identity()
    assert t.dtype == np.uint8 and t.shape == (3, 256) and np.array_equal(t, ident)
    # posterize: bits 0 keeps nothing, 1 the top bit, 4 the top nibble, 8 everything
    assert not na.tone_posterize(0).any() and np.array_equal(na.tone_posterize(8), ident)
    assert np.array_equal(na.tone_posterize(1)[1], np.where(x < 128, 0, 128)) and np.array_equal(na.tone_posterize(4)[2], x // 16 * 16)
    p = na.tone_posterize((0, 4, 8))
    assert p.dtype == np.uint8 and not p[0].any() and np.array_equal(p[1], x // 16 * 16) and np.array_equal(p[2], x)
    # solarize: 0 inverts everything, 1 all but 0, 128 the upper half, 255 the last byte alone, 256 nothing
    assert np.array_equal(na.tone_solarize(0), 255 - ident) and np.array_equal(na.tone_solarize(256), ident)
    assert na.tone_solarize(1)[0].tolist() == [0] + list(range(254, -1, -1))
    assert na.tone_solarize(128)[0].tolist() == list(range(128)) + list(range(127, -1, -1))
    assert na.tone_solarize(255)[0].tolist() == list(range(255)) + [0]
    assert np.array_equal(na.tone_solarize((0, 256, 128))[1], x)
    # gamma: 1 is the identity; 0.5: 255 sqrt(x / 255); 2.2 on stated entries
    assert np.array_equal(na.tone_gamma(1.0), ident)
    g = na.tone_gamma(0.5)[0]
    assert (g[0], g[1], g[64], g[128], g[255]) == (0, 16, 128, 181, 255)         # sqrt(255) = 15.97, sqrt(255 x 64) = 127.75, sqrt(255 x 128) = 180.67
    g = na.tone_gamma(2.2)[2]
    assert (g[0], g[16], g[64], g[128], g[192], g[254], g[255]) == (0, 1, 12, 56, 137, 253, 255)
    assert na.tone_gamma(1.0, gain=2.0)[0].tolist() == [min(2 * v, 255) for v in range(256)]
    assert np.array_equal(na.tone_gamma((1.0, 0.5, 1.0), (1.0, 1.0, 0.0)), np.stack([x, na.tone_gamma(0.5)[0], 0 * x]))
    # affine: halves go up at either sign
    assert na.tone_affine(0.5, 0)[0][[1, 2, 3, 255]].tolist() == [1, 1, 2, 128]
    assert na.tone_affine(-0.5, 200)[0][[0, 1, 2, 3]].tolist() == [200, 200, 199, 199]   # 199.5 -> 200, 198.5 -> 199
    assert na.tone_affine(-0.5, 1)[0][[1, 2, 3, 5]].tolist() == [1, 0, 0, 0]              # 0.5 -> 1, -0.5 -> 0 (clamped from floor(0) = 0), -1.5 -> -1 -> 0
    assert na.tone_affine(2, -100)[1].tolist() == [min(max(2 * v - 100, 0), 255) for v in range(256)]
    assert np.array_equal(na.tone_affine((1, 0, -1), (0, 7, 255)), np.stack([x, 0 * x + 7, 255 - x]))
    # compose on two permutations: then[first[x]], a channel at a time
    rng = np.random.default_rng(7)
    a, b = (np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8) for _ in range(2))
    c = na.tone_compose(a, b)
    for ch in range(3):
        for v in (0, 1, 100, 255):
            assert c[ch][v] == b[ch][a[ch][v]]
    assert not np.array_equal(c, na.tone_compose(b, a)) and c.dtype == np.uint8
    # fixed: the struct's rows are B, G, R
    rows = np.stack([np.full(256, 10), x, 255 - x]).astype(np.uint8)           # R, G, B
    f = na.tone_fixed(rows)
    assert f.dtype == np.uint8 and f.shape == (768,) and np.array_equal(f[:256], 255 - x) and np.array_equal(f[256:512], x) and (f[512:] == 10).all()


def test_builders_refuse():
    import nhwcodec_amd as na
    nan, inf = float("nan"), float("inf")
    for call, bads in ((na.tone_posterize, (-1, 9, 1.5, nan, "x", None, True, (1, 2), (1, 2, 9))),
                       (na.tone_solarize, (-1, 257, nan, inf, "x", None, (1, 2), (1, nan, 3))),
                       (na.tone_gamma, (-0.1, 1001, nan, inf, "x", None, (1, 2))),
                       (lambda v: na.tone_gamma(1.0, v), (-1, nan, inf, "x", (1, 2))),
                       (lambda v: na.tone_affine(v, 0), (nan, inf, -inf, "x", None, 1e9, (1, 2))),
                       (lambda v: na.tone_affine(1, v), (nan, inf, "x", (1, nan, 2)))):
        for bad in bads:
            with pytest.raises(na.NhwError):
                call(bad)
    ident = na.tone_identity()
    for bad in (ident[:2], ident.astype(np.float64), ident.astype(np.int64) + 1, ident.astype(np.int64) - 1, ident.T, "x", None, [1, 2, 3]):
        with pytest.raises(na.NhwError):
            na.tone_fixed(bad)
        with pytest.raises(na.NhwError):
            na.tone_compose(ident, bad)
        with pytest.raises(na.NhwError):
            na.tone_compose(bad, ident)


def test_python_refusals_before_any_device():
    """a wrong count, a wrong shape and a value out of range raise before a picture, a container or a device is looked at: the pictures here are
    no tensors at all, and the decoder is no decoder"""
    import nhwcodec_amd as na
    fmt, grey = na.TensorFormat("float16", "CHW", "RGB"), na.TensorFormat("float16", "CHW", "GREY")
    t = na.tone_identity()
    row = t[0]
    colour_bad = ([t], [t, t, t], [t, row], [t, t.astype(np.float32)], [t, t.astype(np.int32) + 1], t[0], "xx", [t, None], 5)
    grey_bad = ([row], [row, row, row], [row, t], [row, row[:255]], [row, row.astype(np.float64)], [row, row.astype(np.int16) - 1], "xx", 7)
    pics = ["no tensor", "no tensor"]
    mats = [[[1, 0, 0], [0, 1, 0]]] * 2
    dec = na.Decoder.__new__(na.Decoder)                               # no handle, no device: the refusals come first
    crops = [(0, 0, 0, 8, 8), (0, 1, 1, 8, 8)]
    for bad in colour_bad:
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            na.resize_to_tensor_device(pics, (4, 4), fmt, tones=bad)
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            na.warp_to_tensor_device(pics, mats, (4, 4), fmt, tones=bad)
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            dec.decode_crops_device(["no container"], crops, (4, 4), fmt, tones=bad)
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            dec.decode_warps_device(["no container"], [0, 0], mats, (4, 4), fmt, tones=bad)
    for bad in grey_bad:
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            na.resize_grey_to_tensor_device(pics, (4, 4), grey, tones=bad)
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            na.warp_grey_to_tensor_device(pics, mats, (4, 4), grey, tones=bad)
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            dec.decode_crops_grey_device(["no container"], crops, (4, 4), grey, tones=bad)
        with pytest.raises(na.NhwError, match="tone|`tones`"):
            dec.decode_warps_grey_device(["no container"], [0, 0], mats, (4, 4), grey, tones=bad)
    # a good table with colours that are not: the colours' refusal still comes, and first
    with pytest.raises(na.NhwError, match="colour|`colours`"):
        na.resize_to_tensor_device(pics, (4, 4), fmt, colours=[np.eye(3)], tones=[t, t])
    with pytest.raises(na.NhwError):
        na.hist_device("no list")
    with pytest.raises(na.NhwError):
        na.hist_device([])
    with pytest.raises(na.NhwError):
        na.hist_device(["no tensor"])
    # the host table of a call: rows exchanged into the struct's order, the grey row in front
    rows = np.stack([np.full(256, 1), np.full(256, 2), np.full(256, 3)]).astype(np.uint8)
    a = na._tone_arg([rows, t], 2, "test")
    assert a.dtype == np.uint8 and a.shape == (2, 768) and a[0].reshape(3, 256)[:, 0].tolist() == [3, 2, 1] and np.array_equal(a[1], t.reshape(768))
    g = na._tone_arg([255 - row], 1, "test", channels=1)
    assert g.shape == (1, 768) and np.array_equal(g[0, :256], 255 - row) and not g[0, 256:].any()


def test_the_tables_and_the_numpy_rule():
    """the tables hold what the tests say of them, and the gather the GPU tests use reads row c for byte c"""
    assert len(TABLES) == 5 and all(t.shape == (3, 256) and t.dtype == np.uint8 for t in TABLES.values())
    p = TABLES["permutations"]
    assert all(sorted(p[c].tolist()) == list(range(256)) for c in range(3)) and len({p[c].tobytes() for c in range(3)}) == 3
    px = np.array([[0, 1, 2], [255, 128, 7]], np.uint8)
    assert apply_tone(px, p).tolist() == [[p[0][0], p[1][1], p[2][2]], [p[0][255], p[1][128], p[2][7]]]
    assert apply_tone(px, TABLES["constants"]).tolist() == [[3, 141, 250]] * 2
    assert apply_tone_grey(px, TABLES["constants"]).tolist() == [[3, 3, 3]] * 2
    assert apply_tone(px, TABLES["posterize 1"]).tolist() == [[0, 0, 0], [128, 128, 0]]
