"""Affine warps into tensors: the rule, the kernel k_warp_to_tensor behind nhw_warp_to_tensor_device, the host call
nhw_dec_warps_to_device and the Python layer (warp_fixed, warp_scale, warp_window, crop_warp, warp_to_tensor_device,
Decoder.decode_warps_device).  The rule -- two taps a direction at a position that an integer matrix gives, a border colour or the nearest edge
pixel outside the picture -- is stated here in numpy's int64 with arithmetic shifts, straight from include/nhw_hip.h, and held against torch's
CPU grid_sample in float64 as an outside yardstick.  Every comparison with the product is exact: bytes for uint8, bit patterns for the floats."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests.picture_cases import SIZES, Rect, World, expected_stats, make_container, parse_container, selected
from tests.support import CANARY, ROOT, load_lib
from tests.tensor_cases import ALL_FORMATS, expected_tensor, tensor_bits

NEW_SYMBOLS = ("nhw_warp_to_tensor_device", "nhw_dec_warps_to_device")
PROTOTYPES = """
int nhw_warp_to_tensor_device(const nhw_picture *d_pics, int n, uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt,
                              const nhw_warp *d_warps, const uint64_t *d_out_addr, void *stream);
int nhw_dec_warps_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                            uint32_t out_width, uint32_t out_height, const nhw_tensor_format *fmt, const nhw_warp *warps, const uint64_t *dst_addr,
                            int32_t *status);
"""
DEFINES = {"NHW_WARP_REPLICATE": 1, "NHW_WARP_MAX_STEP": 64}
NHW_E_ARG, NHW_E_FORMAT = -4, -6
STEP, OFFSET = 1 << 22, 1 << 40                                     # the limits of a step and of an offset
GUARD = 4096                                                        # canary bytes kept in front of and behind a batch
SCALES = (1, 2, 4)
BIG, SMALL = 2, 1                                                   # 1023 x 1025: a 2 x 3 grid of tiles, odd sides; 500 x 375: smaller than a tile
WARP = np.dtype([("c", "<i8"), ("f", "<i8"), ("a", "<i4"), ("b", "<i4"), ("d", "<i4"), ("e", "<i4"), ("fill", "u1", (3,)), ("flags", "u1"), ("reserved", "<u4")])

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
NEGATIVE = dict(scale=(-1 / 255, -0.5, -2.0), bias=(1.0, 127.5, 3.25))
BYTES = ("uint8", "HWC", "BGR", "file")
HALF = ("float16", "CHW", "RGB", "reversed")
FILLS = ((0, 0, 0), (9, 8, 7), (255, 1, 128))


def _fmt(dtype, layout, channels, rows, k=0):
    """the TensorFormat of a parameter tuple; the float types take the ImageNet constants and a set with negative scales in turn"""
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, channels, rows)
    return na.TensorFormat(dtype, layout, channels, rows, **(IMAGENET, NEGATIVE)[k % 2])


# ---------------------------------------------------------------- the rule, in the test's own words
def fixed(M):
    """[[A, B, C], [D, E, F]] -> (a, b, c, d, e, f): 65536 times the entry, the offsets less a half pixel, rounded to nearest even in float64"""
    M = np.asarray(M, dtype=np.float64)
    return tuple(int(np.rint(v * 65536.0)) for v in (M[0, 0], M[0, 1], M[0, 2] - 0.5, M[1, 0], M[1, 1], M[1, 2] - 0.5))


def positions(six, out_w, out_h, xs=None, ys=None):
    """(ix, fx, iy, fy) of every output pixel, int64 [out_h, out_w] -- or of the columns xs and the rows ys alone"""
    a, b, c, d, e, f = (np.int64(v) for v in six)
    xs, ys = np.arange(out_w) if xs is None else np.asarray(xs), np.arange(out_h) if ys is None else np.asarray(ys)
    tx, ty = 2 * xs.astype(np.int64)[None, :] + 1, 2 * ys.astype(np.int64)[:, None] + 1
    SX, SY = ((a * tx + b * ty) >> 1) + c, ((d * tx + e * ty) >> 1) + f
    X8, Y8 = (SX + 128) >> 8, (SY + 128) >> 8
    return X8 >> 8, X8 & 255, Y8 >> 8, Y8 & 255


def rule(P, out_w, out_h, six, fill=(0, 0, 0), replicate=False):
    """P uint8 [h, w, 3] -> uint8 [out_h, out_w, 3] under the rule of section 21"""
    h, w = P.shape[:2]
    assert 1 <= w <= 65535 and 1 <= h <= 65535 and 1 <= out_w <= 4096 and 1 <= out_h <= 4096
    assert all(abs(v) <= STEP for v in (six[0], six[1], six[3], six[4])) and abs(six[2]) <= OFFSET and abs(six[5]) <= OFFSET
    ix, fx, iy, fy = positions(six, out_w, out_h)
    border = np.array(fill, np.int64)

    def tap(y, x):
        v = P[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        if replicate:
            return v
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)                # judged from the index alone, whatever the weight
        return np.where(inside[..., None], v, border)

    S = (((256 - fx) * (256 - fy))[..., None] * tap(iy, ix) + (fx * (256 - fy))[..., None] * tap(iy, ix + 1)
         + ((256 - fx) * fy)[..., None] * tap(iy + 1, ix) + (fx * fy)[..., None] * tap(iy + 1, ix + 1))
    R = (S + 32768) >> 16
    assert R.min() >= 0 and R.max() <= 255
    return R.astype(np.uint8)


def centred(w, h, out_w, out_h, angle=0.0, zoom=1.0, shear=(0.0, 0.0), shift=(0.0, 0.0)):
    """the matrix that lays the output's centre on the w x h source's centre (moved by `shift`), turned by `angle`, a step of `zoom` source
    pixels an output pixel, sheared"""
    L = zoom * np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]]) @ np.array([[1.0, shear[0]], [shear[1], 1.0]])
    t = np.array([w / 2 + shift[0], h / 2 + shift[1]]) - L @ np.array([out_w / 2, out_h / 2])
    return np.concatenate([L, t[:, None]], axis=1)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


# ---------------------------------------------------------------- without a GPU
def _header_struct(text):
    """nhw_warp as the header declares it, as a ctypes.Structure: the C layout rules applied to the header's own fields"""
    body = re.search(r"typedef struct nhw_warp \{(.*?)\} nhw_warp;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            kind, names = decl.split(None, 1)
            for name in (n.strip() for n in names.split(",")):
                m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
                fields.append((m.group(1), kinds[kind] * int(m.group(2))) if m else (name, kinds[kind]))
    return type("HeaderWarp", (ctypes.Structure,), {"_fields_": fields})


def test_warp_symbols_prototypes_and_struct(lib):
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
    S = _header_struct(text)
    assert ctypes.sizeof(S) == 40 and ctypes.alignment(S) == 8
    assert [n for n, _ in S._fields_] == ["c", "f", "a", "b", "d", "e", "fill", "flags", "reserved"]
    mine = np.dtype(na.WARP_DTYPE)
    assert mine == WARP and mine.itemsize == 40
    for name, kind in S._fields_:
        assert getattr(S, name).offset == mine.fields[name][1] and getattr(S, name).size == mine.fields[name][0].itemsize, name
    assert {n: getattr(S, n).offset for n in ("c", "f", "a", "b", "d", "e", "fill", "flags", "reserved")} == dict(c=0, f=8, a=16, b=20, d=24, e=28, fill=32, flags=35, reserved=36)
    assert na.WARP_MAX_STEP == 64 and na.WARP_BORDERS == {"fill": 0, "replicate": 1}


def lib_fixed(M):
    """warp_fixed of the library, held against the test's own words: what the hand-worked cases feed the rule with"""
    import nhwcodec_amd as na
    six = na.warp_fixed(M)
    assert six == fixed(M) and all(type(v) is int for v in six), (M, six, fixed(M))
    return six


def test_the_warp_rule_by_hand():
    """the cases of section 21 worked by hand: the matrices as a caller writes them, through warp_fixed, then the rule"""
    rng = np.random.default_rng(210)
    for w, h in ((53, 37), (1, 1)):
        P = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ident = lib_fixed([[1, 0, 0], [0, 1, 0]])
        assert ident == (65536, 0, -32768, 0, 65536, -32768)
        for rep in (False, True):
            assert np.array_equal(rule(P, w, h, ident, (1, 2, 3), rep), P)                                       # identity
            turn = rule(P, h, w, lib_fixed([[0, 1, 0], [-1, 0, h]]), (1, 2, 3), rep)                                 # sx = v, sy = (output width) - u
            assert np.array_equal(turn, np.rot90(P, -1)) and turn.shape == (w, h, 3)
            assert np.array_equal(rule(P, w, h, lib_fixed([[-1, 0, w], [0, 1, 0]]), (1, 2, 3), rep), P[:, ::-1])     # the mirror
            assert np.array_equal(rule(P, w, h, lib_fixed([[-1, 0, w], [0, -1, h]]), (1, 2, 3), rep), P[::-1, ::-1])
    P = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    moved = rule(P, 53, 37, lib_fixed([[1, 0, 5], [0, 1, -3]]), (9, 8, 7))                                           # a translation by (5, -3)
    want = np.empty_like(P)
    want[:] = (9, 8, 7)
    want[3:, :48] = P[:34, 5:]
    assert np.array_equal(moved, want)
    clamped = rule(P, 53, 37, lib_fixed([[1, 0, 5], [0, 1, -3]]), (9, 8, 7), True)
    assert np.array_equal(clamped[3:, :48], P[:34, 5:]) and np.array_equal(clamped[:3, :48], np.broadcast_to(P[0, 5:], (3, 48, 3)))
    assert np.array_equal(clamped[3:, 48:], np.broadcast_to(P[:34, 52:53], (34, 5, 3))) and (clamped[:3, 48:] == P[0, 52]).all()
    # half a pixel to the right on the row 0, 255, 10: (0 + 255) / 2 and (255 + 10) / 2 round up; the last pixel blends with the border
    row = np.repeat(np.array([0, 255, 10], np.uint8)[None, :, None], 3, axis=2)
    half = lib_fixed([[1, 0, 0.5], [0, 1, 0]])
    assert half == (65536, 0, 0, 0, 65536, -32768)
    assert rule(row, 3, 1, half)[0, :, 0].tolist() == [128, 133, 5]                  # (32768 x 10 + 32768) >> 16 = 5
    assert rule(row, 3, 1, half, (9, 8, 7))[0, 2].tolist() == [10, 9, 9]             # (32768 x (10 + 9) + 32768) >> 16 = 10; with 8 and 7: 9
    assert rule(row, 3, 1, half, (9, 8, 7), True)[0, :, 1].tolist() == [128, 133, 10]
    quarter = lib_fixed([[1, 0, -0.25], [0, 1, 0]])                                     # a quarter to the left: 64 / 256 of the left neighbour
    assert rule(row, 3, 1, quarter, (100, 100, 100))[0, :, 0].tolist() == [25, 191, 71]   # (64 x 100 + 192 x 0) / 256 = 25; 191.25; 71.25
    # a tap is judged outside even where its weight is 0: at fx = 0 the right tap of the last column is outside, and adds nothing
    assert rule(row, 3, 1, lib_fixed([[1, 0, 0], [0, 1, 0]]), (255, 255, 255))[0, :, 0].tolist() == [0, 255, 10]
    # wholly outside: the border colour, or with replicate the corner pixel
    for M, corner in (([[1, 0, -60], [0, 1, -60]], (0, 0)), ([[1, 0, 60], [0, 1, 60]], (36, 52)), ([[1, 0, -60], [0, 1, 60]], (36, 0)), ([[1, 0, 60], [0, 1, -60]], (0, 52))):
        assert (rule(P, 6, 5, lib_fixed(M), (9, 8, 7)) == np.array((9, 8, 7))).all()
        assert (rule(P, 6, 5, lib_fixed(M), (9, 8, 7), True) == P[corner]).all()
    # a division that truncates, or a shift of an unsigned number, would place -1/256 at 0: the floor places it in pixel -1
    ix, fx, _, _ = positions(lib_fixed([[1, 0, -1 / 256], [0, 1, 0]]), 1, 1)
    assert (int(ix[0, 0]), int(fx[0, 0])) == (-1, 255)


def test_warp_fixed_ties_and_limits():
    import nhwcodec_amd as na
    u = 1.0 / 65536
    assert na.warp_fixed([[1, 0, 0], [0, 1, 0]]) == (65536, 0, -32768, 0, 65536, -32768)
    assert na.warp_fixed([[0.5 * u, 1.5 * u, 0.5 + 0.5 * u], [2.5 * u, -0.5 * u, 0.5 - 1.5 * u]]) == (0, 2, 0, 2, 0, -2)   # ties to even
    assert na.warp_fixed([[3.5 * u, -1.5 * u, 0.5 + 2.5 * u], [-2.5 * u, 0.49 * u, 0.5 + 0.51 * u]]) == (4, -2, 2, -2, 0, 1)
    rng = np.random.default_rng(211)
    for _ in range(50):
        M = rng.uniform(-60, 60, (2, 3))
        assert na.warp_fixed(M) == fixed(M) == na.warp_fixed(M.tolist())
    assert all(isinstance(v, int) for v in na.warp_fixed(np.eye(2, 3)))
    assert na.warp_fixed([[64, -64, 2.0**24 + 0.5], [-64, 64, -2.0**24 + 0.5]]) == (STEP, -STEP, OFFSET, -STEP, STEP, -OFFSET)   # the limits themselves
    for r, c, v in ((0, 0, 64 + u), (0, 1, -64 - u), (1, 0, 64 + u), (1, 1, -64 - u), (0, 2, 2.0**24 + 0.5 + u * 256), (1, 2, -2.0**24 + 0.5 - u * 256),
                    (0, 0, float("nan")), (1, 2, float("inf")), (0, 1, -float("inf")), (1, 1, 1e300)):
        M = np.array([[1.0, 0, 0], [0, 1.0, 0]])
        M[r, c] = v
        with pytest.raises(na.NhwError):
            na.warp_fixed(M)
    for bad in (np.eye(3), [1, 2, 3, 4, 5, 6], "matrix", None, [[1, 0, 0], [0, 1]]):
        with pytest.raises(na.NhwError):
            na.warp_fixed(bad)


def test_warp_scale():
    import nhwcodec_amd as na
    for step, want in ((1.99, 1), (2, 2), (3.99, 2), (4, 4), (0.3, 1), (63, 4)):
        for angle in (0.0, 0.7, math.pi / 2, -2.0):
            M = centred(100, 100, 10, 10, angle, step)
            if step in (2, 4) and angle:                              # a turned step of exactly 2 may come out a rounding below it
                M = M * (1 + 1e-12)
            assert na.warp_scale(M) == want, (step, angle)
    assert na.warp_scale([[2, 0, 0], [0, 2, 0]]) == 2 and na.warp_scale([[0, 4, 0], [-4, 0, 0]]) == 4
    # a shear: the step along ox is hypot(2.1, 0) = 2.1, along oy hypot(0.4, 1.9) = 1.94: the smaller decides
    assert na.warp_scale([[2.1, 0.4, 0], [0, 1.9, 0]]) == 1 and na.warp_scale([[1.9, 0.4, 0], [0, 2.1, 0]]) == 1
    assert na.warp_scale([[2.1, 0.9, 0], [0, 1.9, 0]]) == 2         # hypot(0.9, 1.9) = 2.10
    assert na.warp_scale([[4.5, 0, 0], [0, 3.9, 0]]) == 2 and na.warp_scale([[4.5, 1, 0], [0, 3.9, 0]]) == 4
    with pytest.raises(na.NhwError):
        na.warp_scale([[float("nan"), 0, 0], [0, 1, 0]])


def seeded_matrices(n, rng, pic_w, pic_h, out_w, out_h, zooms=(0.3, 5.0), outside=True):
    """n matrices in full-resolution coordinates: angles in +-pi, steps of zooms[0] .. zooms[1] pixels, shears of +-0.3, the output's centre
    inside the picture or (every fourth, with `outside`) up to a picture's size beyond it"""
    out = []
    for i in range(n):
        zoom = float(np.exp(rng.uniform(np.log(zooms[0]), np.log(zooms[1]))))
        far = outside and i % 4 == 3
        shift = (rng.uniform(-1.5, 1.5) * pic_w, rng.uniform(-1.5, 1.5) * pic_h) if far else (rng.uniform(-0.5, 0.5) * pic_w, rng.uniform(-0.5, 0.5) * pic_h)
        out.append(centred(pic_w, pic_h, out_w, out_h, rng.uniform(-math.pi, math.pi), zoom, (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)), shift))
    return out


def test_warp_window_is_the_warp_of_the_whole_picture():
    """200 seeded matrices over a 1300 x 700 picture at the scales 1, 2, 4: the rule on the window under fixed' is the rule on the whole scaled
    picture under m, with both borders; the window lies inside the scaled picture, is never empty and holds every tap that lies in the picture"""
    import nhwcodec_amd as na
    W, H = 1300, 700
    rng = np.random.default_rng(212)
    full = {s: rng.integers(0, 256, (-(-H // s), -(-W // s), 3), dtype=np.uint8) for s in SCALES}
    seen_outside = seen_partial = 0
    for i, M in enumerate(seeded_matrices(200, rng, W, H, 24, 16)):
        s = SCALES[i % 3]
        out_w, out_h = ((24, 16), (7, 31), (1, 1), (40, 3))[i % 4]
        sh, sw = full[s].shape[:2]
        (x0, y0, w0, h0), fx = na.warp_window(M, (out_h, out_w), W, H, s)
        m = fixed(np.asarray(M) / s)
        assert fx == (m[0], m[1], m[2] - 65536 * x0, m[3], m[4], m[5] - 65536 * y0)
        assert w0 >= 1 and h0 >= 1 and 0 <= x0 and x0 + w0 <= sw and 0 <= y0 and y0 + h0 <= sh, (i, x0, y0, w0, h0)
        ix, _, iy, _ = positions(m, out_w, out_h)
        taps_x, taps_y = np.stack([ix, ix + 1, ix, ix + 1]), np.stack([iy, iy, iy + 1, iy + 1])
        inside = (taps_x >= 0) & (taps_x < sw) & (taps_y >= 0) & (taps_y < sh)
        held = (taps_x >= x0) & (taps_x < x0 + w0) & (taps_y >= y0) & (taps_y < y0 + h0)
        assert (held | ~inside).all(), i
        seen_outside += not inside.any()
        seen_partial += inside.any() and not inside.all()
        window = full[s][y0:y0 + h0, x0:x0 + w0]
        for rep in (False, True):
            assert np.array_equal(rule(window, out_w, out_h, fx, (9, 8, 7), rep), rule(full[s], out_w, out_h, m, (9, 8, 7), rep)), (i, s, rep)
    assert seen_outside >= 5 and seen_partial >= 10
    with pytest.raises(na.NhwError):
        na.warp_window(np.eye(2, 3), (16, 24), W, H, 3)
    with pytest.raises(na.NhwError):
        na.warp_window(np.eye(2, 3) * 100, (16, 24), W, H, 1)


def test_the_widths_of_the_rule():
    """over the extreme entries -- steps of +-2^22, offsets of +-2^40, the corners of a 4096 x 4096 output -- |SX| stays below 2^41 and ix
    inside 32 bits (it stays below 2^25).  The library's own integers walk the same corners: warp_fixed gives the extreme entries from
    their matrices, and warp_window, which evaluates the rule at the four corners, gives the window those positions select"""
    import nhwcodec_amd as na
    most, most_ix = 0, 0
    for A in (-64.0, 64.0):
        for B in (-64.0, 64.0):
            for C in (-2.0**24 + 0.5, 2.0**24 + 0.5):
                M = [[A, B, C], [B, A, C]]
                a, b, c = int(A) << 16, int(B) << 16, (1 << 40 if C > 0 else -(1 << 40))
                assert na.warp_fixed(M) == (a, b, c, b, a, c) and abs(a) == abs(b) == STEP and abs(c) == OFFSET
                got = positions((a, b, c, b, a, c), 4096, 4096, (0, 4095), (0, 4095))
                ixs, iys = [], []
                for i, ox in enumerate((0, 4095)):
                    for j, oy in enumerate((0, 4095)):
                        SX = ((a * (2 * ox + 1) + b * (2 * oy + 1)) >> 1) + c                  # Python's integers: no width to overflow
                        SY = ((b * (2 * ox + 1) + a * (2 * oy + 1)) >> 1) + c
                        ix, iy = (SX + 128) >> 16, (SY + 128) >> 16
                        most, most_ix = max(most, abs(SX), abs(SY)), max(most_ix, abs(ix), abs(ix + 1), abs(iy), abs(iy + 1))
                        assert int(got[0][j, i]) == ix and int(got[2][j, i]) == iy
                        ixs.append(ix)
                        iys.append(iy)
                clamp = lambda v: min(max(v, 0), 65534)
                x0, x1, y0, y1 = clamp(min(ixs)), clamp(max(ixs) + 1), clamp(min(iys)), clamp(max(iys) + 1)
                win, fx = na.warp_window(M, (4096, 4096), 65535, 65535, 1)
                assert win == (x0, y0, x1 - x0 + 1, y1 - y0 + 1) and win in ((0, 0, 1, 1), (65534, 65534, 1, 1)), (M, win)   # 2^24 pixels away: a corner pixel
                assert fx == (a, b, c - 65536 * x0, b, a, c - 65536 * y0) and abs(fx[2]) <= OFFSET and abs(fx[5]) <= OFFSET
    assert most == (STEP * 8191 * 2 >> 1) + OFFSET < 1 << 41 and most_ix < 1 << 25 < 1 << 31


YARDSTICK_SEED = 1


def test_the_rule_against_torch_grid_sample():
    """the rule against an outside implementation of bilinear sampling in float64: no byte is more than 1 from torch's rounded, clipped value.
    Seeded noise and a smooth 300 x 200 picture, 64 x 48 outputs, 40 matrices each: a turn in +-pi, steps of 0.5 .. 1.9 pixels, shears of
    +-0.3, the centre within (+-40, +-30) of the picture's.  (Observed, printed below and recorded in DESIGN.md section 21, not gated: the
    largest distance from torch's real value 1.252 on noise and 0.757 on the smooth picture; 10.7 % and 0.4 % of the bytes differ from
    the rounded value -- the positions are quantised to 1/256 pixel, which noise shows.)"""
    import torch
    import torch.nn.functional as F
    w, h, out_w, out_h = 300, 200, 64, 48
    rng = np.random.default_rng(YARDSTICK_SEED)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), xx * 255 / (w - 1), yy * 255 / (h - 1)], -1).astype(np.uint8)
    for kind, P in (("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), ("smooth", smooth)):
        t = torch.from_numpy(P).permute(2, 0, 1)[None].double()
        worst = worst_real = 0.0
        differ = []
        for _ in range(40):
            M = centred(w, h, out_w, out_h, rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 1.9), (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)),
                        (rng.uniform(-40, 40), rng.uniform(-30, 30)))
            u, v = np.meshgrid(np.arange(out_w) + 0.5, np.arange(out_h) + 0.5)
            sx, sy = M[0, 0] * u + M[0, 1] * v + M[0, 2], M[1, 0] * u + M[1, 1] * v + M[1, 2]
            grid = torch.from_numpy(np.stack([2 * sx / w - 1, 2 * sy / h - 1], -1))[None]
            T = F.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0].permute(1, 2, 0).numpy()
            got = rule(P, out_w, out_h, lib_fixed(M)).astype(np.int64)                       # the integers a caller's matrix becomes
            d = np.abs(got - np.clip(np.floor(T + 0.5), 0, 255))
            worst, worst_real = max(worst, float(d.max())), max(worst_real, float(np.abs(got - np.clip(T, 0, 255)).max()))
            differ.append(float((d > 0).mean()))
        print(f"{kind}: largest byte difference {worst:.0f}, largest real difference {worst_real:.3f}, share of differing bytes {np.mean(differ):.4f}")
        assert worst <= 1, kind


def test_warp_refusals_before_any_device():
    import torch
    import nhwcodec_amd as na
    fmt = _fmt(*BYTES)
    host = [torch.zeros((4, 5, 3), dtype=torch.uint8)]               # host tensors: what is wrong with the call is said before where they live
    eye = np.eye(2, 3)
    dec = object.__new__(na.Decoder)                                 # no handle, no device
    for border in ("clamp", "FILL", "", None, 1):
        with pytest.raises(na.NhwError, match="'fill', 'replicate'"):
            na.warp_to_tensor_device(host, [eye], (8, 8), fmt, border=border)
        with pytest.raises(na.NhwError, match="'fill', 'replicate'"):
            dec.decode_warps_device([b"no container"], [0], [eye], (8, 8), fmt, border=border)
    for fill in ((0, 0), (0, 0, 0, 0), (0, 0, 256), (-1, 0, 0), (0.5, 0, 0), 7, None, "abc"):
        with pytest.raises(na.NhwError, match="three bytes"):
            na.warp_to_tensor_device(host, [eye], (8, 8), fmt, fill=fill)
        with pytest.raises(na.NhwError, match="three bytes"):
            dec.decode_warps_device([b"no container"], [0], [eye], (8, 8), fmt, fill=fill)
    for bad in (np.eye(3), np.zeros(6), [[1, 0], [0, 1]], "m", None, np.zeros((2, 3), dtype=complex), [[1, 0, 0], [0, 1, "x"]]):
        with pytest.raises(na.NhwError, match="2 x 3"):
            na.warp_to_tensor_device(host, [bad], (8, 8), fmt)
        with pytest.raises(na.NhwError, match="2 x 3"):
            dec.decode_warps_device([b"no container"], [0], [bad], (8, 8), fmt)
    for matrices in ([], [eye, eye]):                                # one matrix a picture, one a container index
        with pytest.raises(na.NhwError, match="same length"):
            na.warp_to_tensor_device(host, matrices, (8, 8), fmt)
        with pytest.raises(na.NhwError, match="same length"):
            dec.decode_warps_device([b"no container"], [0], matrices, (8, 8), fmt)
    with pytest.raises(na.NhwError, match="limits"):                 # a step of 65 pixels; the six integers beyond the limits
        na.warp_to_tensor_device(host, [eye * 65], (8, 8), fmt)
    with pytest.raises(na.NhwError, match="limits"):
        na.warp_to_tensor_device(host, [(STEP + 1, 0, 0, 0, 65536, 0)], (8, 8), fmt)
    with pytest.raises(na.NhwError, match="container index"):
        dec.decode_warps_device([b"no container"], [1], [eye], (8, 8), fmt)
    with pytest.raises(na.NhwError, match="size"):
        dec.decode_warps_device([b"no container"], [0], [eye], (8, 4097), fmt)
    with pytest.raises(na.NhwError, match="scale"):
        dec.decode_warps_device([b"no container"], [0], [eye], (8, 8), fmt, scale=3)
    with pytest.raises(na.NhwError, match="CUDA"):                   # ... and with everything else right, the next check speaks
        na.warp_to_tensor_device(host, [eye], (8, 8), fmt)
    with pytest.raises(na.NhwError, match="CUDA"):
        na.warp_to_tensor_device(host, [(65536, 0, -32768, 0, 65536, -32768)], (8, 8), fmt, border="replicate")


def test_crop_warp_matrices():
    import nhwcodec_amd as na
    assert np.array_equal(na.crop_warp(10, 20, 32, 24, (24, 32)), [[1, 0, 10], [0, 1, 20]])
    assert np.array_equal(na.crop_warp(10, 20, 64, 12, (24, 32)), [[2, 0, 10], [0, 0.5, 20]])
    assert np.array_equal(na.crop_warp(10, 20, 32, 24, (24, 32), flip=True), [[-1, 0, 42], [0, 1, 20]])
    assert fixed(na.crop_warp(10, 20, 30, 30, (30, 30), math.pi / 2)) == fixed([[0, -1, 40], [1, 0, 20]])
    assert fixed(na.crop_warp(10, 20, 30, 30, (30, 30), math.pi)) == fixed([[-1, 0, 40], [0, -1, 50]])
    M = na.crop_warp(3, 4, 50, 40, (20, 25), 0.3, True)
    assert np.allclose(M @ [12.5, 10, 1], [28, 24])                  # the output's centre lies on the rectangle's
    assert na.warp_scale(na.crop_warp(0, 0, 900, 900, (224, 224), 0.5)) == 4 and "stored rows" in na.crop_warp.__doc__.lower()
    for bad in ((0, 0, 0, 5), (0, 0, 5, -1), (float("nan"), 0, 5, 5), ("x", 0, 5, 5)):
        with pytest.raises(na.NhwError):
            na.crop_warp(*bad, (8, 8))


# ---------------------------------------------------------------- on the MI355X: the kernel alone
SRC_SIZES = [(1, 1), (2, 1), (1, 3), (5, 4), (53, 37), (300, 200)]                                                # W, H
OUT_SIZES = [(1, 1), (3, 2), (7, 9), (8, 8), (9, 7), (65, 17), (37, 53), (100, 75), (224, 224), (4096, 1)]        # W, H
ALL_32 = (100, 75)                                                  # the output size that meets all 32 formats


def kernel_warps(w, h, out_w, out_h):
    """the warps a w x h source meets on its way to out_w x out_h, as six integers"""
    c = lambda *a, **k: fixed(centred(w, h, out_w, out_h, *a, **k))
    inside = (65536 * (w - 1) // 2 + 77, 65536 * (h - 1) // 3 + 12345)
    return [
        fixed([[1, 0, 0], [0, 1, 0]]), fixed([[0, 1, 0], [-1, 0, h]]), fixed([[-1, 0, w], [0, -1, h]]), fixed([[-1, 0, w], [0, 1, 0]]),   # identity, 90, 180 degrees, mirror
        c(math.pi / 2), c(math.pi / 6, 0.7), c(math.pi / 6, 1.9), c(-2.0, min(w / out_w, 60.0)), c(0.0, 1.0, (0.3, -0.2)),                  # turns; a shear
        c(0.4, min(max(w / out_w, h / out_h), 30.0) * 1.3, (0.1, 0.2)),                                                                          # the whole picture and a border all round
        (0, 0, inside[0], 0, 0, inside[1]), (0, 0, -1, 0, 0, 65536 * h - 32768 - 128),                                                      # all-zero steps: one position for all
        fixed([[1, 0, -out_w - 2], [0, 1, 0]]), fixed([[1, 0, w + 1], [0, 1, 0]]), fixed([[1, 0, 0], [0, 1, -out_h - 2]]), fixed([[1, 0, 0], [0, 1, h + 1]]),   # wholly outside, four sides
        (65536, 3000, -32768, 16384, 65536, -32768), (65536, -3000, -32768, -16385, 65536, -32768),                                           # either side of the kernel's choice of walk
        (STEP, 0, -STEP // 2 + 13, 0, -STEP, 65536 * (h - 1) + STEP // 2), (-STEP, STEP, inside[0], STEP, STEP, -32768),                    # steps at +-2^22
        (65536, 0, OFFSET, 0, 65536, -32768), (65536, 0, -OFFSET, 0, 65536, -32768), (65536, 0, -32768, 0, 65536, OFFSET), (0, 65536, -32768, -65536, 0, -OFFSET),   # offsets at +-2^40
    ]


class Sources:
    """sizes -> views of one device buffer of random bytes, every row followed by a gap of 1 .. bytes and every picture at an odd address;
    .own their bytes on the host; .table the nhw_picture table on the host"""

    def __init__(self, sizes, seed):
        import torch
        import nhwcodec_amd as na
        at, places = 1, []
        for k, (w, h) in enumerate(sizes):
            pitch = 3 * w + 1 + 2 * (k % 5)
            places.append((at, pitch))
            at = (at + h * pitch + 7) | 1
        host = np.random.default_rng(seed).integers(0, 256, at + 64, dtype=np.uint8)
        self.sizes = sizes
        self.own = [np.stack([host[o + r * p: o + r * p + 3 * w] for r in range(h)]).reshape(h, w, 3).copy() for (o, p), (w, h) in zip(places, sizes)]
        self.buf = torch.from_numpy(host).cuda()
        self.views = [self.buf.as_strided((h, w, 3), (p, 3, 1), o) for (o, p), (w, h) in zip(places, sizes)]
        assert all(v.data_ptr() % 2 == 1 for v in self.views)
        self.table = na._picture_table(self.views, "test")[0].cpu().numpy().view(na.PICTURE_DTYPE).copy()


@pytest.fixture(scope="module")
def sources():
    return Sources(SRC_SIZES, 213)


def warp_table(entries):
    """[(six integers, fill, replicate)] -> the nhw_warp table on the host; bits of the flag byte above bit 0 are set on some: they are not read"""
    t = np.zeros(len(entries), WARP)
    for i, ((a, b, c, d, e, f), fill, rep) in enumerate(entries):
        t[i] = (c, f, a, b, d, e, fill, int(rep) | (0xFE if i % 3 == 1 else 0), 0)
    return t


def _guarded(n, per, fmt):
    """a canary-filled byte buffer with room for n tensors of `per` elements between two guards -> (buffer, the byte offset of tensor 0)"""
    import torch
    buf = torch.full((2 * GUARD + n * per * fmt.dtype.itemsize,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, GUARD


def _launch(table, warps, out_w, out_h, fmt, other_addr=None, n=None, null_warps=False):
    """one launch of nhw_warp_to_tensor_device over a host table into a guarded batch; other_addr: {entry: function of its slot's address} for
    the entries that get another address -> (rc, the batch's slots as byte arrays, guards intact)"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    count, per, es = len(table), 3 * out_w * out_h, fmt.dtype.itemsize
    buf, at = _guarded(count, per, fmt)
    slots = [buf.data_ptr() + at + i * per * es for i in range(count)]
    addr = torch.tensor([(other_addr or {}).get(i, int)(s) for i, s in enumerate(slots)], dtype=torch.int64, device="cuda")
    d_tab = torch.from_numpy(np.ascontiguousarray(table).view(np.int64).copy()).cuda()
    d_warps = torch.from_numpy(np.ascontiguousarray(warps).view(np.int64).copy()).cuda()
    assert d_warps.data_ptr() % 8 == 0 and d_warps.numel() == 5 * len(warps)
    c = fmt.c_struct()
    rc = L.nhw_warp_to_tensor_device(d_tab.data_ptr(), count if n is None else n, out_w, out_h, ctypes.byref(c), None if null_warps else d_warps.data_ptr(), addr.data_ptr(), None)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:at] == CANARY).all() and (host[at + count * per * es:] == CANARY).all())
    return rc, [host[at + i * per * es: at + (i + 1) * per * es] for i in range(count)], intact


def _same(got, px, fmt):
    want = expected_tensor(px, fmt)
    return np.array_equal(got.view(want.dtype).reshape(want.shape), want)


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h", OUT_SIZES)
def test_gpu_warp_kernel_on_random_bytes(sources, out_w, out_h):
    """every source under every warp of kernel_warps in one launch, the borders and three border colours mixed over the entries: under all 32
    formats for one output size, under two formats for the others; the batch between guards; then the wrapper"""
    import nhwcodec_amd as na
    which, entries = [], []
    for k, (w, h) in enumerate(SRC_SIZES):
        for six in kernel_warps(w, h, out_w, out_h):
            which.append(k)
            entries.append((six, FILLS[(len(entries) // 2) % 3], len(entries) % 2 == 1))
    assert len(entries) == 24 * len(SRC_SIZES)
    want = [rule(sources.own[k], out_w, out_h, *e) for k, e in zip(which, entries)]
    assert out_w * out_h < 6 or sum((r != r[0, 0]).any() for r in want) > len(want) // 3   # pictures, not flat colours
    warps = warp_table(entries)
    formats = [_fmt(*four, k=i // 2) for i, four in enumerate(ALL_FORMATS)] if (out_w, out_h) == ALL_32 else [_fmt(*BYTES), _fmt(*HALF)]
    assert len(formats) in (2, 32)
    for fmt in formats:
        rc, slots, intact = _launch(sources.table[which], warps, out_w, out_h, fmt)
        assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
        for j, (k, e) in enumerate(zip(which, entries)):
            assert _same(slots[j], want[j], fmt), f"{fmt} source {SRC_SIZES[k]} to {out_w} x {out_h}, entry {j}: warp {e}"
    fmt = _fmt(*HALF)
    for border, fill in (("fill", (9, 8, 7)), ("replicate", (1, 2, 3))):
        mine = [j for j in range(len(entries)) if j % 7 == 0 or j < 24]
        got = na.warp_to_tensor_device([sources.views[which[j]] for j in mine], [np.array(entries[j][0]) if j % 2 else entries[j][0] for j in mine], (out_h, out_w), fmt,
                                       fill=fill, border=border)
        assert got.dtype == fmt.dtype and tuple(got.shape) == (len(mine), 3, out_h, out_w)
        bits = tensor_bits(got)
        for i, j in enumerate(mine):
            assert np.array_equal(bits[i], expected_tensor(rule(sources.own[which[j]], out_w, out_h, entries[j][0], fill, border == "replicate"), fmt)), (border, j)
    M = centred(300, 200, out_w, out_h, 0.5, 1.1)                    # ... and a matrix of floats goes through warp_fixed
    got = na.warp_to_tensor_device([sources.views[5]], [M], (out_h, out_w), fmt, fill=(3, 2, 1))
    assert np.array_equal(tensor_bits(got)[0], expected_tensor(rule(sources.own[5], out_w, out_h, fixed(M), (3, 2, 1)), fmt))


@pytest.mark.gpu
def test_gpu_warp_either_walk_gives_the_same_bytes(sources, lib):
    """the kernel walks an entry by rows or by 8 x 8 blocks, chosen from d; with nhw_debug_warp_row_limit every entry takes the one, then the
    other: the bytes are the rule's both times, at sizes that leave partial rows and partial blocks on every edge"""
    try:
        for limit in (-1, STEP, 8192):
            lib.nhw_debug_warp_row_limit(limit)
            for out_w, out_h in ((9, 7), (65, 17), (37, 53), (100, 75)):
                which, entries = [], []
                for k in (3, 4, 5):
                    for six in kernel_warps(*SRC_SIZES[k], out_w, out_h)[:14]:
                        which.append(k)
                        entries.append((six, FILLS[len(entries) % 3], len(entries) % 2 == 1))
                for four in (BYTES, HALF):
                    fmt = _fmt(*four)
                    rc, slots, intact = _launch(sources.table[which], warp_table(entries), out_w, out_h, fmt)
                    assert rc == 0 and intact
                    for j, (k, e) in enumerate(zip(which, entries)):
                        assert _same(slots[j], rule(sources.own[k], out_w, out_h, *e), fmt), (limit, out_w, out_h, fmt, j, e)
    finally:
        lib.nhw_debug_warp_row_limit(-2)                                 # the rule's own limit again


@pytest.mark.gpu
def test_gpu_warp_large_sources():
    """a 65535 x 2 source sampled at its far end, so that ix = 65534 and 65535 are reached, and a 2 x 65535 source at its last row (the row
    offset is 65534 times the pitch)"""
    src = Sources([(65535, 2), (2, 65535)], 214)
    out_w, out_h = 9, 5
    entries = []
    for rep in (False, True):
        entries += [(fixed([[1, 0, 65535 - 7.25], [0, 1, -1.5]]), (9, 8, 7), rep), (fixed([[-1, 0, 65535 + 1.5], [0, 0.5, 0.25]]), (9, 8, 7), rep)]
    ix = np.concatenate([positions(e[0], out_w, out_h)[0].reshape(-1) for e in entries])
    assert {65533, 65534, 65535} <= set(ix.tolist())
    for four in (BYTES, HALF):
        fmt = _fmt(*four)
        rc, slots, intact = _launch(src.table[[0] * 4], warp_table(entries), out_w, out_h, fmt)
        assert rc == 0 and intact
        for j, e in enumerate(entries):
            assert _same(slots[j], rule(src.own[0], out_w, out_h, *e), fmt), (fmt, j)
    tall = []
    for rep in (False, True):
        tall += [(fixed([[1, 0, -1.5], [0, 1, 65535 - 3.25]]), (9, 8, 7), rep), (fixed([[0.5, 0, 0.25], [0, -1, 65535 + 1.5]]), (9, 8, 7), rep)]
    iy = np.concatenate([positions(e[0], out_w, out_h)[2].reshape(-1) for e in tall])
    assert {65533, 65534, 65535} <= set(iy.tolist())
    for four in (BYTES, HALF):
        fmt = _fmt(*four)
        rc, slots, intact = _launch(src.table[[1] * 4], warp_table(tall), out_w, out_h, fmt)
        assert rc == 0 and intact
        for j, e in enumerate(tall):
            assert _same(slots[j], rule(src.own[1], out_w, out_h, *e), fmt), (fmt, j)


@pytest.mark.gpu
def test_gpu_warp_entries_that_store_nothing(sources):
    """a step of 2^22 + 1, an offset of 2^40 + 1 (of either sign, in every field), a zero side, an oversize side, a zero address and a misaligned
    one: their slots keep the canary, the valid entries between them are right"""
    out_w, out_h = 9, 7
    good = fixed(centred(53, 37, out_w, out_h, 0.3, 2.0))
    beyond = []
    for i in (0, 1, 3, 4):
        for v in (STEP + 1, -STEP - 1, -(1 << 31)):
            beyond.append(tuple(v if j == i else x for j, x in enumerate(good)))
    for i in (2, 5):
        for v in (OFFSET + 1, -OFFSET - 1, (1 << 63) - 1, -(1 << 63)):
            beyond.append(tuple(v if j == i else x for j, x in enumerate(good)))
    sixes = []
    for six in beyond:
        sixes += [good, six]
    picks = [4] * len(sixes) + [4, 4, 4, 4, 4, 4]
    sixes += [good] * 6
    n = len(sixes)
    tab = sources.table[picks]
    tab["width"][n - 6] = 0
    tab["height"][n - 5] = 65536
    warps = np.zeros(n, WARP)
    for i, (a, b, c, d, e, f) in enumerate(sixes):
        warps[i] = (c, f, a, b, d, e, (9, 8, 7), i % 2, 0)
    for four in (BYTES, HALF, ("float32", "HWC", "BGR", "file")):
        fmt = _fmt(*four)
        other = {n - 4: lambda a: 0}                                                    # no address
        silent = set(range(1, n - 6, 2)) | {n - 6, n - 5, n - 4}
        if fmt.dtype.itemsize > 1:                                                      # no multiple of the element size (a byte's divides every address)
            other[n - 3] = lambda a: a + 1
            silent.add(n - 3)
        rc, slots, intact = _launch(tab, warps, out_w, out_h, fmt, other)
        assert rc == 0 and intact
        for i in range(n):
            if i in silent:
                assert (slots[i] == CANARY).all(), (fmt, i)
            else:
                assert _same(slots[i], rule(sources.own[4], out_w, out_h, good, (9, 8, 7), bool(i % 2)), fmt), (fmt, i)


@pytest.mark.gpu
def test_gpu_warp_many_entries():
    """4096 entries of 7 x 5 -> 3 x 4, each under a seeded warp of its own: with so many an entry is one band"""
    n, out_w, out_h = 4096, 3, 4
    src = Sources([(7, 5)] * 5, 215)
    rng = np.random.default_rng(216)
    which = np.arange(n) % 5
    mats = seeded_matrices(n, rng, 7, 5, out_w, out_h, zooms=(0.3, 3.0))
    entries = [(fixed(M), FILLS[i % 3], i % 2 == 1) for i, M in enumerate(mats)]
    fmt = _fmt("float16", "CHW", "BGR", "reversed")
    rc, slots, intact = _launch(src.table[which], warp_table(entries), out_w, out_h, fmt)
    assert rc == 0 and intact
    for i, e in enumerate(entries):
        assert _same(slots[i], rule(src.own[which[i]], out_w, out_h, *e), fmt), (i, e)


@pytest.mark.gpu
def test_gpu_warp_entry_refusals(sources):
    """a null table of warps, no entries, an oversize or empty output: NHW_E_ARG, and nothing is written"""
    import nhwcodec_amd as na
    fmt = _fmt(*HALF)
    warps = warp_table([(fixed(np.eye(2, 3)), (0, 0, 0), False)] * len(SRC_SIZES))
    for kw, (out_w, out_h) in ((dict(null_warps=True), (8, 8)), (dict(n=0), (8, 8)), (dict(n=-1), (8, 8)), (dict(n=(1 << 24) + 1), (8, 8)), ({}, (4097, 1)), ({}, (1, 4097)),
                               ({}, (0, 8)), ({}, (8, 0))):
        rc, slots, intact = _launch(sources.table, warps, out_w, out_h, fmt, **kw)
        assert rc == NHW_E_ARG and intact and all((s == CANARY).all() for s in slots), (kw, out_w, out_h)
    assert b"4096" in na._library().nhw_last_error()
    rc, slots, intact = _launch(sources.table, warps, 8, 8, fmt)
    assert rc == 0 and intact and _same(slots[4], rule(sources.own[4], 8, 8, fixed(np.eye(2, 3))), fmt)


# ---------------------------------------------------------------- on the MI355X: the decoder path
@pytest.fixture(scope="module")
def world():
    """the crops' pictures (SIZES: 1 x 700, 500 x 375, 1023 x 1025, crops of one seeded scene of generated images) as containers at q20, a
    decoder of 4 tiles a chunk, and each picture decoded whole at every scale: what a warp is held against"""
    import nhwcodec_amd as na
    w = World()
    enc = na.Encoder(0, max_batch=24)
    scene = na.untile_images(enc.synth_device(24, 1300).cpu().numpy(), 4, 6)
    w.containers = enc.encode_pictures([np.ascontiguousarray(scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES], 20)
    enc.close()
    w.dec = na.Decoder(0, max_batch=4)
    w.full = {s: w.dec.decode_pictures_scaled(w.containers, s) for s in SCALES}
    for s in SCALES:
        for a in w.full[s]:
            a.setflags(write=False)
    yield w
    w.dec.close()


def seeded_warps(n, rng, out_w, out_h, scale=None):
    """n (container, matrix) over the large and the small picture: with a scale, steps that suit it; without, steps of 0.4 .. 7 pixels"""
    out = []
    zooms = (0.4, 7.0) if scale is None else (0.6 * scale, 1.95 * scale)
    for i in range(n):
        ci = (BIG, BIG, SMALL)[i % 3]
        four = seeded_matrices(4, rng, *SIZES[ci], out_w, out_h, zooms=zooms)      # the fourth has its centre up to a picture's size outside
        out.append((ci, four[3 if i % 8 == 7 else 0]))
    return out


def _windows(warps, out_w, out_h, scales):
    import nhwcodec_amd as na
    return [(ci, *na.warp_window(M, (out_h, out_w), *SIZES[ci], s)[0]) for (ci, M), s in zip(warps, scales)]


@pytest.mark.gpu
@pytest.mark.parametrize("out_w,out_h,four", [(32, 24, BYTES), (224, 224, HALF)])
@pytest.mark.parametrize("scale", SCALES)
def test_gpu_warps_equal_the_rule_on_the_whole_decoded_picture(world, scale, out_w, out_h, four):
    """40 seeded warps in one call on a decoder of max_batch 4, against the rule on decode_pictures_scaled of the whole picture under
    fixed(matrix / scale): warp_window's identity, end to end; the statistics are those of decode_windows_device on the same windows; then
    the warps shuffled, into a tensor of the caller's"""
    import torch
    fmt = _fmt(*four)
    rng = np.random.default_rng(2100 + 10 * scale + out_w)
    warps = seeded_warps(40, rng, out_w, out_h, scale)
    border, fill = ("fill", (9, 8, 7)) if out_w == 32 else ("replicate", (0, 0, 0))
    rects = _windows(warps, out_w, out_h, [scale] * len(warps))
    world.dec.decode_windows_device(world.containers, rects, scale)
    stats = world.dec.region_stats()
    assert stats == expected_stats(world.containers, rects, scale, unique=True) and stats[0] >= 3
    got, scales = world.dec.decode_warps_device(world.containers, [ci for ci, _ in warps], [M for _, M in warps], (out_h, out_w), fmt, fill=fill, border=border, scale=scale)
    assert scales == [scale] * len(warps) and got.dtype == fmt.dtype and tuple(got.shape) == (len(warps),) + fmt.shape(out_h, out_w)
    assert world.dec.region_stats() == stats
    bits = tensor_bits(got)
    for i, (ci, M) in enumerate(warps):
        want = rule(world.full[scale][ci], out_w, out_h, fixed(M / scale), fill, border == "replicate")
        assert np.array_equal(bits[i], expected_tensor(want, fmt)), (scale, i, ci, M.tolist())
    perm = rng.permutation(len(warps))
    per = 3 * out_w * out_h
    mine = torch.full((len(warps) * per + 64,), 1, dtype=fmt.dtype, device="cuda")
    before = tensor_bits(mine[len(warps) * per:]).copy()
    again, _ = world.dec.decode_warps_device(world.containers, [warps[i][0] for i in perm], [warps[i][1] for i in perm], (out_h, out_w), fmt, fill=fill, border=border,
                                             scale=scale, out=mine)
    assert again.data_ptr() == mine.data_ptr() and world.dec.region_stats() == stats
    assert np.array_equal(tensor_bits(again), bits[perm])
    assert np.array_equal(tensor_bits(mine[len(warps) * per:]), before)


@pytest.mark.gpu
def test_gpu_warps_choose_their_scale(world):
    """scale=None: every warp at warp_scale of its matrix, all three scales in one call"""
    import nhwcodec_amd as na
    out_w, out_h = 64, 48
    rng = np.random.default_rng(217)
    warps = seeded_warps(36, rng, out_w, out_h)
    fmt = _fmt("float32", "CHW", "RGB", "reversed", k=1)
    got, scales = world.dec.decode_warps_device(world.containers, [ci for ci, _ in warps], [M for _, M in warps], (out_h, out_w), fmt, fill=(255, 1, 128))
    assert scales == [na.warp_scale(M) for _, M in warps] and all(scales.count(s) >= 4 for s in SCALES)
    for (_, M), s in zip(warps, scales):
        step = min(math.hypot(M[0, 0], M[1, 0]), math.hypot(M[0, 1], M[1, 1]))
        assert s == (4 if step >= 4 else 2 if step >= 2 else 1)
    bits = tensor_bits(got)
    for i, ((ci, M), s) in enumerate(zip(warps, scales)):
        assert np.array_equal(bits[i], expected_tensor(rule(world.full[s][ci], out_w, out_h, fixed(M / s), (255, 1, 128)), fmt)), (i, s)


@pytest.mark.gpu
def test_gpu_crop_warp_is_the_crop_and_its_quarter_turn(world):
    """crop_warp at angle 0 where the crop has the output's size is the slice of the decode; at pi / 2, for a square crop, rot90 of it; with
    flip, the mirror"""
    import nhwcodec_amd as na
    fmt = _fmt(*BYTES)
    full = world.full[1][BIG]
    W, H = SIZES[BIG]
    crops = [(500, 490, 48, 48), (0, 0, 48, 48), (W - 48, H - 48, 48, 48), (3, 700, 48, 48)]
    for angle, flip, turned in ((0.0, False, lambda a: a), (0.0, True, lambda a: a[:, ::-1]), (math.pi / 2, False, lambda a: np.rot90(a, 1)),
                                (-math.pi / 2, False, lambda a: np.rot90(a, -1)), (math.pi, False, lambda a: a[::-1, ::-1])):
        mats = [na.crop_warp(*c, (48, 48), angle, flip) for c in crops]
        got, scales = world.dec.decode_warps_device(world.containers, [BIG] * len(crops), mats, (48, 48), fmt)
        assert scales == [1] * len(crops)
        for i, (x, y, w, h) in enumerate(crops):
            assert np.array_equal(got[i].cpu().numpy(), turned(full[y:y + h, x:x + w])), (angle, flip, crops[i])
    x, y, w, h = 100, 200, 64, 40                                    # not square: the size of the output
    got, _ = world.dec.decode_warps_device(world.containers, [BIG], [na.crop_warp(x, y, w, h, (h, w))], (h, w), fmt)
    assert np.array_equal(got[0].cpu().numpy(), full[y:y + h, x:x + w])
    half = world.full[2][BIG]                                        # a crop of twice the output's size at scale 2: the slice of the half-scale decode
    got, scales = world.dec.decode_warps_device(world.containers, [BIG], [na.crop_warp(2 * x, 2 * y, 2 * w, 2 * h, (h, w))], (h, w), fmt)
    assert scales == [2] and np.array_equal(got[0].cpu().numpy(), half[y:y + h, x:x + w])


def _call_warps(dec, containers, rects, scale, out_w, out_h, fmt, warps, addrs, null_warps=False):
    """nhw_dec_warps_to_device by ctypes -> (rc, status)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    addr = np.array(addrs, np.uint64)
    warps = np.ascontiguousarray(warps)
    c = fmt.c_struct()
    rc = dec.lib.nhw_dec_warps_to_device(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out_w, out_h, ctypes.byref(c),
                                         None if null_warps else warps.ctypes.data, addr.ctypes.data, status.ctypes.data)
    return rc, status


@pytest.mark.gpu
def test_gpu_warps_beyond_the_limits_and_refused_calls(world):
    """a rect whose warp is beyond the limits is NHW_E_ARG, selects no tile -- rect 1 alone would have selected one -- and keeps its slot's
    canary while its neighbours are right; a null table of warps and an oversize output are refused at call level"""
    import torch
    fmt = _fmt(*HALF)
    out_w, out_h = 8, 6
    per, es = 3 * out_w * out_h, 2
    rects = [(BIG, 0, 0, 60, 50), (BIG, 600, 1024, 65, 1), (SMALL, 10, 10, 64, 64), (BIG, 0, 0, 65, 5), (SMALL, 0, 0, 5, 65), (BIG, 3, 3, 30, 30)]
    good = fixed([[2, 0.5, 1], [-0.5, 2, 3]])
    sixes = [good, (STEP + 1,) + good[1:], good, good[:2] + (OFFSET + 1,) + good[3:], good[:4] + (-STEP - 1,) + good[5:], good]
    bad = [s != good for s in sixes]
    ok = [r for r, b in zip(rects, bad) if not b]
    warps = np.zeros(len(rects), WARP)
    for i, (a, b, c, d, e, f) in enumerate(sixes):
        warps[i] = (c, f, a, b, d, e, (9, 8, 7), i % 2, 0)
    buf, at = _guarded(len(rects), per, fmt)
    addrs = [buf.data_ptr() + at + i * per * es for i in range(len(rects))]
    rc, status = _call_warps(world.dec, world.containers, rects, 1, out_w, out_h, fmt, warps, addrs)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_ARG if b else 0 for b in bad]
    assert world.dec.region_stats() == expected_stats(world.containers, ok, 1, unique=True)
    assert expected_stats(world.containers, ok + rects[1:2], 1, unique=True)[0] == world.dec.region_stats()[0] + 1   # rect 1 would have brought a tile of its own
    host = buf.cpu().numpy()
    for i, (r, b) in enumerate(zip(rects, bad)):
        got = host[at + i * per * es: at + (i + 1) * per * es]
        if b:
            assert (got == CANARY).all(), r
        else:
            ci, x, y, w, h = r
            assert _same(got, rule(world.full[1][ci][y:y + h, x:x + w], out_w, out_h, good, (9, 8, 7), bool(i % 2)), fmt), r
    assert (host[:at] == CANARY).all() and (host[at + len(rects) * per * es:] == CANARY).all()
    stats = world.dec.region_stats()
    buf.fill_(CANARY)
    for kw, size in ((dict(null_warps=True), (out_w, out_h)), ({}, (4097, 6)), ({}, (8, 0))):
        rc, status = _call_warps(world.dec, world.containers, ok, 1, *size, fmt, warps[[0, 2, 5]], addrs[:3], **kw)
        assert rc == NHW_E_ARG and (status == 99).all()
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and world.dec.region_stats() == stats


@pytest.mark.gpu
def test_gpu_warps_over_a_truncated_tile(world):
    """a container whose tile (ty 1, tx 1) is cut short: NHW_E_FORMAT for exactly the warps whose window selects it; the others are right"""
    import torch
    import nhwcodec_amd as na
    k = 3                                                            # 1023 x 1025, 2 x 3 tiles: tile (ty 1, tx 1)
    W, H, files = parse_container(world.containers[BIG])
    cut = list(files)
    cut[k] = files[k][:len(files[k]) // 2]
    broken = make_container(W, H, cut)
    assert na.picture_info(broken) == (W, H)
    out_w, out_h = 32, 24
    rng = np.random.default_rng(218)
    mats = [centred(W, H, out_w, out_h, rng.uniform(-3, 3), rng.uniform(0.7, 1.9), shift=(rng.uniform(-500, 500), rng.uniform(-500, 500))) for _ in range(40)]
    wins = [na.warp_window(M, (out_h, out_w), W, H, 1) for M in mats]
    rects = [(0, *win) for win, _ in wins]
    hit = [k in [n for n, _, _ in selected(W, 1, *r[1:])] for r in rects]
    assert 5 < sum(hit) < len(rects) - 5
    fmt = _fmt(*HALF)
    per, es = 3 * out_w * out_h, 2
    buf, at = _guarded(len(rects), per, fmt)
    addrs = [buf.data_ptr() + at + i * per * es for i in range(len(rects))]
    warps = warp_table([(fx, (9, 8, 7), i % 2 == 1) for i, (_, fx) in enumerate(wins)])
    rc, status = _call_warps(world.dec, [broken], rects, 1, out_w, out_h, fmt, warps, addrs)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    assert world.dec.region_stats() == expected_stats([broken], rects, 1, unique=True)
    host = buf.cpu().numpy()
    for i, (M, h) in enumerate(zip(mats, hit)):
        got = host[at + i * per * es: at + (i + 1) * per * es]
        if h:
            assert (got == CANARY).all(), i
        else:
            assert _same(got, rule(world.full[1][BIG], out_w, out_h, fixed(M), (9, 8, 7), i % 2 == 1), fmt), i
    assert (host[:at] == CANARY).all() and (host[at + len(rects) * per * es:] == CANARY).all()
    with pytest.raises(na.NhwError, match="status"):
        world.dec.decode_warps_device([broken], [0] * len(mats), mats, (out_h, out_w), fmt, scale=1)


@pytest.mark.gpu
def test_gpu_one_handle_serves_windows_crops_and_warps_in_turn(world):
    import nhwcodec_amd as na
    rng = np.random.default_rng(219)
    out_w, out_h = 32, 24
    fmt = _fmt(*HALF)
    warps = seeded_warps(12, rng, out_w, out_h, 2)
    rects = _windows(warps, out_w, out_h, [2] * len(warps))
    args = (world.containers, [ci for ci, _ in warps], [M for _, M in warps], (out_h, out_w), fmt)
    before = world.dec.decode_windows(world.containers, rects, 2)
    first = tensor_bits(world.dec.decode_warps_device(*args, scale=2)[0]).copy()
    cubic = tensor_bits(world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, scale=2, filter="cubic")[0]).copy()
    second = tensor_bits(world.dec.decode_warps_device(*args, scale=2)[0]).copy()
    after = world.dec.decode_windows(world.containers, rects, 2)
    again = tensor_bits(world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), fmt, scale=2, filter="cubic")[0])
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and np.array_equal(first, second) and np.array_equal(cubic, again)
    assert not np.array_equal(first, cubic)
    for i, (ci, M) in enumerate(warps):
        assert np.array_equal(first[i], expected_tensor(rule(world.full[2][ci], out_w, out_h, fixed(M / 2)), fmt)), i
        ci, x, y, w, h = rects[i]
        assert np.array_equal(before[i], world.full[2][ci][y:y + h, x:x + w])
