"""Decode straight into training tensors: nhw_tensor_format, nhw_dec_batch_device_tensor (the store policies of k_dec_final
and k_dec_scaled<2> / <4>), nhw_bytes_to_tensor_device (k_bytes_to_tensor) and their Python faces.

The expected values come from the specification, not from the code under test.  The expected BYTES of a file are the oracle decoder's (scale 1)
or section 14's pictures as tests/tensor_cases.py builds them (scales 2, 4).  The expected TENSOR is made on the CPU by
tests/tensor_cases.py's exact_elements: the exact b * scale + bias in rationals, rounded once to float32 as the fma rounds it and once more to the
target type, a table of 256 bit patterns per output channel that expected_tensor indexes with the bytes, flips and permutes by the format.  On
the constants of this file that equals the float64 form these tests used before (product and sum in double, astype(float32), numpy's and
torch's rounding to the type), which test_tensor_values.py asserts bit for bit; check_constants states the condition under which that form
is the fma.  Bit patterns are compared as integers.

Batches (committed files of tests/golden/dec, the smallest shapes that take every path): THREE = q20_0 (eight pixels a thread), q10_0 (four) and
a file truncated to 40 bytes (a refused slot), under all 32 formats; TWO = q23_0, q01_0; NINE = nine files of mixed qualities (its workgroup
count at scale 4 is 36, no multiple of eight; at scale 2 it is 72), the last two under four formats in which every enum value appears.  Every
batch runs at scales 1, 2 and 4 into a sentinel-filled buffer: a refused slot and everything past n * 3 * S * S elements must stay as they were."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle.harness import class_image
from tests.support import ROOT, device_arena, golden, golden_names
from tests.tensor_cases import (ALL_FORMATS, CONSTANTS, DTYPES, IMAGENET_MEAN, IMAGENET_STD, SENTINEL, assert_tensor, check_constants, decode_tensor,
                                expected_bytes, expected_tensor, tensor_bits, tensor_format)

NHW_E_ARG, NHW_E_FORMAT = -4, -6
# the float32 constants TensorFormat(mean=IMAGENET_MEAN, std=IMAGENET_STD) must arrive at: 1 / (255 std) and -mean / std in float32 arithmetic
IMAGENET_SCALE32 = (0.017124753445386887, 0.017507001757621765, 0.01742919348180294)
IMAGENET_BIAS32 = (-2.1179039478302, -2.0357141494750977, -1.804444432258606)
FOUR_FORMATS = [("uint8", "CHW", "RGB", "reversed"), ("float16", "HWC", "BGR", "file"), ("bfloat16", "CHW", "BGR", "reversed"), ("float32", "HWC", "RGB", "file")]


def _batch(name):
    if name == "three":
        return [golden("q20_0.nhw"), golden("q10_0.nhw"), golden("q20_0.nhw")[:40]], [0, 0, NHW_E_FORMAT]
    if name == "two":
        return [golden("q23_0.nhw"), golden("q01_0.nhw")], [0, 0]
    names = golden_names()[::4]
    assert len(names) == 9
    return [golden(n) for n in names], [0] * 9


# ---------------------------------------------------------------- without a GPU
def test_header_declares_the_format_and_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    for name in ("nhw_tensor_format", "nhw_dec_batch_device_tensor", "nhw_bytes_to_tensor_device", "NHW_T_U8", "NHW_T_F16", "NHW_T_BF16", "NHW_T_F32",
                 "NHW_T_HWC", "NHW_T_CHW", "NHW_T_BGR", "NHW_T_RGB", "NHW_T_ROWS_FILE", "NHW_T_ROWS_REVERSED"):
        assert re.search(rf"\b{name}\b", hdr), name
    values = dict(re.findall(r"\b(NHW_T_[A-Z0-9_]+) = (\d+)", hdr))
    import nhwcodec_amd as na
    assert {k: int(values["NHW_T_" + v]) for k, v in (("uint8", "U8"), ("float16", "F16"), ("bfloat16", "BF16"), ("float32", "F32"))} == na.TENSOR_DTYPES
    assert {"HWC": int(values["NHW_T_HWC"]), "CHW": int(values["NHW_T_CHW"])} == na.TENSOR_LAYOUTS
    assert {"BGR": int(values["NHW_T_BGR"]), "RGB": int(values["NHW_T_RGB"])} == na.TENSOR_CHANNELS
    assert {"file": int(values["NHW_T_ROWS_FILE"]), "reversed": int(values["NHW_T_ROWS_REVERSED"])} == na.TENSOR_ROWS
    struct = re.search(r"typedef struct \{([^}]*)\} nhw_tensor_format;", hdr).group(1)
    assert re.sub(r"\s+", " ", struct).strip() == "int32_t dtype, layout, channels, rows; float scale[3], bias[3]; uint32_t reserved;"
    assert ctypes.sizeof(na.CTensorFormat) == 44
    assert re.search(r"nhw_dec_bmp_header writes a POSITIVE height", hdr) and re.search(r"NHW_T_ROWS_REVERSED is therefore the top-down picture", hdr)


def test_bmp_header_is_bottom_up():
    """what the header comment says about the two row directions rests on this: the height nhw_dec_bmp_header writes is positive"""
    import nhwcodec_amd as na
    h = ctypes.create_string_buffer(54)
    na.load_library().nhw_dec_bmp_header(ctypes.cast(h, ctypes.c_void_p))
    assert int.from_bytes(h.raw[22:26], "little", signed=True) == 512


def test_tensor_format_mean_std_arithmetic():
    import torch
    import nhwcodec_amd as na
    f = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=IMAGENET_MEAN, std=IMAGENET_STD)
    assert f.scale == IMAGENET_SCALE32 and f.bias == IMAGENET_BIAS32
    for c in range(3):                          # the stated constants are the float32 arithmetic, done here a second way
        std, mean = np.float32(IMAGENET_STD[c]), np.float32(IMAGENET_MEAN[c])
        assert np.float32(f.scale[c]) == np.float32(1) / (np.float32(255) * std) and np.float32(f.bias[c]) == -mean / std
    assert f.dtype is torch.float16 and f.dtype_name == "float16" and f.shape(5, 7) == (3, 5, 7)
    c = f.c_struct()
    assert (c.dtype, c.layout, c.channels, c.rows, c.reserved) == (1, 1, 1, 1, 0)
    assert tuple(c.scale) == IMAGENET_SCALE32 and tuple(c.bias) == IMAGENET_BIAS32
    g = na.TensorFormat("float32", "HWC", "BGR", "file", scale=1 / 255, bias=(0, 0.5, -1))
    assert g.scale == (float(np.float32(1 / 255)),) * 3 and g.bias == (0.0, 0.5, -1.0) and g.shape(5, 7) == (5, 7, 3)
    d = na.TensorFormat()
    assert (d.dtype_name, d.layout, d.channels, d.rows, d.scale, d.bias) == ("float32", "CHW", "RGB", "reversed", (1.0,) * 3, (0.0,) * 3)
    assert na.TensorFormat("uint8").scale == (1.0, 1.0, 1.0)
    for name in CONSTANTS:
        check_constants(tensor_format("float32", "CHW", "RGB", "file", name))


@pytest.mark.parametrize("kw", [
    dict(dtype="float64"), dict(dtype="int8"), dict(dtype=None), dict(layout="NCHW"), dict(layout=1), dict(channels="GBR"), dict(rows="top-down"),
    dict(scale=float("inf")), dict(scale=(1, float("nan"), 1)), dict(bias=float("-inf")), dict(bias=(0, 0, 1e39)), dict(scale=(1, 2)), dict(scale="x"),
    dict(mean=(0, 0, 0), std=(1, 0, 1)), dict(mean=float("nan"), std=1), dict(mean=0.5, std=0.2, scale=1), dict(dtype="uint8", scale=2), dict(dtype="uint8", bias=1),
    dict(dtype="uint8", mean=0.5, std=0.5),
])
def test_tensor_format_refuses(kw):
    import nhwcodec_amd as na
    with pytest.raises(na.NhwError):
        na.TensorFormat(**kw)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=16)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("dtype,layout,channels,rows", ALL_FORMATS)
def test_gpu_tensor_three_files_every_format(dec, oracle, dtype, layout, channels, rows, scale):
    """both colour branches and a refused slot, under all 32 formats, bit for bit"""
    files, status = _batch("three")
    fmt = tensor_format(dtype, layout, channels, rows)
    bits, st, qq = decode_tensor(dec, files, fmt, scale)
    assert st.tolist() == status and qq.tolist()[:2] == [20, 10]
    assert_tensor(oracle, bits, files, status, fmt, scale, "three")


def test_the_four_formats_hold_every_enum_value():
    for k, values in enumerate((DTYPES, ("HWC", "CHW"), ("BGR", "RGB"), ("file", "reversed"))):
        assert {f[k] for f in FOUR_FORMATS} == set(values)
    assert len({list(CONSTANTS)[ALL_FORMATS.index(f) % 4] for f in ALL_FORMATS if f[0] != "uint8"}) == 4      # every constant set is used


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("batch", ["two", "nine"])
@pytest.mark.parametrize("k", range(4))
def test_gpu_tensor_other_batches(dec, oracle, batch, k, scale):
    """q23 (the level-1 corrections) and q1 (the low colour matrix); nine files, whose workgroups at scale 4 are no multiple of eight"""
    files, status = _batch(batch)
    fmt = tensor_format(*FOUR_FORMATS[k], constants=list(CONSTANTS)[k])
    bits, st, _ = decode_tensor(dec, files, fmt, scale)
    assert st.tolist() == status
    assert_tensor(oracle, bits, files, status, fmt, scale, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4])
def test_gpu_byte_format_is_the_byte_path_and_u8_chw_its_permutation(dec, scale):
    import torch
    import nhwcodec_amd as na
    files, status = _batch("three")
    s = 512 // scale
    ref = torch.full((3, s, s, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    px, st0, q0 = dec.decode_scaled_device(*device_arena(files), scale, out=ref)
    same, st1, q1 = decode_tensor(dec, files, na.TensorFormat("uint8", "HWC", "BGR", "file"), scale)
    perm, st2, q2 = decode_tensor(dec, files, na.TensorFormat("uint8", "CHW", "RGB", "reversed"), scale)
    torch.cuda.synchronize()
    assert st0.cpu().tolist() == status == st1.tolist() == st2.tolist() and q0.cpu().tolist() == q1.tolist() == q2.tolist()
    px = px.cpu().numpy()
    assert np.array_equal(same, px)
    assert np.array_equal(perm[:2], px[:2, ::-1, :, ::-1].transpose(0, 3, 1, 2)) and (perm[2] == SENTINEL).all()


@pytest.mark.gpu
def test_gpu_one_handle_bytes_and_tensors_in_any_order(oracle):
    """byte -> tensor -> byte -> tensor (another dtype) at mixed scales on ONE handle, a dense batch (white noise) and a sparse one (flat, gradient)
    in turn; each call equals a fresh handle's answer, and the tensors the specification"""
    import torch
    import nhwcodec_amd as na
    enc = na.Encoder(0, 4)
    images = {"dense": np.stack([class_image("noise", s) for s in range(4)]),
              "sparse": np.stack([class_image("flat", 1), class_image("gradient", 2), class_image("black", 0)])}
    batches = {}
    for key, img in images.items():
        out, sizes, status = enc.encode_device(torch.from_numpy(img).cuda(), 20)
        torch.cuda.synchronize()
        ok = [i for i in range(len(img)) if int(status[i]) == 0]       # white noise may overflow the code books: such a slot holds no file
        assert len(ok) >= 2, (key, status.tolist())
        batches[key] = [out[i, : int(sizes[i])].cpu().numpy().tobytes() for i in ok]
    enc.close()
    f16 = tensor_format("float16", "CHW", "RGB", "reversed", "imagenet")
    f32 = tensor_format("float32", "HWC", "BGR", "file", "negative")
    plan = [("dense", 1, None), ("sparse", 2, f16), ("dense", 4, None), ("dense", 1, f32), ("sparse", 1, None), ("dense", 2, f16), ("sparse", 4, f32)]

    def run(d, key, scale, fmt):
        if fmt is None:
            px, st, _ = d.decode_scaled_device(*device_arena(batches[key]), scale)
        else:
            px, st, _ = d.decode_tensor_device(*device_arena(batches[key]), fmt, scale=scale)
        torch.cuda.synchronize()
        assert not bool(st.any())
        return tensor_bits(px)

    one = na.Decoder(0, 4)
    got = [run(one, *step) for step in plan]
    one.close()
    for (key, scale, fmt), g in zip(plan, got):
        fresh = na.Decoder(0, 4)
        want = run(fresh, key, scale, fmt)
        fresh.close()
        assert np.array_equal(g, want), f"{key} at scale {scale}, {fmt}: a reused handle decodes differently from a fresh one"
        for i, f in enumerate(batches[key][:2]):
            px = expected_bytes(oracle, f, scale)
            assert np.array_equal(g[i], px if fmt is None else expected_tensor(px, fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_gpu_tensor_under_forced_slice_orders(dec, oracle, mode):
    """the bands of k_dec_final one per launch, ascending and descending (the orders nhw_dec_debug_slice_order offers): the same tensors"""
    files, status = _batch("three")
    for k, four in enumerate(FOUR_FORMATS):
        fmt = tensor_format(*four, constants=list(CONSTANTS)[k])
        want, st_w, _ = decode_tensor(dec, files, fmt, 1)
        assert dec.lib.nhw_dec_debug_slice_order(dec.h, mode) == 0
        try:
            got, st, _ = decode_tensor(dec, files, fmt, 1)
        finally:
            assert dec.lib.nhw_dec_debug_slice_order(dec.h, 0) == 0
        assert st.tolist() == st_w.tolist() == status
        assert np.array_equal(got, want)
        assert_tensor(oracle, got, files, status, fmt, 1, f"slice order {mode}")


# ---------------------------------------------------------------- what is already bytes
PICTURE_SIZES = [(1, 1), (513, 7), (600, 515)]       # W, H: a single pixel; a width past one row of threads, odd; more rows than a picture's workgroups


def _picture_views(arrangement, fill_seed):
    """the three pictures as views of one device buffer -> (views, their bytes on the host).  The pictures' own bytes depend on the arrangement
    only; what lies between their rows and around them depends on fill_seed.  "pitch": every row padded by 5 .. bytes; "crop": windows of one
    larger picture, starting at an odd byte offset"""
    import torch
    rng = np.random.default_rng(17)
    own = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in PICTURE_SIZES]
    host = np.random.default_rng(fill_seed).integers(0, 256, 4 << 20, dtype=np.uint8)
    at, places = 1, []                                                   # (offset, pitch)
    if arrangement == "pitch":
        for (w, h), px in zip(PICTURE_SIZES, own):
            pitch = 3 * w + 5 + 2 * len(places)
            places.append((at, pitch))
            at = (at + h * pitch + 7) | 1
    else:
        big_w = 700
        for (w, h), px in zip(PICTURE_SIZES, own):
            places.append((at + 3 * 12 * len(places), 3 * big_w))      # from column 12 k of a 700-wide picture that starts at an odd address
            at = (at + h * 3 * big_w) | 1
    for (off, pitch), (w, h), px in zip(places, PICTURE_SIZES, own):
        for r in range(h):
            host[off + r * pitch: off + r * pitch + 3 * w] = px[r].reshape(-1)
    buf = torch.from_numpy(host).cuda()
    views = [buf.as_strided((h, w, 3), (pitch, 3, 1), off) for (off, pitch), (w, h) in zip(places, PICTURE_SIZES)]
    assert all(v.data_ptr() % 2 == 1 for v in views)
    return views, own


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement", ["pitch", "crop"])
def test_gpu_pictures_to_tensor(arrangement):
    """1 x 1, 513 x 7 and 600 x 515 in one table, under all 32 formats, against the CPU rule on the pictures' bytes; the bytes between the rows and
    beyond the pictures play no part: another filling gives the same tensors"""
    import torch
    import nhwcodec_amd as na
    views, own = _picture_views(arrangement, 1)
    other, own2 = _picture_views(arrangement, 2)
    assert all(np.array_equal(a, b) for a, b in zip(own, own2))
    for four in ALL_FORMATS:
        fmt = tensor_format(*four)
        got = na.pictures_to_tensor_device(views, fmt)
        again = na.pictures_to_tensor_device(other, fmt)
        torch.cuda.synchronize()
        for (w, h), px, g, g2 in zip(PICTURE_SIZES, own, got, again):
            assert g.dtype == fmt.dtype and tuple(g.shape) == fmt.shape(h, w)
            bits, want = tensor_bits(g), expected_tensor(px, fmt)
            assert np.array_equal(bits, want), f"{fmt} {w} x {h}: {int((bits != want).sum())} elements differ"
            assert np.array_equal(tensor_bits(g2), want)


@pytest.mark.gpu
def test_gpu_bytes_to_tensor_writes_only_the_tensors(dec):
    """the C entry on tensors laid into a sentinel-filled buffer with gaps: nothing outside a tensor's H * W * 3 elements is written, and an
    entry whose address is no multiple of the element size is passed over"""
    import torch
    import nhwcodec_amd as na
    views, own = _picture_views("pitch", 3)
    table, _, dev = na._picture_table(views, "test")
    for four in FOUR_FORMATS:
        fmt = tensor_format(*four)
        es = fmt.dtype.itemsize
        sizes = [3 * w * h * es for w, h in PICTURE_SIZES]
        offs, at = [], 64
        for sz in sizes:
            offs.append(at)
            at += sz + 64 + (-sz % 16)
        buf = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
        for misalign in ((0, 0, 0), (0, 1, 0)) if es > 1 else ((0, 0, 0),):
            buf.fill_(SENTINEL)
            addr = torch.tensor([buf.data_ptr() + o + m for o, m in zip(offs, misalign)], dtype=torch.int64, device="cuda")
            c = fmt.c_struct()
            assert dec.lib.nhw_bytes_to_tensor_device(table.data_ptr(), 3, ctypes.byref(c), addr.data_ptr(), None) == 0
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            mask = np.ones(at, bool)
            for o, sz, m, px in zip(offs, sizes, misalign, own):
                if m:
                    continue                                             # passed over: its bytes stay sentinel
                mask[o:o + sz] = False
                assert np.array_equal(host[o:o + sz], expected_tensor(px, fmt).reshape(-1).view(np.uint8)), fmt
            assert (host[mask] == SENTINEL).all(), f"{fmt}: bytes outside the tensors were written"


# ---------------------------------------------------------------- refusals
def _c_format(**kw):
    import nhwcodec_amd as na
    c = na.TensorFormat("float32", "CHW", "RGB", "reversed").c_struct()
    for k, v in kw.items():
        if k in ("scale", "bias"):
            getattr(c, k)[1] = v
        else:
            setattr(c, k, v)
    return c


REFUSED_FORMATS = [dict(scale=float("inf")), dict(scale=float("nan")), dict(bias=float("-inf")), dict(bias=float("nan")),
                   dict(dtype=4), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(channels=2), dict(rows=2), dict(rows=-1), dict(reserved=1),
                   dict(dtype=0, scale=2.0), dict(dtype=0, bias=1.0)]


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing(dec):
    """every NHW_E_ARG case of the format and of the entry point: the call returns before any launch, so the output, the status and the quality
    stay at their sentinel"""
    import torch
    files, _ = _batch("two")
    arena, offs, lens = device_arena(files)
    out = torch.full((2 * 3 * 512 * 512 * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    qq = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 16 == 0

    def call(c, scale=1, shift=0, n=2):
        rc = dec.lib.nhw_dec_batch_device_tensor(dec.h, arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, scale, ctypes.byref(c) if c is not None else None,
                                                 out.data_ptr() + shift, st.data_ptr(), qq.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((out == SENTINEL).all()) and bool((st == 0x5A5A5A5A).all()) and bool((qq == 0x5A5A5A5A).all())

    for kw in REFUSED_FORMATS:
        assert call(_c_format(**kw)) == NHW_E_ARG, kw
        assert dec.lib.nhw_dec_last_error()
        assert untouched(), kw
    good = _c_format()
    byte_format = _c_format(dtype=0, layout=0, channels=0, rows=0)
    assert call(None) == NHW_E_ARG and untouched()
    for shift in (1, 2, 4, 8):
        assert call(good, shift=shift) == NHW_E_ARG and untouched(), shift
        assert call(byte_format, shift=shift) == NHW_E_ARG and untouched(), shift
    for scale in (0, 3, 8, -1):
        assert call(good, scale=scale) == NHW_E_ARG and untouched(), scale
    assert call(good, n=0) == NHW_E_ARG and call(good, n=dec.max_batch + 1) == NHW_E_ARG and untouched()
    for scale in (1, 2, 4):                                             # a debug stop on the handle, at every scale, the byte format too
        dec.lib.nhw_dec_debug_stop_after(dec.h, 4)
        try:
            assert call(good, scale=scale) == NHW_E_ARG and call(byte_format, scale=scale) == NHW_E_ARG
        finally:
            dec.lib.nhw_dec_debug_stop_after(dec.h, 0)
        assert untouched(), scale
    # the pointwise entry refuses the same formats
    import nhwcodec_amd as na
    views, _ = _picture_views("pitch", 4)
    table, _, _ = na._picture_table(views, "test")
    addr = torch.tensor([out.data_ptr() + 16 + 4096 * k for k in range(3)], dtype=torch.int64, device="cuda")
    for kw in REFUSED_FORMATS:
        c = _c_format(**kw)
        assert dec.lib.nhw_bytes_to_tensor_device(table.data_ptr(), 3, ctypes.byref(c), addr.data_ptr(), None) == NHW_E_ARG, kw
    assert dec.lib.nhw_bytes_to_tensor_device(table.data_ptr(), 0, ctypes.byref(good), addr.data_ptr(), None) == NHW_E_ARG
    assert dec.lib.nhw_bytes_to_tensor_device(None, 3, ctypes.byref(good), addr.data_ptr(), None) == NHW_E_ARG
    assert dec.lib.nhw_bytes_to_tensor_device(table.data_ptr(), 3, ctypes.byref(good), None, None) == NHW_E_ARG
    torch.cuda.synchronize()
    assert untouched()
    assert call(good) == 0 and not untouched()                          # ... and the same call with nothing wrong does run


@pytest.mark.gpu
def test_gpu_python_argument_errors(dec):
    import torch
    import nhwcodec_amd as na
    files, _ = _batch("two")
    a = device_arena(files)
    fmt = na.TensorFormat("float32", "CHW", "RGB", "reversed")
    room = 2 * 3 * 512 * 512
    buf = torch.full((room + 8,), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(na.NhwError, match="16-byte aligned"):
        dec.decode_tensor_device(*a, fmt, out=buf[1:])                  # 4 bytes off
    with pytest.raises(na.NhwError, match="float32"):
        dec.decode_tensor_device(*a, fmt, out=buf.to(torch.float16))    # the wrong dtype
    with pytest.raises(na.NhwError):
        dec.decode_tensor_device(*a, fmt, out=buf[:room - 1])           # too small
    with pytest.raises(na.NhwError):
        dec.decode_tensor_device(*a, fmt, scale=3)
    with pytest.raises(na.NhwError, match="TensorFormat"):
        dec.decode_tensor_device(*a, "float32")
    with pytest.raises(na.NhwError, match="TensorFormat"):
        na.pictures_to_tensor_device([torch.zeros((2, 2, 3), dtype=torch.uint8, device="cuda")], None)
    with pytest.raises(na.NhwError):
        na.pictures_to_tensor_device([], fmt)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
