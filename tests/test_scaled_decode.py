"""Decode at half or quarter scale straight from the wavelet pyramid: the definition, k_dec_scaled<2> / <4>, the
scaled crop (k_untile_crop on tiles of 256 / 128), nhw_dec_batch_device_scaled / nhw_dec_batch_scaled / nhw_dec_pictures_scaled /
nhw_untile_pictures_scaled_device / nhw_picture_scaled_size, their Python wrappers and nhw-dec --scale.

The reference has no such mode; the expected pictures are built here from the oracle decoder's intermediate planes (the probe() calls of
oracle/nhwo_dec.c) and the oracle's own colour matrix (nhwo_dec_color of liboracle.so):
  scale 2: Y = clip8(probe 6, the level-1 LL after the residual lists), U, V = probes 46, 47 (the sharpened, clipped 4:2:0 planes);
  scale 4: Y = clip8(probe 4's level-2 LL quadrant, TRANSPOSED), U, V = clip8(probes 42, 43's quadrant: level 2 + corrections).
Every output byte of the GPU must equal them.  The construction itself is tests/tensor_cases.py's expected(): other modules hold their
scaled decodes against it too."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from oracle.harness import class_image
from tests.picture_cases import parse_container
from tests.support import CANARY, ROOT, built_cli, device_arena, golden, golden_names, load_lib, psnr, run
from tests.tensor_cases import decode_scaled, expected, expected_planes

NEW_SYMBOLS = ("nhw_dec_batch_device_scaled", "nhw_dec_batch_scaled", "nhw_picture_scaled_size", "nhw_untile_pictures_scaled_device",
               "nhw_dec_pictures_scaled")
PROTOTYPES = """
int nhw_dec_batch_device_scaled(nhw_dec *d, const void *d_nhw, const uint64_t *d_off, const uint32_t *d_len, int n, int scale, void *d_out,
                                int32_t *d_status, int32_t *d_quality, void *stream);
int nhw_dec_batch_scaled(nhw_dec *d, const uint8_t *nhw, const uint64_t *off, int n, int scale, uint8_t *out, int32_t *status, int32_t *quality);
int nhw_picture_scaled_size(uint32_t width, uint32_t height, int scale, uint32_t *scaled_width, uint32_t *scaled_height);
int nhw_untile_pictures_scaled_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int n_tiles, int scale, void *stream);
int nhw_dec_pictures_scaled(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n, int scale, uint8_t *out, const uint64_t *out_off, int32_t *status);
"""
NHW_E_ARG, NHW_E_FORMAT = -4, -6


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def cli():
    return built_cli("nhw-dec")


def expected_picture(oracle, container, scale):
    """the scaled picture of a container: the per-tile expected pictures side by side, cropped to ceil(W / s) x ceil(H / s)"""
    w, h, files = parse_container(container)
    t, nx, ny = 512 // scale, -(-w // 512), -(-h // 512)
    full = np.empty((ny * t, nx * t, 3), np.uint8)
    for k, f in enumerate(files):
        full[(k // nx) * t:(k // nx + 1) * t, (k % nx) * t:(k % nx + 1) * t] = expected(oracle, f, scale)
    return full[:-(-h // scale), :-(-w // scale)]


# ---------------------------------------------------------------- without a GPU
def _box(a, s):
    return a.astype(np.float64).reshape(a.shape[0] // s, s, a.shape[1] // s, s).mean(axis=(1, 3))


@pytest.mark.parametrize("q", [1, 10, 20, 23])
def test_definition_orientation_tripwire(oracle, q):
    """An orientation check, not a quality claim: the expected small planes against the box means of the oracle's full-decode planes.  With the
    right orientation scale-2 Y comes out at 44 dB or more, the scale-4 planes at 36 dB or more; transposed, all are at 25.5 dB or less (measured on
    the CPU on this image at these qualities).  The thresholds sit between the two groups."""
    nhw = oracle.encode(oracle.synth(3), q)
    planes, qq = oracle.decode(nhw, planes=True)
    assert qq == q
    y2, u2, v2, _ = expected_planes(oracle, nhw, 2)
    y4, u4, v4, _ = expected_planes(oracle, nhw, 4)
    figures = {"Y2": psnr(y2, _box(planes[0], 2)), "Y4": psnr(y4, _box(planes[0], 4)), "U4": psnr(u4, _box(planes[1], 4)), "V4": psnr(v4, _box(planes[2], 4))}
    wrong = {"Y2": psnr(y2.T, _box(planes[0], 2)), "Y4": psnr(y4.T, _box(planes[0], 4))}
    print(f"q{q}: " + ", ".join(f"{k} {v:.1f} dB" for k, v in figures.items()) + " | transposed: " + ", ".join(f"{k} {v:.1f} dB" for k, v in wrong.items()))
    assert figures["Y2"] >= 35.0, figures
    assert min(figures["Y4"], figures["U4"], figures["V4"]) >= 30.0, figures
    for c, p in enumerate((u2, v2)):
        assert np.array_equal(p, planes[1 + c][::2, ::2]), f"scale-2 chroma plane {c} is not the full decode's plane at every second sample"


def test_scaled_size_rule():
    import nhwcodec_amd as na
    for s in (1, 2, 4):
        t = 512 // s
        for w in (1, 2, 3, 4, 511, 512, 513, 65535):
            sw, sh = na.scaled_size(w, 7, s)
            assert sw == -(-w // s) and sh == -(-7 // s)
            assert na.scaled_size(7, w, s) == (-(-7 // s), sw)
            assert -(-sw // t) == -(-w // 512), (w, s)           # as many tiles as the whole picture
    for bad in ((0, 5, 2), (5, 0, 2), (65536, 5, 2), (5, 65536, 4), (5, 5, 3), (5, 5, 0), (5, 5, 8), (5, 5, 2.0), (5, 5, True)):
        with pytest.raises(na.NhwError):
            na.scaled_size(*bad)


def test_scaled_size_c_abi(lib):
    lib.nhw_picture_scaled_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    for s in (1, 2, 4):
        for side in (1, 2, 3, 4, 511, 512, 513, 65535):
            assert lib.nhw_picture_scaled_size(side, 65535 - side + 1, s, ctypes.byref(w), ctypes.byref(h)) == 0
            assert (w.value, h.value) == (-(-side // s), -(-(65535 - side + 1) // s))
    for bad in ((0, 5, 2), (5, 0, 2), (65536, 5, 2), (5, 65536, 2), (5, 5, 3), (5, 5, 0), (5, 5, -2)):
        assert lib.nhw_picture_scaled_size(*bad, ctypes.byref(w), ctypes.byref(h)) == NHW_E_ARG
    assert lib.nhw_picture_scaled_size(5, 5, 2, None, ctypes.byref(h)) == NHW_E_ARG


def test_scaled_symbols_and_prototypes(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    hdr = squeeze(open(os.path.join(ROOT, "include", "nhw_hip.h")).read())
    decls = re.split(r"\n(?=int )", PROTOTYPES.strip())
    assert len(decls) == 5
    for decl in decls:
        assert squeeze(decl) in hdr, decl
    import nhwcodec_amd as na
    for name in ("scaled_size", "untile_scaled_pictures_device"):
        assert callable(getattr(na, name))
    for name in ("decode_scaled_device", "decode_scaled", "decode_pictures_scaled"):
        assert callable(getattr(na.Decoder, name))


@pytest.mark.parametrize("args", [
    ("--scale",),
    ("in.nhw", "out.bmp", "--scale"),
    ("--scale", "3", "in.nhw", "out.bmp"),
    ("--scale", "x", "in.nhw", "out.bmp"),
    ("--scale", "22", "in.nhw", "out.bmp"),
    ("--scale=2", "in.nhw", "out.bmp"),
    ("--scale", "2", "--picture", "in.nhwp", "out.bmp", "--region", "0,0,8,8"),
    ("--picture", "in.nhwp", "out.bmp", "--region", "0,0,8,8", "--scale", "2"),
])
def test_cli_refuses_a_bad_scale_before_any_gpu_work(cli, tmp_path, args):
    """refused like a malformed --region: exit 1 with a message on stderr, no file read, none written, the GPU never opened (this runs without one)"""
    args = tuple(str(tmp_path / a) if a.endswith((".nhw", ".nhwp", ".bmp")) else a for a in args)
    rc, out, err = run(cli, *args)
    assert rc == 1 and "--scale" in err and out == "", (rc, out, err)
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=64)
    yield d
    d.close()


def _assert_pictures(oracle, got, files, scale, names=None, only=None):
    bad = []
    for i, f in enumerate(files):
        if only is not None and i not in only:
            continue
        want = expected(oracle, f, scale)
        if not np.array_equal(got[i], want):
            bad.append((names[i] if names else i, int((got[i] != want).sum())))
    assert not bad, f"scale {scale}: (file, differing bytes) {bad[:8]} of {len(files)}"


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
def test_gpu_scaled_every_quality_one_mixed_batch(dec, oracle, scale):
    """the 34 committed files (q1 .. 23, every colour branch, every residual list) in one call: every output byte"""
    names = golden_names()
    assert len(names) == 34
    files = [golden(n) for n in names]
    px, st, qq = decode_scaled(dec, files, scale)
    assert not st.any()
    assert qq.tolist() == [int(n[1:3]) for n in names]
    _assert_pictures(oracle, px, files, scale, names)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("name", ["q20_0.nhw", "q10_0.nhw"])
def test_gpu_scaled_single_file(dec, oracle, scale, name):
    f = golden(name)
    px, st, qq = decode_scaled(dec, [f], scale)
    assert st.tolist() == [0] and qq.tolist() == [int(name[1:3])]
    _assert_pictures(oracle, px, [f], scale, [name])


@pytest.mark.gpu
def test_gpu_scale_1_is_the_full_decode(dec):
    import torch
    files = [golden(n) for n in golden_names()]
    a = device_arena(files)
    px1, st1, q1 = dec.decode_scaled_device(*a, 1)
    px, st, q = dec.decode_device(*a)
    torch.cuda.synchronize()
    assert tuple(px1.shape) == (len(files), 512, 512, 3)
    assert torch.equal(px1, px) and torch.equal(st1, st) and torch.equal(q1, q)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
def test_gpu_scaled_refused_files_and_good_neighbours(dec, oracle, scale):
    """a truncated, a zero-filled and a foreign file among good ones: status and quality as the full decode reports them, a refused file's bytes
    untouched, every good neighbour byte-exact"""
    import torch
    good, other = golden("q20_0.nhw"), golden("q10_0.nhw")
    files = [good, good[:40], other, bytes(3000), bytes([9, 20]) + good[2:], good[: len(good) // 2], golden("q23_0.nhw"), good]
    a = device_arena(files)
    _, st_full, q_full = dec.decode_device(*a)
    torch.cuda.synchronize()
    px, st, qq = decode_scaled(dec, files, scale)
    assert st.tolist() == st_full.cpu().tolist() == [0, NHW_E_FORMAT, 0, NHW_E_FORMAT, NHW_E_FORMAT, NHW_E_FORMAT, 0, 0]
    assert qq.tolist() == q_full.cpu().tolist()
    _assert_pictures(oracle, px, files, scale, only={0, 2, 6, 7})
    for i in (1, 3, 4, 5):
        assert (px[i] == CANARY).all(), f"refused file {i}: its output bytes were written"


@pytest.mark.gpu
def test_gpu_one_handle_full_and_scaled_in_any_order(oracle):
    """full decode of a dense batch (white noise: nearly every group of the detail bands in memory), scale 4 of a sparse one (flat, gradient:
    whole bands left out of the plane), scale 2 of the dense one, the full decode again -- on ONE handle; each equals a fresh handle's answer,
    and the scaled ones the expected pictures.  The workspace is shared: plane A, the group map, plane_l1 and the chroma planes of the batch
    before are all still there."""
    import torch
    import nhwcodec_amd as na
    enc = na.Encoder(0, 8)
    dense_img = np.stack([class_image("noise", s) for s in range(5)])
    sparse_img = np.stack([class_image("flat", 1), class_image("gradient", 2), class_image("flat", 3), class_image("gradient", 4), class_image("black", 0)])
    batches = {}
    for key, img, q in (("dense", dense_img, 20), ("sparse", sparse_img, 20)):
        out, sizes, status = enc.encode_device(torch.from_numpy(img).cuda(), q)
        torch.cuda.synchronize()
        ok = [i for i in range(len(img)) if int(status[i]) == 0]       # white noise may overflow the code books: such a slot holds no file
        assert len(ok) >= 3, (key, status.tolist())
        batches[key] = [out[i, : int(sizes[i])].cpu().numpy().tobytes() for i in ok]
    enc.close()
    plan = [("dense", 1), ("sparse", 4), ("dense", 2), ("dense", 1), ("sparse", 2), ("dense", 4)]

    def run(d, key, scale):
        px, st, qq = d.decode_scaled_device(*device_arena(batches[key]), scale)
        torch.cuda.synchronize()
        assert not bool(st.any())
        return px.cpu().numpy()

    one = na.Decoder(0, 8)
    got = [run(one, key, scale) for key, scale in plan]
    one.close()
    for (key, scale), g in zip(plan, got):
        fresh = na.Decoder(0, 8)
        want = run(fresh, key, scale)
        fresh.close()
        assert np.array_equal(g, want), f"{key} at scale {scale}: a reused handle decodes differently from a fresh one"
        if scale == 1:
            for i, f in enumerate(batches[key][:2]):
                assert np.array_equal(g[i], oracle.decode(f)[0])
        else:
            _assert_pictures(oracle, g, batches[key], scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1, 2, 4])
def test_gpu_scaled_host_path_is_chunked(oracle, scale):
    """decode_scaled of 5 files on a handle of max_batch 2: three chunks"""
    import nhwcodec_amd as na
    names = ["q20_0.nhw", "q10_gradient.nhw", "q23_tiles.nhw", "q01_0.nhw", "q17_0.nhw"]
    files = [golden(n) for n in names]
    d = na.Decoder(0, max_batch=2)
    try:
        px, qs = d.decode_scaled(files, scale)
        with pytest.raises(na.NhwError):
            d.decode_scaled(files + [bytes(100)], scale)
        with pytest.raises(na.NhwError):
            d.decode_scaled(files, 3)
    finally:
        d.close()
    assert px.shape == (5, 512 // scale, 512 // scale, 3) and qs == [int(n[1:3]) for n in names]
    if scale == 1:
        for i, f in enumerate(files):
            assert np.array_equal(px[i], oracle.decode(f)[0])
    else:
        _assert_pictures(oracle, px, files, scale, names)


PICTURES = [(1, 1, 20), (2, 3, 20), (513, 511, 20), (1025, 5, 20), (700, 1030, 20), (513, 511, 10)]   # W, H, quality


@pytest.fixture(scope="module")
def containers(oracle):
    """the test pictures (crops of a 3 x 3 mosaic of generator images) as .nhwp containers"""
    import nhwcodec_amd as na
    mosaic = np.concatenate([np.concatenate([oracle.synth(40 + 3 * r + c) for c in range(3)], axis=1) for r in range(3)], axis=0)
    enc = na.Encoder(0, 8)
    out = []
    for w, h, q in PICTURES:
        out.append(enc.encode_pictures([np.ascontiguousarray(mosaic[100:100 + h, 200:200 + w])], q)[0])
    enc.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
def test_gpu_scaled_pictures(oracle, containers, scale):
    """decode_pictures_scaled (chunked: max_batch 4 against 15 tiles) equals the per-tile expected pictures side by side, cropped"""
    import nhwcodec_amd as na
    d = na.Decoder(0, max_batch=4)
    try:
        got = d.decode_pictures_scaled(containers, scale)
        with pytest.raises(na.NhwError):
            d.decode_pictures_scaled(containers, 3)
        with pytest.raises(na.NhwError):
            d.decode_pictures_scaled([containers[0][:-1]], scale)
    finally:
        d.close()
    for (w, h, q), c, g in zip(PICTURES, containers, got):
        assert g.shape == (-(-h // scale), -(-w // scale), 3) == (*na.scaled_size(w, h, scale)[::-1], 3)
        want = expected_picture(oracle, c, scale)
        assert np.array_equal(g, want), f"{w} x {h} q{q} at scale {scale}: {int((g != want).sum())} bytes differ"


@pytest.mark.gpu
def test_gpu_scale_1_pictures_are_decode_pictures(containers):
    import nhwcodec_amd as na
    d = na.Decoder(0, max_batch=4)
    try:
        a, b = d.decode_pictures_scaled(containers, 1), d.decode_pictures(containers)
    finally:
        d.close()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
def test_gpu_untile_scaled_writes_only_the_pictures_bytes(oracle, containers, scale):
    """untile_scaled_pictures_device into pitch views of a larger canary-filled tensor, at odd byte offsets: the pictures' own bytes and no other"""
    import torch
    import nhwcodec_amd as na
    t = 512 // scale
    files = [f for c in containers for f in parse_container(c)[2]]
    d = na.Decoder(0, max_batch=len(files))
    tiles, st, _ = d.decode_scaled_device(*device_arena(files), scale)
    torch.cuda.synchronize()
    d.close()
    assert not bool(st.any()) and tuple(tiles.shape) == (len(files), t, t, 3)
    sizes = [na.scaled_size(w, h, scale) for w, h, _ in PICTURES]
    rows = sum(h for _, h in sizes) + 2 * len(sizes) + 2
    pitch = 3 * max(w for w, _ in sizes) + 37
    canvas = torch.full((rows, pitch), CANARY, dtype=torch.uint8, device="cuda")
    views, mask, at = [], np.zeros((rows, pitch), bool), 1
    for k, (w, h) in enumerate(sizes):
        x0 = 1 + 5 * k                                               # odd and even byte phases
        views.append(canvas[at:at + h, x0:x0 + 3 * w].unflatten(1, (w, 3)))
        mask[at:at + h, x0:x0 + 3 * w] = True
        at += h + 2
    na.untile_scaled_pictures_device(tiles, views, scale)
    torch.cuda.synchronize()
    host = canvas.cpu().numpy()
    assert (host[~mask] == CANARY).all(), "a byte outside the pictures was written"
    for c, v, (w, h, q) in zip(containers, views, PICTURES):
        assert np.array_equal(v.cpu().numpy(), expected_picture(oracle, c, scale)), f"{w} x {h} q{q}"
    with pytest.raises(na.NhwError):
        na.untile_scaled_pictures_device(tiles, views, 3)
    with pytest.raises(na.NhwError):
        na.untile_scaled_pictures_device(tiles[:-1], views, scale)


@pytest.mark.gpu
def test_gpu_scaled_call_with_a_debug_stop_is_refused(oracle):
    import nhwcodec_amd as na
    d = na.Decoder(0, max_batch=2)
    try:
        d.lib.nhw_dec_debug_stop_after(d.h, 4)
        with pytest.raises(na.NhwError):
            d.decode_scaled_device(*device_arena([golden("q20_0.nhw")]), 2)
        d.lib.nhw_dec_debug_stop_after(d.h, 0)
        px, st, _ = d.decode_scaled_device(*device_arena([golden("q20_0.nhw")]), 2)
        assert np.array_equal(px[0].cpu().numpy(), expected(oracle, golden("q20_0.nhw"), 2))
        with pytest.raises(na.NhwError):
            d.decode_scaled_device(*device_arena([golden("q20_0.nhw")] * 3), 2)      # more files than max_batch
    finally:
        d.close()


def _bmp_header(dec, w, h):
    """the decoder's 54 bytes with the size fields of a w x h picture, rows padded to 4 bytes"""
    hdr = bytearray(dec.bmp_header())
    size = ((3 * w + 3) & ~3) * h
    struct.pack_into("<I", hdr, 2, size + 54)
    struct.pack_into("<II", hdr, 18, w, h)
    struct.pack_into("<I", hdr, 34, size)
    return bytes(hdr)


@pytest.mark.gpu
def test_gpu_cli_scale(dec, oracle, cli, containers, tmp_path):
    """nhw-dec --scale 2 on one file: the header of a 256 x 256 BMP and the expected bytes; --scale 1 is the plain call; --batch --scale 4;
    --picture --scale 4 on the 513 x 511 container"""
    f = golden("q20_0.nhw")
    src = tmp_path / "a.nhw"
    src.write_bytes(f)
    rc, out, err = run(cli, "--scale", "2", str(src), str(tmp_path / "a2.bmp"))
    assert rc == 0, (out, err)
    assert (tmp_path / "a2.bmp").read_bytes() == _bmp_header(dec, 256, 256) + expected(oracle, f, 2).tobytes()
    assert run(cli, str(src), str(tmp_path / "a1.bmp"), "--scale", "1")[0] == 0 and run(cli, str(src), str(tmp_path / "a0.bmp"))[0] == 0
    assert (tmp_path / "a1.bmp").read_bytes() == (tmp_path / "a0.bmp").read_bytes() == dec.bmp_header() + oracle.decode(f)[0].tobytes()
    bdir = tmp_path / "batch"
    bdir.mkdir()
    for n in ("q10_0.nhw", "q23_0.nhw"):
        (bdir / n).write_bytes(golden(n))
    rc, out, err = run(cli, "--batch", str(bdir), "--scale", "4")
    assert rc == 0 and "2 file(s) decoded" in out, (out, err)
    for n in ("q10_0", "q23_0"):
        assert (bdir / (n + ".bmp")).read_bytes() == _bmp_header(dec, 128, 128) + expected(oracle, golden(n + ".nhw"), 4).tobytes()
    c = containers[2]
    (tmp_path / "p.nhwp").write_bytes(c)
    rc, out, err = run(cli, "--picture", "--scale", "4", str(tmp_path / "p.nhwp"), str(tmp_path / "p4.bmp"))
    assert rc == 0 and "129 x 128 picture" in out, (out, err)
    want = expected_picture(oracle, c, 4)
    rows = b"".join(want[r].tobytes() + bytes(-3 * 129 % 4) for r in range(128))
    assert (tmp_path / "p4.bmp").read_bytes() == _bmp_header(dec, 129, 128) + rows
