"""Encode grey on the GPU: the grey source forms of the front kernels and of the colour kernel, the one-channel tensor and
tile-pad kernels, the host and Python layers and nhw-enc --grey.  Everything expected is the oracle's file of the picture with every grey byte in
B, G and R (tests/grey_encode_cases.oracle_file), never the code under test.  A 512 x 512 picture is the codec's unit; the batches are the smallest
that reach each path (n = 3; n = 517 where sub-batches start at 512)."""
import ctypes
import os

import numpy as np
import pytest

from tests.grey_encode_cases import (GREY_BYTES, NHW_E_ARG, NHW_E_QUALITY, NP_BITS, SEEDS, all_greys, files_of, oracle_file, pad_tiles, replicated, rule_bytes,
                                     synth_grey, to_bits, to_device, widen)
from tests.support import built_cli, run

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096


@pytest.fixture(scope="module")
def enc():
    import nhwcodec_amd
    e = nhwcodec_amd.Encoder(0, max_batch=4)
    yield e
    e.close()


def _three():
    return np.stack([synth_grey(SEEDS[0]), synth_grey(SEEDS[1]), all_greys()])


@pytest.mark.parametrize("q", list(range(1, 24)))
def test_every_quality(enc, oracle, q):
    """all four colour families, both fused kernels and the grey colour kernel: files, sizes and status are the oracle's"""
    import torch
    g = _three()
    files, status = files_of(*enc.encode_grey_device(torch.from_numpy(g).cuda(), q))
    assert status == [0, 0, 0]
    for i in range(3):
        assert files[i] == oracle_file(oracle, g[i], q), f"q{q} picture {i}: {len(files[i])} bytes for {len(oracle_file(oracle, g[i], q))}"
    if q in (10, 20):
        assert enc.encode_grey(g, q) == files                              # the host path


@pytest.mark.parametrize("q", [13, 20])
def test_compatibility_mode(oracle, q):
    """the grey colour kernel's replay behind the fused kernel (q 20) and the low path (q 13) against the oracle's stock-binary mode"""
    import torch
    import nhwcodec_amd
    e = nhwcodec_amd.Encoder(0, max_batch=3)
    e.set_compat(True)
    g = _three()
    files, status = files_of(*e.encode_grey_device(torch.from_numpy(g).cuda(), q))
    e.close()
    assert status == [0, 0, 0]
    for i in range(3):
        assert files[i] == oracle_file(oracle, g[i], q, compat=True), f"q{q} picture {i}"


def test_one_handle_any_order(oracle):
    """grey, colour, grey on one handle in one stream, with n = max_batch and below it: the colour files are what they are without the grey calls
    (no chroma plane of 128s left standing), the grey files the oracle's"""
    import torch
    import nhwcodec_amd
    e = nhwcodec_amd.Encoder(0, max_batch=3)
    g = _three()
    colour = np.stack([oracle.synth(s) for s in SEEDS[:3]])
    d_g, d_c = torch.from_numpy(g).cuda(), torch.from_numpy(colour).cuda()
    for q in (20, 10):
        for n_grey, n_col in ((3, 3), (2, 3), (3, 2)):
            a = files_of(*e.encode_grey_device(d_g[:n_grey], q))
            b = files_of(*e.encode_device(d_c[:n_col], q))
            c = files_of(*e.encode_grey_device(d_g[:n_grey], q))
            assert a == c and a[1] == [0] * n_grey and b[1] == [0] * n_col
            assert a[0] == [oracle_file(oracle, g[i], q) for i in range(n_grey)], (q, n_grey)
            assert b[0] == [oracle.encode(colour[i], q) for i in range(n_col)], (q, n_col)
    e.close()


DTYPES = ["uint8", "float16", "bfloat16", "float32"]
_RANDOM = {}


def _random_batch(dtype):
    """two pictures of random elements [2, 512, 512] as bit patterns, the format's constants, and the rule's bytes in tensor row order"""
    if dtype not in _RANDOM:
        rng = np.random.default_rng(77 + DTYPES.index(dtype))
        if dtype == "uint8":
            bits, sc, bi = rng.integers(0, 256, (2, 512, 512), dtype=np.uint8), 1.0, 0.0
            t = bits
        else:
            sc, bi = float(np.float32(rng.uniform(200, 300))), float(np.float32(rng.uniform(-20, 20)))   # on x in -0.15 .. 1.25: both clamps fire
            bits = to_bits(rng.random((2, 512, 512), dtype=np.float32) * np.float32(1.4) - np.float32(0.15), dtype)
            t = rule_bytes(widen(bits, dtype), sc, bi)
            assert (t == 0).mean() > 0.02 and (t == 255).mean() > 0.02
        _RANDOM[dtype] = (bits, sc, bi, t)
    return _RANDOM[dtype]


def _grey_bytes_guarded(lib, x, fmt):
    import torch
    n = x.shape[0]
    buf = torch.full((GUARD + n * GREY_BYTES + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + n * GREY_BYTES]
    c = fmt.c_struct()
    assert lib.nhw_tensor_to_bytes_grey_device(x.data_ptr(), n, ctypes.byref(c), out.data_ptr(), None) == 0, lib.nhw_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n * GREY_BYTES:] == SENTINEL).all()), f"{fmt}: bytes outside n * 262144 were written"
    return out.cpu().numpy().reshape(n, 512, 512)


@pytest.mark.parametrize("rows", ["file", "reversed"])
@pytest.mark.parametrize("layout", ["CHW", "HWC"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensors(enc, dtype, layout, rows):
    import torch
    import nhwcodec_amd as na
    bits, sc, bi, t = _random_batch(dtype)
    fmt = na.TensorFormat(dtype, layout, "GREY", rows, **({} if dtype == "uint8" else dict(scale=sc, bias=bi)))
    x = to_device(bits.reshape((2,) + fmt.shape(512, 512)), dtype)
    want = t[:, ::-1] if rows == "reversed" else t
    got = _grey_bytes_guarded(enc.lib, x, fmt)
    bad = got != want
    assert not bad.any(), f"{fmt}: {int(bad.sum())} bytes differ, first at {tuple(np.argwhere(bad)[0])}"
    py = na.tensor_to_grey_bytes_device(x, fmt)
    assert py.dtype == torch.uint8 and tuple(py.shape) == (2, 512, 512) and np.array_equal(py.cpu().numpy(), got)
    assert files_of(*enc.encode_grey_tensor_device(x, fmt, 20)) == files_of(*enc.encode_grey_device(py, 20))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_special_values(enc, dtype):
    """exact ties under scale 1 (to even), signed zeros, NaNs of both signs, infinities, the largest finite values, out of range"""
    import torch
    import nhwcodec_amd as na
    fin = float(torch.finfo(getattr(torch, dtype)).max)
    x32 = np.zeros((1, 512, 512), np.float32)
    hand = {}
    holds = lambda v: widen(to_bits(np.array([v], np.float32), dtype), dtype)[0] == v
    for k in range(256):
        if holds(k + 0.5):
            x32[0, 0, k] = k + 0.5
            hand[(0, k)] = min(255, k + (k & 1))
    assert hand[(0, 0)] == 0 and hand[(0, 1)] == 2 and hand[(0, 2)] == 2
    for j, (v, want) in enumerate([(-0.5, 0), (-0.0, 0), (float("nan"), 0), (-float("nan"), 0), (float("inf"), 255), (float("-inf"), 0), (fin, 255), (-fin, 0), (300.0, 255), (-7.0, 0), (256.0, 255)]):
        x32[0, 1, j] = v
        hand[(1, j)] = want
    x32[0, 2:] = np.random.default_rng(9).random((510, 512), dtype=np.float32) * 300 - 20
    bits = to_bits(x32, dtype)
    top = 8 * bits.itemsize - 1
    quiet = {"float16": 0x7E00, "bfloat16": 0x7FC0, "float32": 0x7FC00000}[dtype]
    bits[0, 1, 1], bits[0, 1, 2], bits[0, 1, 3] = 1 << top, quiet, quiet | 1 << top
    fmt = na.TensorFormat(dtype, "CHW", "GREY", "file", scale=1.0, bias=0.0)
    want = rule_bytes(widen(bits, dtype), 1.0, 0.0)
    got = _grey_bytes_guarded(enc.lib, to_device(bits.reshape(1, 1, 512, 512), dtype), fmt)
    for (r, c), b in hand.items():
        assert want[0, r, c] == b and got[0, r, c] == b, (r, c, float(x32[0, r, c]), int(got[0, r, c]))
    assert np.array_equal(got, want)


SIZES = [(1, 1), (511, 513), (512, 512), (513, 1025)]                      # W, H


def _pictures():
    """each size as a contiguous array and as a crop view at an odd offset in a wider parent -> [(host picture, device tensor)]"""
    import torch
    rng = np.random.default_rng(31)
    out = []
    for w, h in SIZES:
        g = rng.integers(0, 256, (h, w), dtype=np.uint8)
        out.append((g, torch.from_numpy(g).cuda()))
        parent = torch.from_numpy(rng.integers(0, 256, (h + 5, w + 37), dtype=np.uint8)).cuda()
        view = parent[3:3 + h, 7:7 + w]
        out.append((view.cpu().numpy().copy(), view))
    return out


def test_pictures_of_any_size(oracle):
    import torch
    import nhwcodec_amd as na
    pics = _pictures()
    tiles = na.tile_pictures_grey_device([d for _, d in pics])
    torch.cuda.synchronize()
    want = np.concatenate([pad_tiles(g) for g, _ in pics])
    assert tuple(tiles.shape) == want.shape and np.array_equal(tiles.cpu().numpy(), want)
    e = na.Encoder(0, max_batch=4)                                          # 6 tiles in the largest picture: two chunks
    dec = na.Decoder(0, max_batch=4)
    q = 20
    hosts = [g for g, _ in pics[::2]]
    containers = e.encode_pictures_grey(hosts, q)
    for g, c in zip(hosts, containers):
        t = pad_tiles(g)
        assert na.picture_info(c) == (g.shape[1], g.shape[0])
        lens = np.frombuffer(c, np.uint32, len(t), 16)
        at = 16 + 4 * len(t)
        for k in range(len(t)):
            assert c[at:at + lens[k]] == oracle_file(oracle, t[k], q), (g.shape, k)
            at += int(lens[k])
        assert at == len(c)
    for g, d in zip(hosts, dec.decode_pictures_grey(containers)):
        assert d.shape == g.shape
    e.close()
    dec.close()


def test_refusals_launch_nothing(enc, oracle):
    import torch
    import nhwcodec_amd as na
    lib = enc.lib
    g = torch.from_numpy(_three()).cuda()
    before = files_of(*enc.encode_grey_device(g, 20))
    flat = torch.zeros((3 * GREY_BYTES + 64,), dtype=torch.uint8, device="cuda")
    x = torch.zeros((3 * GREY_BYTES + 8,), dtype=torch.float32, device="cuda")
    out = torch.full((3 * (512 << 10),), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    status = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bytes_out = torch.full((3 * GREY_BYTES + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    grey_fmt = na.TensorFormat("float32", "CHW", "GREY", "reversed").c_struct()
    colour_fmt = na.TensorFormat("float32", "CHW", "RGB", "reversed").c_struct()
    P = lambda t: t.data_ptr() if t is not None else None

    def call(src=flat.data_ptr(), n=3, q=20, h=enc.h, o=out, s=sizes, t=status):
        return lib.nhw_enc_batch_device_grey(h, src, n, q, P(o), P(s), P(t), None)

    def tcall(fn, c, src=x.data_ptr(), n=3, q=20):
        return fn(enc.h, src, n, ctypes.byref(c), q, P(out), P(sizes), P(status), None)

    assert call(src=None) == NHW_E_ARG and call(h=None) == NHW_E_ARG and call(o=None) == NHW_E_ARG and call(s=None) == NHW_E_ARG and call(t=None) == NHW_E_ARG
    for shift in (1, 2, 4, 8):
        assert call(src=flat.data_ptr() + shift) == NHW_E_ARG, shift
        assert tcall(lib.nhw_enc_batch_device_grey_tensor, grey_fmt, src=x.data_ptr() + shift) == NHW_E_ARG, shift
        assert lib.nhw_tensor_to_bytes_grey_device(x.data_ptr(), 3, ctypes.byref(grey_fmt), bytes_out.data_ptr() + shift, None) == NHW_E_ARG, shift
    for n in (0, -1, 5):
        assert call(n=n) == NHW_E_ARG and tcall(lib.nhw_enc_batch_device_grey_tensor, grey_fmt, n=n) == NHW_E_ARG, n
    assert call(q=0) == NHW_E_QUALITY and call(q=24) == NHW_E_QUALITY
    assert tcall(lib.nhw_enc_batch_device_grey_tensor, colour_fmt) == NHW_E_ARG          # a colour format to a grey call
    assert lib.nhw_tensor_to_bytes_grey_device(x.data_ptr(), 3, ctypes.byref(colour_fmt), bytes_out.data_ptr(), None) == NHW_E_ARG
    assert tcall(lib.nhw_enc_batch_device_tensor, grey_fmt) == NHW_E_ARG                 # a grey format to a colour call
    assert lib.nhw_tensor_to_bytes_device(x.data_ptr(), 1, ctypes.byref(grey_fmt), bytes_out.data_ptr(), None) == NHW_E_ARG
    assert lib.nhw_tile_pictures_grey_device(None, 1, 0, 1, bytes_out.data_ptr(), None) == NHW_E_ARG
    table, tiles, _ = na._picture_table([g[0]], "test", channels=1)
    assert lib.nhw_tile_pictures_grey_device(table.data_ptr(), 1, 0, 1, bytes_out.data_ptr() + 4, None) == NHW_E_ARG
    assert lib.nhw_tile_pictures_grey_device(table.data_ptr(), 0, 0, 1, bytes_out.data_ptr(), None) == NHW_E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((sizes == 0x5A5A5A5A).all()) and bool((status == 0x5A5A5A5A).all()) and bool((bytes_out == SENTINEL).all())
    assert files_of(*enc.encode_grey_device(g, 20)) == before
    assert before[0] == [oracle_file(oracle, _three()[i], 20) for i in range(3)]
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).all())                                             # the same call with nothing wrong does run


@pytest.mark.parametrize("q", [20, 10])
def test_cli_grey(oracle, tmp_path, q):
    """a PGM's rows are top-down: PGM row r is byte-path row 511 - r"""
    exe = built_cli("nhw-enc")
    g = synth_grey(SEEDS[2])
    src, out = tmp_path / "in.pgm", tmp_path / "out.nhw"
    src.write_bytes(b"P5\n# a comment\n512 512\n255\n" + g[::-1].tobytes())
    rc, so, se = run(exe, f"-q{q}", "--grey", str(src), str(out))
    assert rc == 0, (so, se)
    assert out.read_bytes() == oracle_file(oracle, g, q)
