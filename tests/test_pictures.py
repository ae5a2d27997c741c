"""Pictures of any size as padded 512 x 512 tiles in one .nhwp container: the padding rule, the container, the device
kernels k_tile_pad / k_untile_crop (nhw_tile_pictures_device / nhw_untile_pictures_device), the host conveniences nhw_enc_pictures /
nhw_dec_pictures, their Python wrappers and nhw-enc / nhw-dec --picture.  Every tile file must be byte-identical to the oracle's encode of
the padded tile."""
import ctypes
import os
import struct

import numpy as np
import pytest

from tests.picture_cases import SPECS, make_container, pad_reference, parse_container, picture_views
from tests.support import DEC_CLI, ROOT, built_cli, load_lib, run

NEW_SYMBOLS = ("nhw_picture_tiles", "nhw_tile_pictures_device", "nhw_untile_pictures_device", "nhw_picture_info", "nhw_enc_pictures",
               "nhw_dec_pictures")


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def cli():
    built_cli("nhw-dec")
    return built_cli("nhw-enc")


# ---------------------------------------------------------------- without a GPU
def test_picture_symbols_are_exported(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    assert "uint64_t addr, pitch; uint32_t width, height, first_tile, reserved; } nhw_picture;" in hdr


@pytest.mark.parametrize("w,h,tiles", [(1, 1, 1), (512, 512, 1), (513, 512, 2), (512, 513, 2), (1920, 1080, 12), (500, 375, 1),
                                       (65535, 65535, 16384), (0, 5, -4), (5, 0, -4), (65536, 1, -4), (1, 65536, -4)])
def test_picture_tiles_counts(lib, w, h, tiles):
    lib.nhw_picture_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    assert lib.nhw_picture_tiles(w, h) == tiles


def _info(lib, c):
    lib.nhw_picture_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    w, h = ctypes.c_uint32(7), ctypes.c_uint32(7)
    rc = lib.nhw_picture_info(c, len(c), ctypes.byref(w), ctypes.byref(h))
    return rc, w.value, h.value


GOOD = make_container(700, 300, [b"\x02abc", b"\x03de"])
MALFORMED = {
    "empty": b"",
    "short header": GOOD[:15],
    "bad magic": b"NHWQ" + GOOD[4:],
    "version 2": make_container(700, 300, [b"\x02abc", b"\x03de"], version=2),
    "version 0": make_container(700, 300, [b"\x02abc", b"\x03de"], version=0),
    "reserved byte 5": make_container(700, 300, [b"\x02abc", b"\x03de"], reserved=b"\1\0\0"),
    "reserved byte 7": make_container(700, 300, [b"\x02abc", b"\x03de"], reserved=b"\0\0\1"),
    "width 0": make_container(0, 300, [b"\x02abc", b"\x03de"]),
    "height 0": make_container(700, 0, [b"\x02abc", b"\x03de"]),
    "width 65536": make_container(65536, 1, [b"\x02abc"] * 129),
    "height 65536": make_container(1, 65536, [b"\x02abc"] * 129),
    "length 0": make_container(700, 300, [b"", b"\x03de"]),
    "length over the limit": make_container(700, 300, [b"\x02abc", b"\x03de"], lens=[4, (512 << 10) + 1]),
    "truncated": GOOD[:-1],
    "over-long": GOOD + b"\0",
    "directory cut short": GOOD[:19],
    "one tile too few": make_container(700, 300, [b"\x02abc"]),
}


def test_picture_info_accepts_a_hand_built_container(lib):
    import nhwcodec_amd as na
    assert _info(lib, GOOD) == (0, 700, 300)
    assert na.picture_info(GOOD) == (700, 300)
    assert parse_container(GOOD) == (700, 300, [b"\x02abc", b"\x03de"])
    assert _info(lib, make_container(1, 1, [b"\x06" * (512 << 10)]))[0] == 0          # a tile of exactly NHW_OUT_STRIDE bytes
    assert _info(lib, make_container(65535, 1, [b"\x01"] * 128)) == (0, 65535, 1)


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_picture_info_refuses_malformed_containers(lib, case):
    import nhwcodec_amd as na
    assert _info(lib, MALFORMED[case])[0] == na.NHW_E_FORMAT
    with pytest.raises(na.NhwError):
        na.picture_info(MALFORMED[case])


def test_padding_reference_equals_tile_images_for_multiples_of_512():
    import nhwcodec_amd as na
    rng = np.random.default_rng(11)
    for shape in [(512, 512, 3), (1024, 1536, 3), (1536, 512, 3)]:
        big = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(pad_reference(big), na.tile_images(big)[0])
    pic = rng.integers(0, 256, (3, 700, 3), dtype=np.uint8)          # and the rule itself on an odd size
    t = pad_reference(pic)
    assert t.shape == (2, 512, 512, 3)
    assert np.array_equal(t[0][:3], pic[:, :512]) and np.array_equal(t[1][:3, :188], pic[:, 512:])
    assert (t[1][:3, 188:] == pic[:, -1:]).all() and (t[0][3:] == t[0][2]).all()


@pytest.mark.parametrize("args", [["--max-bytes", "5000"], ["--min-psnr", "30"], ["--min-quality", "3"], ["--synthetic", "4", "--outdir", "d"],
                                  ["--tar"], ["--tiles"], ["--batch", "somedir"]])
def test_cli_picture_refuses_other_modes_before_any_gpu_work(cli, tmp_path, args):
    """(a.bmp does not exist: a run that got as far as reading it would say "Could not open file" and exit 255)"""
    rc, out, err = run(cli, "--picture", *args, str(tmp_path / "a.bmp"), str(tmp_path / "b.nhwp"))
    assert rc == 1 and "--picture works alone" in err and "Could not open" not in out
    assert "--picture" in run(cli, "-h")[1] and "--picture" in run(DEC_CLI)[1]


def test_cli_dec_picture_refuses_a_file_that_is_no_container(cli, tmp_path):
    (tmp_path / "x.nhwp").write_bytes(MALFORMED["over-long"])
    rc, out, _ = run(DEC_CLI, "--picture", str(tmp_path / "x.nhwp"), str(tmp_path / "x.bmp"))
    assert rc == 3 and "Not an .nhwp file" in out and not (tmp_path / "x.bmp").exists()


# ---------------------------------------------------------------- on the MI355X
@pytest.mark.gpu
def test_tile_pad_matches_the_padding_rule():
    import nhwcodec_amd as na
    import torch
    assert sorted({(3 * w) % 16 for w, *_ in SPECS}) == list(range(16))
    buf, views = picture_views(SPECS)
    want = np.concatenate([pad_reference(v.cpu().numpy()) for v in views])
    got = na.tile_pictures_device(views)                            # every picture of mixed sizes in one call
    torch.cuda.synchronize()
    assert got.shape == want.shape
    for t in range(want.shape[0]):
        assert np.array_equal(got[t].cpu().numpy(), want[t]), t
    for v in views[:8]:                                              # one picture a call, each path on its own
        assert np.array_equal(na.tile_pictures_device([v]).cpu().numpy(), pad_reference(v.cpu().numpy()))
    # a tile range that starts and ends inside a picture: global tiles [2, T - 3) of (1023 x 1025, 1920 x 1080, 700 x 1)
    pics = [views[6], views[7], views[2]]
    table, tiles, dev = na._picture_table(pics, "test")
    ref = np.concatenate([pad_reference(v.cpu().numpy()) for v in pics])
    out = torch.full((tiles - 5, 512, 512, 3), 7, dtype=torch.uint8, device=dev)
    lib = na._library()
    assert lib.nhw_tile_pictures_device(table.data_ptr(), 3, 2, tiles - 5, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[2:tiles - 3])
    # what the host can check is refused
    assert lib.nhw_tile_pictures_device(table.data_ptr(), 0, 0, 1, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_tile_pictures_device(table.data_ptr(), 3, -1, 1, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_tile_pictures_device(table.data_ptr(), 3, 0, 0, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_tile_pictures_device(None, 3, 0, 1, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_untile_pictures_device(out.data_ptr() + 4, table.data_ptr(), 3, 0, 1, None) == na.NHW_E_ARG


@pytest.mark.gpu
def test_untile_inverts_tile_and_writes_only_the_pictures():
    import nhwcodec_amd as na
    import torch
    src_buf, src = picture_views(SPECS, seed=1)
    tiles = na.tile_pictures_device(src)
    dst_buf, dst = picture_views(SPECS, seed=2)                    # same layout: pitch gaps and slack between pictures
    dst_buf.fill_(0xA5)
    na.untile_pictures_device(tiles, dst)
    torch.cuda.synchronize()
    mask = torch.zeros_like(dst_buf, dtype=torch.bool)
    for v in dst:
        mask.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
    for s, d in zip(src, dst):
        assert torch.equal(s, d)
    assert int(mask.sum()) == sum(3 * w * h for w, h, *_ in SPECS)
    assert bool((dst_buf[~mask] == 0xA5).all()), "a byte outside the pictures was written"


def _test_pictures(oracle):
    """natural pictures (crops of the generator's images): 700 x 300 (2 tiles), 513 x 600 (4), 1024 x 512 (2), 1 x 1 (1)"""
    import nhwcodec_amd as na
    big = na.untile_images(np.stack([oracle.synth(900 + t) for t in range(4)]), 2, 2)
    return [big[5:305, 11:711].copy(), big[100:700, 300:813].copy(), big[512:, :].copy(), big[40:41, 40:41].copy()]


@pytest.mark.gpu
@pytest.mark.parametrize("q", [20, 10])
def test_encode_pictures_tiles_equal_the_oracle(oracle, q):
    import nhwcodec_amd as na
    pics = _test_pictures(oracle)
    e = na.Encoder(0, max_batch=4)                                   # 9 tiles: three chunks, a picture straddles two of them
    got = e.encode_pictures(pics, q)
    assert len(got) == len(pics)
    for pic, c in zip(pics, got):
        w, h, files = parse_container(c)
        assert (w, h) == (pic.shape[1], pic.shape[0]) and na.picture_info(c) == (w, h)
        for t, (f, tile) in enumerate(zip(files, pad_reference(pic))):
            assert f == oracle.encode(tile, q), (pic.shape, t)
    if q == 20:
        files, shape = e.encode_tiled(pics[2], 20)                    # a multiple of 512: the tiles are encode_tiled's
        assert shape == (1, 2) and parse_container(got[2])[2] == files
    e.close()


@pytest.mark.gpu
def test_decode_pictures_equals_the_oracle_crops(oracle):
    import nhwcodec_amd as na
    import torch
    pics = _test_pictures(oracle)
    e = na.Encoder(0, max_batch=4)
    containers = e.encode_pictures(pics, 20)
    e.close()
    want = []
    for pic, c in zip(pics, containers):
        w, h, files = parse_container(c)
        nx = -(-w // 512)
        dec = [oracle.decode(f)[0] for f in files]
        full = np.concatenate([np.concatenate(dec[r * nx:(r + 1) * nx], axis=1) for r in range(len(dec) // nx)], axis=0)
        want.append(full[:h, :w])
    d = na.Decoder(0, max_batch=4)
    got = d.decode_pictures(containers)
    for g, wnt in zip(got, want):
        assert g.shape == wnt.shape and np.array_equal(g, wnt)
    # the device composition: decode_device on the tile files, then untile_pictures_device into crop views of one tensor
    files = [f for c in containers for f in parse_container(c)[2]]
    arena = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]), dtype=torch.int64).cuda()
    lens = torch.tensor([len(f) for f in files], dtype=torch.int32).cuda()
    d9 = na.Decoder(0, max_batch=len(files))
    px, status, _ = d9.decode_device(arena, offs, lens)
    assert int(status.abs().sum()) == 0
    canvas = torch.full((700, 2300, 3), 0x5A, dtype=torch.uint8, device="cuda")
    outs, x = [], 0
    for wnt in want:
        h, w = wnt.shape[:2]
        outs.append(canvas[:h, x:x + w])
        x += w + 3
    na.untile_pictures_device(px, outs)
    torch.cuda.synchronize()
    for o, wnt in zip(outs, want):
        assert np.array_equal(o.cpu().numpy(), wnt)
    d.close(); d9.close()
    # a malformed container and a refused tile: NHW_E_FORMAT, that picture's bytes untouched
    bad_tile = make_container(1, 1, [b"\x07" + containers[3][21:]])          # res_high 7: the decoder refuses the tile
    blob = np.frombuffer(containers[3] + bad_tile + MALFORMED["over-long"], np.uint8)
    off = np.array([0, len(containers[3]), len(containers[3]) + len(bad_tile), blob.size], np.uint64)
    out = np.full(9, 0xEE, np.uint8)
    out_off = np.array([0, 3, 6], np.uint64)
    status = np.zeros(3, np.int32)
    d1 = na.Decoder(0, max_batch=4)
    assert d1.lib.nhw_dec_pictures(d1.h, blob.ctypes.data, off.ctypes.data, 3, out.ctypes.data, out_off.ctypes.data, status.ctypes.data) == 0
    assert status.tolist() == [0, na.NHW_E_FORMAT, na.NHW_E_FORMAT]
    assert np.array_equal(out[:3], want[3].reshape(-1)) and (out[3:] == 0xEE).all()
    d1.close()


def _bmp(pic, top_down=False):
    """a 24-bit BMP of pic (rows in file order), rows padded to 4 bytes; top_down stores them the other way round under a negative height"""
    h, w = pic.shape[:2]
    stride = (3 * w + 3) & ~3
    rows = pic[::-1] if top_down else pic
    body = b"".join(r.tobytes() + b"\0" * (stride - 3 * w) for r in rows)
    return struct.pack("<2sIHHIIiiHHIIiiII", b"BM", 54 + len(body), 0, 0, 54, 40, w, -h if top_down else h, 1, 24, 0, len(body), 0, 0, 0, 0) + body


@pytest.mark.gpu
def test_cli_picture_round_trip(cli, oracle, tmp_path):
    """nhw-enc --picture on odd-width BMPs, bottom-up and top-down: the container's tiles are the oracle's files of the padded tiles;
    nhw-dec --picture writes the crop of the oracle's decodes under a 54-byte header of the picture's size, rows padded to 4 bytes"""
    big = np.stack([oracle.synth(950 + t) for t in range(2)])
    pic = np.ascontiguousarray(np.concatenate([big[0], big[1]], axis=1)[:301, 3:520])          # 517 x 301: 2 tiles, 3W = 1551
    files = [oracle.encode(t, 20) for t in pad_reference(pic)]
    want = np.concatenate([oracle.decode(f)[0] for f in files], axis=1)[:301, :517]
    for top_down in (False, True):
        (tmp_path / "p.bmp").write_bytes(_bmp(pic, top_down))
        rc, out, err = run(cli, "-q20", "--picture", str(tmp_path / "p.bmp"), str(tmp_path / "p.nhwp"))
        assert rc == 0 and "517 x 301" in out, err
        c = (tmp_path / "p.nhwp").read_bytes()
        assert parse_container(c) == (517, 301, files)
        rc, out, err = run(DEC_CLI, "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "o.bmp"))
        assert rc == 0, err
        b = (tmp_path / "o.bmp").read_bytes()
        stride = (3 * 517 + 3) & ~3
        assert len(b) == 54 + stride * 301
        hdr = bytearray(b[:54])
        assert struct.unpack_from("<IiiI", hdr, 18)[:2] == (517, 301) and struct.unpack_from("<I", hdr, 2)[0] == len(b)
        assert struct.unpack_from("<I", hdr, 34)[0] == stride * 301
        ref = bytearray(na_header())
        for o in (2, 18, 22, 34):
            hdr[o:o + 4] = ref[o:o + 4]
        assert hdr == ref                                           # the reference's header but for the size fields
        rows = np.frombuffer(b[54:], np.uint8).reshape(301, stride)
        assert (rows[:, 3 * 517:] == 0).all() and np.array_equal(rows[:, :3 * 517].reshape(301, 517, 3), want)


def na_header():
    import nhwcodec_amd as na
    d = na.Decoder(0, max_batch=1)
    h = d.bmp_header()
    d.close()
    return h
