"""A rectangle of a .nhwp picture from only the tiles it touches: the rule, the kernel k_untile_region
(nhw_untile_regions_device), the host calls nhw_dec_regions / nhw_dec_regions_to_device / nhw_dec_last_region_stats, their Python
wrappers and nhw-dec --picture --region.  A region must equal, byte for byte, the slice of what decode_pictures returns, be made from its
own tiles only and write its own bytes only."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from tests.picture_cases import (SPECS, Rect, Region, World, check_host_result, dest_views, expected_stats, fixed_rects, make_container,
                                 parse_container, picture_views, random_rects, selected, views_mask)
from tests.support import CANARY, ROOT, built_cli, load_lib, run

NEW_SYMBOLS = ("nhw_region_tiles", "nhw_untile_regions_device", "nhw_dec_regions", "nhw_dec_regions_to_device", "nhw_dec_last_region_stats")
PROTOTYPES = """
typedef struct { uint64_t addr, pitch; uint32_t x, y, width, height, pic_width, pic_height, first_tile, reserved; } nhw_region;
int nhw_region_tiles(uint32_t pic_width, uint32_t pic_height, uint32_t x, uint32_t y, uint32_t width, uint32_t height); /* count, or NHW_E_ARG */
int nhw_untile_regions_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, int tile0, int m, void *stream);
typedef struct { uint32_t container, x, y, width, height; } nhw_rect;
int nhw_dec_regions(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                    uint8_t *bgr, const uint64_t *out_off, int32_t *status);
int nhw_dec_regions_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects,
                              const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status);
int nhw_dec_last_region_stats(nhw_dec *d, uint64_t *tiles_decoded, uint64_t *bytes_uploaded);
"""
NHW_E_ARG, NHW_E_FORMAT = -4, -6


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def cli():
    return built_cli("nhw-dec")


# ---------------------------------------------------------------- without a GPU
def test_region_symbols_and_prototypes(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    hdr = squeeze(open(os.path.join(ROOT, "include", "nhw_hip.h")).read())
    decls = re.split(r"\n(?=typedef|int )", PROTOTYPES.strip())
    assert len(decls) == 7
    for decl in decls:
        assert squeeze(decl) in hdr, decl
    assert ctypes.sizeof(Region) == 48 and ctypes.sizeof(Rect) == 20
    import nhwcodec_amd as na
    assert np.dtype(na.REGION_DTYPE).itemsize == 48 and np.dtype(na.RECT_DTYPE).itemsize == 20


@pytest.mark.parametrize("args,want", [
    ((1920, 1080, 10, 20, 300, 200), 1),                  # inside one tile
    ((1920, 1080, 512, 512, 512, 512), 1),                # exactly one tile
    ((1920, 1080, 511, 0, 2, 1), 2),                      # x = 511, w = 2
    ((1920, 1080, 0, 511, 1, 2), 2),
    ((1920, 1080, 511, 511, 2, 2), 4),                    # around a tile corner
    ((1920, 1080, 1000, 500, 100, 100), 4),
    ((1920, 1080, 0, 0, 1920, 1080), 12),                 # = nhw_picture_tiles
    ((1920, 1080, 0, 700, 1920, 1), 4),                   # one full-width row
    ((1920, 1080, 700, 0, 1, 1080), 3),                   # one full-height column
    ((65535, 65535, 0, 0, 65535, 65535), 16384),
    ((65535, 65535, 65534, 65534, 1, 1), 1),
    ((1, 1, 0, 0, 1, 1), 1),
    ((1920, 1080, 0, 0, 0, 5), NHW_E_ARG),                # w = 0
    ((1920, 1080, 0, 0, 5, 0), NHW_E_ARG),                # h = 0
    ((1920, 1080, 1900, 0, 21, 5), NHW_E_ARG),            # x + w = W + 1
    ((1920, 1080, 0, 1000, 5, 81), NHW_E_ARG),            # y + h = H + 1
    ((1920, 1080, 0xFFFFFFFF, 0, 2, 1), NHW_E_ARG),       # x + w overflows 32 bits
    ((1920, 1080, 0, 0xFFFFFFF0, 1, 0x20), NHW_E_ARG),
    ((0, 1080, 0, 0, 1, 1), NHW_E_ARG),                   # W = 0
    ((1920, 0, 0, 0, 1, 1), NHW_E_ARG),
    ((65536, 10, 0, 0, 1, 1), NHW_E_ARG),
])
def test_region_tiles_counts(lib, args, want):
    import nhwcodec_amd as na
    lib.nhw_region_tiles.argtypes = [ctypes.c_uint32] * 6
    assert lib.nhw_region_tiles(*args) == want
    if want > 0:
        assert na.region_tiles(*args) == want == len(selected(args[0], 1, *args[2:]))
        if args[2:] == (0, 0) + args[:2]:
            assert want == na.picture_tiles(*args[:2])
    else:
        with pytest.raises(na.NhwError):
            na.region_tiles(*args)


@pytest.mark.parametrize("tail", [["--region"], ["--region", "x,1,2,3"], ["--region", "1,2,3"], ["--region", "-1,2,3,4"],
                                  ["--region", "1,2,3,4,5"], ["--region", "1,2,3,4 "], ["--region", "1,,3,4"], ["--region", "1,2,3,4", "more"]])
def test_cli_region_refuses_a_malformed_argument(cli, tmp_path, tail):
    """(a does not exist: a run that got as far as reading it would say "Could not open file")"""
    rc, out, err = run(cli, "--picture", str(tmp_path / "a"), str(tmp_path / "b"), *tail)
    assert rc == 1 and "--region" in err and len(err.strip().splitlines()) == 1 and "Could not open" not in out
    assert not (tmp_path / "b").exists()


def test_cli_region_needs_picture(cli, tmp_path):
    for args in (["a.nhw", "b.bmp", "--region", "0,0,1,1"], ["--region", "0,0,1,1", "a.nhw", "b.bmp"], ["--batch", "dir", "--region", "0,0,1,1"],
                 ["--region", "0,0,1,1"]):
        rc, out, err = run(cli, *[str(tmp_path / a) if not a.startswith("-") and "," not in a else a for a in args])
        assert rc == 1 and "--picture" in err and "Could not open" not in out, args
    assert "--region" in run(cli)[1]                                # the usage text names it


def test_cli_region_outside_the_picture_is_refused_before_any_gpu_work(cli, tmp_path):
    """a well-formed container of two files that are no .nhw files: a run that reached the decoder would not exit 1"""
    (tmp_path / "p.nhwp").write_bytes(make_container(700, 300, [b"\x02abc", b"\x03de"]))
    for reg in ("0,0,701,1", "700,0,1,1", "0,300,1,1", "0,299,1,2", "0,0,0,1", "0,0,1,0", "4294967295,0,2,1"):
        rc, out, err = run(cli, "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "o.bmp"), "--region", reg)
        assert rc == 1 and "--region" in err and len(err.strip().splitlines()) == 1, reg
        assert not (tmp_path / "o.bmp").exists()


# ---------------------------------------------------------------- on the MI355X
SIZES = [(1, 700), (500, 375), (1023, 1025), (1920, 1080), (2600, 1600)]          # W, H
QUALITIES = (10, 20)                                                                # one <= 16, one >= 17


@pytest.fixture(scope="module")
def world():
    """the pictures (crops of one seeded 3072 x 2048 scene of generated images), their containers at both qualities -- container
    q * 5 + p is picture p at QUALITIES[q] -- and what decode_pictures makes of them"""
    import nhwcodec_amd as na
    w = World()
    e = na.Encoder(0, max_batch=24)
    scene = na.untile_images(e.synth_device(24, 1300).cpu().numpy(), 4, 6)
    w.pics = [np.ascontiguousarray(scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES]
    w.containers = [c for q in QUALITIES for c in e.encode_pictures(w.pics, q)]
    e.close()
    w.dec = na.Decoder(0, max_batch=8)
    w.full = w.dec.decode_pictures(w.containers)
    for c, f in zip(w.containers, w.full):
        assert na.picture_info(c) == (f.shape[1], f.shape[0])
    yield w
    w.dec.close()


@pytest.mark.gpu
def test_regions_equal_the_slices_of_decode_pictures(world, oracle):
    import nhwcodec_amd as na
    rng = np.random.default_rng(77)
    rects = []
    for ci, f in enumerate(world.full):
        H, W = f.shape[:2]
        mine = fixed_rects(W, H, 512, residues=False) + random_rects(W, H, 200, rng, 700, 40)
        if W >= 64:                                                  # both phases take every residue, picture by picture
            assert sorted({3 * x % 16 for x, _, w, _ in mine}) == list(range(16)) == sorted({3 * w % 16 for x, _, w, _ in mine}), (W, H)
        rects += [(ci, *r) for r in mine]
    assert len(rects) > 2000
    got = world.dec.decode_regions(world.containers, rects)        # one call; max_batch 8: thousands of tiles in chunks of 8
    want_tiles, want_bytes = expected_stats(world.containers, rects, 1, unique=False)
    assert sum(na.region_tiles(world.full[ci].shape[1], world.full[ci].shape[0], x, y, w, h) for ci, x, y, w, h in rects) == want_tiles
    assert world.dec.region_stats() == (want_tiles, want_bytes)
    for (ci, x, y, w, h), g in zip(rects, got):
        assert g.shape == (h, w, 3) and g.dtype == np.uint8
        assert np.array_equal(g, world.full[ci][y:y + h, x:x + w]), (ci, x, y, w, h)
    # two pictures against the plain-C decode of their padded tiles: 500 x 375 at the low quality, 1023 x 1025 at the high one
    for ci in (1, 5 + 2):
        W, H, files = parse_container(world.containers[ci])
        nx = -(-W // 512)
        dec = [oracle.decode(f)[0] for f in files]
        whole = np.concatenate([np.concatenate(dec[r * nx:(r + 1) * nx], axis=1) for r in range(len(dec) // nx)], axis=0)[:H, :W]
        n = 0
        for (c, x, y, w, h), g in zip(rects, got):
            if c == ci:
                assert np.array_equal(g, whole[y:y + h, x:x + w]), (ci, x, y, w, h)
                n += 1
        assert n > 200


def _own_bytes_rects(W, H, rng):
    rects = fixed_rects(W, H, 512, residues=False) + random_rects(W, H, 40, rng, 700, 40)
    return [r for r in rects if r[2] * r[3] < 600000]


@pytest.mark.gpu
def test_untile_regions_device_writes_only_the_regions(world):
    """the kernel on its own: the decoded tiles of one picture, the regions' selected tiles gathered in running order, destinations at
    every misalignment, the launch split into two tile ranges"""
    import nhwcodec_amd as na
    import torch
    ci = 5 + 2                                                       # 1023 x 1025 at the high quality: 6 tiles
    W, H, files = parse_container(world.containers[ci])
    arena = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).cuda()
    lens = [len(f) for f in files]
    d9 = na.Decoder(0, max_batch=len(files))
    px, status, _ = d9.decode_device(arena, torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]), dtype=torch.int64).cuda(),
                                     torch.tensor(lens, dtype=torch.int32).cuda())
    assert int(status.abs().sum()) == 0
    rects = _own_bytes_rects(W, H, np.random.default_rng(5))
    buf, views = dest_views([(w, h) for _, _, w, h in rects])
    table = (Region * len(rects))()
    order = []
    for i, ((x, y, w, h), v) in enumerate(zip(rects, views)):
        table[i] = Region(v.data_ptr(), v.stride(0) if h > 1 else 3 * w, x, y, w, h, W, H, len(order), 0)
        order += selected(W, 1, x, y, w, h, coords=False)
    assert {v.data_ptr() % 16 for v in views} == set(range(16))
    tiles = px[torch.tensor(order, device="cuda")].contiguous()
    d_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    lib = na._library()
    T, cut = len(order), len(order) // 3
    for t0, m in ((cut, T - cut), (0, cut)):                         # two launches, each its own range of the running selection
        assert lib.nhw_untile_regions_device(tiles.data_ptr() + t0 * na.IMG_BYTES, d_table.data_ptr(), len(rects), t0, m, None) == 0
    torch.cuda.synchronize()
    full = torch.from_numpy(world.full[ci]).cuda()
    for (x, y, w, h), v in zip(rects, views):
        assert torch.equal(v, full[y:y + h, x:x + w]), (x, y, w, h)
    mask = views_mask(buf, views)
    assert int(mask.sum()) == sum(3 * w * h for _, _, w, h in rects)
    assert bool((buf[~mask] == CANARY).all()), "a byte outside the regions was written"
    # what the host can check is refused
    assert lib.nhw_untile_regions_device(tiles.data_ptr(), d_table.data_ptr(), 0, 0, 1, None) == na.NHW_E_ARG
    assert lib.nhw_untile_regions_device(tiles.data_ptr(), d_table.data_ptr(), 1, -1, 1, None) == na.NHW_E_ARG
    assert lib.nhw_untile_regions_device(tiles.data_ptr(), d_table.data_ptr(), 1, 0, 0, None) == na.NHW_E_ARG
    assert lib.nhw_untile_regions_device(tiles.data_ptr(), None, 1, 0, 1, None) == na.NHW_E_ARG
    assert lib.nhw_untile_regions_device(tiles.data_ptr() + 4, d_table.data_ptr(), 1, 0, 1, None) == na.NHW_E_ARG
    d9.close()


@pytest.mark.gpu
def test_decode_regions_device_writes_only_the_regions(world):
    import nhwcodec_amd as na
    import torch
    rng = np.random.default_rng(6)
    rects = []
    for ci in (0, 1, 5 + 2, 5 + 3, 4):
        H, W = world.full[ci].shape[:2]
        rects += [(ci, *r) for r in _own_bytes_rects(W, H, rng)]
    buf, views = dest_views([(w, h) for _, _, _, w, h in rects])
    got = world.dec.decode_regions_device(world.containers, rects, out=views)
    assert world.dec.region_stats() == expected_stats(world.containers, rects, 1, unique=False)
    for (ci, x, y, w, h), v, g in zip(rects, views, got):
        assert g is v and np.array_equal(v.cpu().numpy(), world.full[ci][y:y + h, x:x + w]), (ci, x, y, w, h)
    mask = views_mask(buf, views)
    assert bool((buf[~mask] == CANARY).all()), "a byte outside the regions was written"
    # without `out`: fresh tensors on the decoder's device; crops straight into the slots of a batch tensor
    crops = [(5 + 3, x, y, 224, 224) for x, y in ((0, 0), (400, 300), (1696, 856), (511, 511))]
    fresh = world.dec.decode_regions_device(world.containers, crops)
    batch = torch.full((4, 224, 224, 3), CANARY, dtype=torch.uint8, device="cuda")
    world.dec.decode_regions_device(world.containers, crops, out=[batch[i] for i in range(4)])
    for i, (ci, x, y, w, h) in enumerate(crops):
        assert fresh[i].is_cuda and fresh[i].dtype == torch.uint8 and tuple(fresh[i].shape) == (224, 224, 3)
        assert np.array_equal(fresh[i].cpu().numpy(), world.full[ci][y:y + h, x:x + w]) and torch.equal(fresh[i], batch[i])
    assert world.dec.region_stats() == expected_stats(world.containers, crops, 1, unique=False) and world.dec.region_stats()[0] == 1 + 4 + 2 + 4
    # destinations the wrapper refuses
    with pytest.raises(na.NhwError):
        world.dec.decode_regions_device(world.containers, crops, out=[batch[i] for i in range(3)])
    with pytest.raises(na.NhwError):
        world.dec.decode_regions_device(world.containers, crops[:1], out=[batch[0][:, :, :2]])
    with pytest.raises(na.NhwError):
        world.dec.decode_regions_device(world.containers, crops[:1], out=[batch[0].cpu()])
    with pytest.raises(na.NhwError):
        world.dec.decode_regions_device(world.containers, crops[:1], out=[batch[0].transpose(0, 1)])


@pytest.mark.gpu
def test_regions_whose_repeated_tiles_straddle_chunks(world):
    """a 700 x 600 picture (a 2 x 2 grid) on a decoder of max_batch 2: tile (1, 1) alone, all four tiles, tile (1, 1) again -- unmerged
    1 + 4 + 1 = 6 slots, so that chunks of 2 cut the four-tile rect's slots 1 .. 4 across three chunks and tile (1, 1) is decoded in three of
    them; the same rects as windows at scale 1 decode the four tiles once"""
    import nhwcodec_amd as na
    import torch
    e = na.Encoder(0, max_batch=4)
    container = e.encode_pictures([np.ascontiguousarray(world.pics[3][:600, :700])], 20)[0]
    e.close()
    W, H, files = parse_container(container)
    assert (W, H, len(files)) == (700, 600, 4)
    rects = [(0, 520, 515, 50, 40), (0, 100, 100, 500, 450), (0, 520, 515, 50, 40)]
    assert [selected(W, 1, *r[1:], coords=False) for r in rects] == [[3], [0, 1, 2, 3], [3]]
    unmerged = (6, 2 * len(files[3]) + sum(len(f) for f in files))
    assert expected_stats([container], rects, 1, unique=False) == unmerged
    dec = na.Decoder(0, max_batch=2)
    full = dec.decode_pictures([container])[0]
    assert full.shape == (600, 700, 3)
    want = [full[y:y + h, x:x + w] for _, x, y, w, h in rects]

    def check(got):
        assert len(got) == len(want)
        for g, f in zip(got, want):
            assert np.array_equal(g.cpu().numpy() if isinstance(g, torch.Tensor) else g, f)

    check(dec.decode_regions([container], rects))
    assert dec.region_stats() == unmerged
    buf, views = dest_views([(w, h) for _, _, _, w, h in rects])
    check(dec.decode_regions_device([container], rects, out=views))
    assert dec.region_stats() == unmerged
    assert bool((buf[~views_mask(buf, views)] == CANARY).all()), "a byte outside the regions was written"
    merged = (4, sum(len(f) for f in files))
    check(dec.decode_windows([container], rects, 1))
    assert dec.region_stats() == merged
    buf2, views2 = dest_views([(w, h) for _, _, _, w, h in rects])
    check(dec.decode_windows_device([container], rects, 1, out=views2))
    assert dec.region_stats() == merged
    assert torch.equal(buf, buf2)                                    # the same bytes, canaries included
    dec.close()


def _call_regions(dec, containers, rects, canary_host=None, dst=None):
    """nhw_dec_regions (or, with dst = (addresses, pitches), nhw_dec_regions_to_device) by ctypes: the wrappers raise on a status
    -> (rc, status, the host buffer, its offsets)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    if dst is not None:
        addr, pitch = (np.array(a, np.uint64) for a in dst)
        rc = dec.lib.nhw_dec_regions_to_device(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects),
                                               addr.ctypes.data, pitch.ctypes.data, status.ctypes.data)
        return rc, status, None, None
    out_off = np.zeros(len(rects) + 1, np.uint64)
    out_off[1:] = np.cumsum([3 * r[3] * r[4] + 7 for r in rects])     # 7 bytes of slack behind every region
    out = np.full(int(out_off[-1]) + 16, CANARY, np.uint8) if canary_host is None else canary_host
    rc = dec.lib.nhw_dec_regions(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), out.ctypes.data,
                                 out_off.ctypes.data, status.ctypes.data)
    return rc, status, out, out_off


@pytest.mark.gpu
def test_a_refused_tile_fails_exactly_the_regions_that_select_it(world):
    import nhwcodec_amd as na
    import torch
    ci, k = 5 + 2, 3                                                 # 1023 x 1025, 2 x 3 tiles: tile (ty 1, tx 1)
    W, H, files = parse_container(world.containers[ci])
    bad = list(files)
    bad[k] = b"\x07" + files[k][1:]                                  # res_high 7: the decoder refuses the tile
    broken = make_container(W, H, bad)
    assert na.picture_info(broken) == (W, H)                         # the directory is consistent: the container is well-formed
    rng = np.random.default_rng(9)
    rects = [(0, *r) for r in fixed_rects(W, H, 512, residues=False) + random_rects(W, H, 60, rng, 700, 40)]
    hit = [k in selected(W, 1, *r[1:], coords=False) for r in rects]
    assert 10 < sum(hit) < len(rects) - 10
    full = world.full[ci]
    rc, status, out, out_off = _call_regions(world.dec, [broken], rects)
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    check_host_result(rects, status, out, out_off, lambda c: full)
    assert world.dec.region_stats() == expected_stats([broken], rects, 1, unique=False)   # every rect was handed to the decoder
    with pytest.raises(na.NhwError):
        world.dec.decode_regions([broken], rects)
    ok = [r for r, h in zip(rects, hit) if not h]
    for (c, x, y, w, h), g in zip(ok, world.dec.decode_regions([broken], ok)):
        assert np.array_equal(g, full[y:y + h, x:x + w])
    # on the device: a failed rect may have bytes of its own rows written, nothing else is touched
    buf, views = dest_views([(w, h) for _, _, _, w, h in rects])
    dst = ([v.data_ptr() for v in views], [v.stride(0) if v.shape[0] > 1 else 3 * v.shape[1] for v in views])
    rc, status, _, _ = _call_regions(world.dec, [broken], rects, dst=dst)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    for (c, x, y, w, h), v, h_ in zip(rects, views, hit):
        if not h_:
            assert np.array_equal(v.cpu().numpy(), full[y:y + h, x:x + w])
    assert bool((buf[~views_mask(buf, views)] == CANARY).all())


@pytest.mark.gpu
def test_statuses_are_per_rect(world):
    import nhwcodec_amd as na
    import torch
    containers = [world.containers[1], world.containers[5 + 2][:-1], world.containers[3]]   # 500 x 375; truncated; 1920 x 1080
    rects = [(0, 10, 20, 100, 50),
             (3, 0, 0, 1, 1),                                        # container index out of range
             (2, 1900, 0, 21, 5),                                    # x + w > W
             (1, 0, 0, 5, 5),                                        # a malformed container
             (2, 500, 500, 30, 30),
             (0, 0, 0, 0, 5),                                        # w = 0
             (0, 0, 371, 5, 5),                                      # y + h > H
             (1, 600, 600, 10, 10),
             (2, 0, 0, 1920, 1080),
             (0xFFFFFFFF, 0, 0, 1, 1),
             (0, 0, 0, 5, 0)]
    want = [0, NHW_E_ARG, NHW_E_ARG, NHW_E_FORMAT, 0, NHW_E_ARG, NHW_E_ARG, NHW_E_FORMAT, 0, NHW_E_ARG, NHW_E_ARG]
    full = {0: world.full[1], 2: world.full[3]}
    rc, status, out, out_off = _call_regions(world.dec, containers, rects)
    assert rc == 0 and status.tolist() == want
    check_host_result(rects, status, out, out_off, lambda c: full[c])
    good = [r for r, s in zip(rects, want) if s == 0]
    assert world.dec.region_stats() == expected_stats(containers, good, 1, unique=False)      # only the good rects reached the decoder
    with pytest.raises(na.NhwError):
        world.dec.decode_regions(containers, rects)
    # the same on the device: the rects that are not NHW_OK leave their destinations untouched
    buf, views = dest_views([(max(w, 1), max(h, 1)) for _, _, _, w, h in rects])
    dst = ([v.data_ptr() for v in views], [v.stride(0) if v.shape[0] > 1 else 3 * v.shape[1] for v in views])
    rc, status, _, _ = _call_regions(world.dec, containers, rects, dst=dst)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == want
    for (ci, x, y, w, h), v, st in zip(rects, views, want):
        if st == 0:
            assert np.array_equal(v.cpu().numpy(), full[ci][y:y + h, x:x + w])
    assert bool((buf[~views_mask(buf, [v for v, st in zip(views, want) if st == 0])] == CANARY).all())
    # the call as a whole fails only for what no rect can answer for
    before = buf.clone()
    assert _call_regions(world.dec, containers, rects[:1], dst=([views[0].data_ptr()], [3 * 100 - 1]))[0] == na.NHW_E_ARG
    assert _call_regions(world.dec, containers, rects[:1], dst=([0], [3 * 100]))[0] == na.NHW_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    blob = np.frombuffer(containers[0], np.uint8)
    off = np.array([0, blob.size], np.uint64)
    table = (Rect * 1)(Rect(0, 0, 0, 1, 1))
    st, oo, px = np.zeros(1, np.int32), np.zeros(1, np.uint64), np.zeros(3, np.uint8)
    L, h = world.dec.lib, world.dec.h
    a = ctypes.addressof(table)
    assert L.nhw_dec_regions(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == 0 and st[0] == 0
    assert L.nhw_dec_regions(h, blob.ctypes.data, off.ctypes.data, 1, a, 0, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_regions(h, blob.ctypes.data, off.ctypes.data, 0, a, 1, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_regions(h, None, off.ctypes.data, 1, a, 1, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_regions(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, None, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_regions(h, blob.ctypes.data, np.array([5, 0], np.uint64).ctypes.data, 1, a, 1, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_regions_to_device(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, None, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG


@pytest.mark.gpu
def test_whole_picture_regions_write_what_untile_pictures_writes():
    import nhwcodec_amd as na
    import torch
    _, src = picture_views(SPECS, seed=1)
    tiles = na.tile_pictures_device(src)
    old_buf, old = picture_views(SPECS, seed=2)
    new_buf, new = picture_views(SPECS, seed=2)                             # the same layout and the same bytes underneath
    old_buf.fill_(CANARY)
    new_buf.fill_(CANARY)
    na.untile_pictures_device(tiles, old)
    table = (Region * len(SPECS))()
    first = 0
    for i, ((w, h, extra, _), v) in enumerate(zip(SPECS, new)):
        table[i] = Region(v.data_ptr(), 3 * w + extra, 0, 0, w, h, w, h, first, 0)
        first += na.picture_tiles(w, h)
    assert first == tiles.shape[0]
    d_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    assert na._library().nhw_untile_regions_device(tiles.data_ptr(), d_table.data_ptr(), len(SPECS), 0, first, None) == 0
    torch.cuda.synchronize()
    for s, v in zip(src, new):
        assert torch.equal(s, v)
    assert torch.equal(old_buf, new_buf)


@pytest.mark.gpu
def test_one_handle_serves_pictures_regions_and_files_in_turn(world):
    import nhwcodec_amd as na
    d = na.Decoder(0, max_batch=8)
    cs = [world.containers[1], world.containers[5 + 2]]
    full = [world.full[1], world.full[5 + 2]]
    rects = [(1, 500, 500, 100, 100), (0, 0, 0, 500, 375), (1, 0, 0, 1023, 1025), (0, 499, 374, 1, 1)]
    files = parse_container(cs[1])[2][:8]
    first = None
    for _ in range(2):
        pics = d.decode_pictures(cs)
        regs = d.decode_regions(cs, rects)
        px, qs = d.decode(files)
        for p, f in zip(pics, full):
            assert np.array_equal(p, f)
        for (ci, x, y, w, h), g in zip(rects, regs):
            assert np.array_equal(g, full[ci][y:y + h, x:x + w])
        assert qs == [QUALITIES[1]] * len(files)
        assert np.array_equal(px[0][:, :, :], full[1][:512, :512])
        if first is None:
            first = px.copy()
        assert np.array_equal(px, first)
        assert d.region_stats() == expected_stats(cs, rects, 1, unique=False)
    d.close()


@pytest.mark.gpu
def test_cli_region_equals_the_rectangle_of_the_whole_bmp(cli, world, tmp_path):
    """X, Y count from the top left of the picture as a viewer shows the (bottom-up) BMP"""
    ci = 5 + 2
    W, H = 1023, 1025
    (tmp_path / "p.nhwp").write_bytes(world.containers[ci])
    rc, out, err = run(cli, "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "full.bmp"))
    assert rc == 0, err
    whole = (tmp_path / "full.bmp").read_bytes()
    stride = (3 * W + 3) & ~3
    rows = np.frombuffer(whole[54:], np.uint8).reshape(H, stride)
    assert np.array_equal(rows[:, :3 * W].reshape(H, W, 3), world.full[ci])
    for x, y, w, h in ((0, 0, 1023, 3), (500, 1000, 30, 25), (510, 300, 5, 400), (1022, 1024, 1, 1)):   # the top row; the bottom row; ...
        rc, out, err = run(cli, "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "r.bmp"), "--region", f"{x},{y},{w},{h}")
        assert rc == 0 and f"{w} x {h}" in out, err
        b = (tmp_path / "r.bmp").read_bytes()
        rs = (3 * w + 3) & ~3
        assert len(b) == 54 + rs * h
        hdr = bytearray(b[:54])
        assert struct.unpack_from("<ii", hdr, 18) == (w, h) and struct.unpack_from("<I", hdr, 2)[0] == len(b) and struct.unpack_from("<I", hdr, 34)[0] == rs * h
        ref = bytearray(whole[:54])
        for o in (2, 18, 22, 34):
            hdr[o:o + 4] = ref[o:o + 4]
        assert hdr == ref                                           # the whole picture's header but for the size fields
        got = np.frombuffer(b[54:], np.uint8).reshape(h, rs)
        assert (got[:, 3 * w:] == 0).all()
        assert np.array_equal(got[:, :3 * w], rows[H - y - h:H - y, 3 * x:3 * (x + w)]), (x, y, w, h)
