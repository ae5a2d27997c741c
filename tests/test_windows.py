"""Windows: rectangles of .nhwp pictures at scale 1, 2 or 4, every tile of a call decoded once: the rule, the kernel
k_untile_window (nhw_untile_windows_device), the host calls nhw_dec_windows / nhw_dec_windows_to_device, their Python wrappers and
nhw-dec --picture --window.  A window must equal, byte for byte, the slice of what decode_pictures_scaled returns at its scale, be made
from its own tiles only -- each uploaded and decoded once a call -- and write its own bytes only."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from tests.picture_cases import (SIZES, Rect, Region, World, check_host_result, dest_views, expected_stats, fixed_rects, make_container,
                                 parse_container, random_rects, selected, views_mask)
from tests.support import CANARY, ROOT, built_cli, load_lib, run

NEW_SYMBOLS = ("nhw_window_tiles", "nhw_untile_windows_device", "nhw_dec_windows", "nhw_dec_windows_to_device")
PROTOTYPES = """
int nhw_window_tiles(uint32_t pic_width, uint32_t pic_height, int scale, uint32_t x, uint32_t y, uint32_t width, uint32_t height);
typedef struct { uint32_t region, slot, tx, ty; } nhw_window_use;   /* 16 bytes */
int nhw_untile_windows_device(const void *d_tiles, const nhw_region *d_regs, int n_regs, const nhw_window_use *d_uses, int n_uses,
                              int tile0, int m, int scale, void *stream);
int nhw_dec_windows(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                    uint8_t *bgr, const uint64_t *out_off, int32_t *status);
int nhw_dec_windows_to_device(nhw_dec *d, const uint8_t *blob, const uint64_t *off, int n_containers, const nhw_rect *rects, int n_rects, int scale,
                              const uint64_t *dst_addr, const uint64_t *dst_pitch, int32_t *status);
"""
NHW_E_ARG, NHW_E_FORMAT = -4, -6
SCALES = (1, 2, 4)


class Use(ctypes.Structure):                                      # the tests' own mirror of nhw_window_use
    _fields_ = [(n, ctypes.c_uint32) for n in ("region", "slot", "tx", "ty")]


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def cli():
    return built_cli("nhw-dec")


# ---------------------------------------------------------------- without a GPU
def test_window_symbols_and_prototypes(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    hdr = squeeze(open(os.path.join(ROOT, "include", "nhw_hip.h")).read())
    decls = re.split(r"\n(?=typedef|int )", PROTOTYPES.strip())
    assert len(decls) == 5
    for decl in decls:
        assert squeeze(decl) in hdr, decl
    assert ctypes.sizeof(Use) == 16 and ctypes.sizeof(Region) == 48
    import nhwcodec_amd as na
    assert np.dtype(na.WINDOW_USE_DTYPE).itemsize == 16
    assert callable(na.window_tiles) and callable(na.Decoder.decode_windows) and callable(na.Decoder.decode_windows_device)


REGION_ARGS = [(1920, 1080, 10, 20, 300, 200), (1920, 1080, 511, 511, 2, 2), (1920, 1080, 0, 0, 1920, 1080), (65535, 65535, 0, 0, 65535, 65535),
               (1, 1, 0, 0, 1, 1), (1920, 1080, 1900, 0, 21, 5), (1920, 1080, 0xFFFFFFFF, 0, 2, 1), (0, 1080, 0, 0, 1, 1), (65536, 10, 0, 0, 1, 1)]


@pytest.mark.parametrize("args,want", [
    ((1023, 1025, 2, 0, 0, 512, 513), 6),                 # the whole scaled picture
    ((1023, 1025, 4, 0, 0, 256, 257), 6),
    ((1023, 1025, 2, 255, 255, 2, 2), 4),                 # around a T = 256 corner
    ((1023, 1025, 4, 127, 0, 2, 1), 2),                   # x = T - 1, w = 2 at T = 128
    ((1023, 1025, 2, 511, 512, 1, 1), 1),                 # the last scaled column and row: from the padding
    ((1023, 1025, 4, 255, 256, 1, 1), 1),
    ((65535, 65535, 4, 0, 0, 16384, 16384), 16384),
    ((65535, 65535, 2, 32767, 32767, 1, 1), 1),
    ((1023, 1025, 2, 511, 0, 2, 1), NHW_E_ARG),           # x + w = W' + 1
    ((1023, 1025, 4, 0, 256, 1, 2), NHW_E_ARG),           # y + h = H' + 1
    ((1023, 1025, 1, 1022, 0, 2, 1), NHW_E_ARG),
    ((1023, 1025, 3, 0, 0, 1, 1), NHW_E_ARG),             # a scale that does not exist
    ((1023, 1025, 0, 0, 0, 1, 1), NHW_E_ARG),
    ((1023, 1025, 8, 0, 0, 1, 1), NHW_E_ARG),
    ((1023, 1025, -2, 0, 0, 1, 1), NHW_E_ARG),
    ((1023, 1025, 2, 0, 0, 0, 5), NHW_E_ARG),             # w = 0
    ((1023, 1025, 2, 0, 0, 5, 0), NHW_E_ARG),
    ((1023, 1025, 2, 0xFFFFFFFF, 0, 2, 1), NHW_E_ARG),    # x + w overflows 32 bits
    ((0, 1025, 2, 0, 0, 1, 1), NHW_E_ARG),                # W = 0
    ((65536, 10, 2, 0, 0, 1, 1), NHW_E_ARG),              # a side above 65535
    ((10, 65536, 4, 0, 0, 1, 1), NHW_E_ARG),
])
def test_window_tiles_counts(lib, args, want):
    import nhwcodec_amd as na
    lib.nhw_window_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_uint32] * 4
    assert lib.nhw_window_tiles(*args) == want
    if want > 0:
        assert na.window_tiles(*args) == want == len(selected(args[0], *args[2:]))
    else:
        with pytest.raises(na.NhwError):
            na.window_tiles(*args)


@pytest.mark.parametrize("args", REGION_ARGS)
def test_window_tiles_at_scale_1_is_region_tiles(lib, args):
    import nhwcodec_amd as na
    lib.nhw_window_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_uint32] * 4
    lib.nhw_region_tiles.argtypes = [ctypes.c_uint32] * 6
    want = lib.nhw_region_tiles(*args)
    assert lib.nhw_window_tiles(args[0], args[1], 1, *args[2:]) == want
    if want > 0:
        assert na.window_tiles(args[0], args[1], 1, *args[2:]) == want == na.region_tiles(*args)
    else:
        assert want == NHW_E_ARG
        with pytest.raises(na.NhwError):
            na.window_tiles(args[0], args[1], 1, *args[2:])


@pytest.mark.parametrize("tail", [["--window"], ["--window", "1,2,3,4"], ["--window", "1,2,3,4,5,6"], ["--window", "3,0,0,1,1"], ["--window", "0,0,0,1,1"],
                                  ["--window", "2,-1,0,1,1"], ["--window", "+2,1,0,1,1"], ["--window", "2,0,0,1,1 "], ["--window", "2, 0,0,1,1"],
                                  ["--window", "2,,0,1,1"], ["--window", "x,0,0,1,1"], ["--window", "2,0,0,1,1", "more"],
                                  ["--window", "2,0,0,1,1", "--scale", "2"], ["--window", "2,0,0,1,1", "--region", "0,0,1,1"],
                                  ["--region", "0,0,1,1", "--window", "2,0,0,1,1"], ["--window=2,0,0,1,1"]])
def test_cli_window_refuses_a_malformed_argument(cli, tmp_path, tail):
    """(a does not exist: a run that got as far as reading it would say "Could not open file")"""
    rc, out, err = run(cli, "--picture", str(tmp_path / "a"), str(tmp_path / "b"), *tail)
    assert rc == 1 and "--window" in err and len(err.strip().splitlines()) == 1 and "Could not open" not in out
    assert not os.listdir(tmp_path)


def test_cli_window_needs_picture(cli, tmp_path):
    for args in (["a.nhw", "b.bmp", "--window", "1,0,0,1,1"], ["--window", "1,0,0,1,1", "a.nhw", "b.bmp"], ["--batch", "dir", "--window", "1,0,0,1,1"],
                 ["--window", "1,0,0,1,1"], ["--scale", "2", "--picture", "a.nhwp", "b.bmp", "--window", "2,0,0,1,1"]):
        rc, out, err = run(cli, *[str(tmp_path / a) if not a.startswith("-") and "," not in a and len(a) > 1 else a for a in args])
        assert rc == 1 and "--window" in err and len(err.strip().splitlines()) == 1 and "Could not open" not in out, args
    assert not os.listdir(tmp_path)
    assert "--window" in run(cli)[1]                                # the usage text names it


def test_cli_window_outside_the_picture_is_refused_before_any_gpu_work(cli, tmp_path):
    """a well-formed container of two files that are no .nhw files: a run that reached the decoder would not exit 1"""
    (tmp_path / "p.nhwp").write_bytes(make_container(700, 300, [b"\x02abc", b"\x03de"]))
    for win in ("2,350,0,1,1", "2,0,0,351,1", "2,0,150,1,1", "2,0,149,1,2", "4,175,0,1,1", "4,0,0,1,76", "1,0,0,701,1", "1,0,300,1,1", "2,0,0,0,1",
                "2,0,0,1,0", "2,4294967295,0,2,1"):
        rc, out, err = run(cli, "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "o.bmp"), "--window", win)
        assert rc == 1 and "--window" in err and len(err.strip().splitlines()) == 1, win
        assert not (tmp_path / "o.bmp").exists()


# ---------------------------------------------------------------- on the MI355X
QUALITIES = (10, 20)                                                # one <= 16, one >= 17
BIG = 3 + 2                                                         # 1023 x 1025 at the high quality: a 2 x 3 grid, odd sides


@pytest.fixture(scope="module")
def world():
    """the pictures (crops of one seeded 3072 x 2048 scene of generated images), their containers at both qualities -- container
    q * 3 + p is picture p at QUALITIES[q] -- and what decode_pictures_scaled makes of them at every scale.  The decoder takes 4 tiles a
    chunk: the six tiles of the large picture span two chunks."""
    import nhwcodec_amd as na
    w = World()
    e = na.Encoder(0, max_batch=24)
    scene = na.untile_images(e.synth_device(24, 1300).cpu().numpy(), 4, 6)
    w.pics = [np.ascontiguousarray(scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES]
    w.containers = [c for q in QUALITIES for c in e.encode_pictures(w.pics, q)]
    e.close()
    w.dec = na.Decoder(0, max_batch=4)
    w.full = {s: w.dec.decode_pictures_scaled(w.containers, s) for s in SCALES}
    for c, f in zip(w.containers, w.full[1]):
        assert na.picture_info(c) == (f.shape[1], f.shape[0])
    yield w
    w.dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_windows_equal_the_slices_of_decode_pictures_scaled(world, scale):
    import nhwcodec_amd as na
    T = 512 // scale
    rng = np.random.default_rng(770 + scale)
    rects = []
    for ci, f in enumerate(world.full[scale]):
        H, W = f.shape[:2]
        assert (W, H) == na.scaled_size(*SIZES[ci % 3], scale)
        mine = fixed_rects(W, H, T, residues=True) + random_rects(W, H, 100, rng, 400, 24)
        if W >= 32:                                                  # both phases take every residue, picture by picture
            assert sorted({3 * x % 16 for x, _, w, _ in mine}) == list(range(16)) == sorted({3 * w % 16 for x, _, w, _ in mine}), (W, H)
        rects += [(ci, *r) for r in mine]
    assert len(rects) > 600
    got = world.dec.decode_windows(world.containers, rects, scale)   # one call; max_batch 4: the 18 unique tiles go in five chunks
    stats = world.dec.region_stats()
    assert stats == expected_stats(world.containers, rects, scale, unique=True)
    assert stats == (18, sum(len(f) for c in world.containers for f in parse_container(c)[2]))   # every tile of every container, once
    assert sum(na.window_tiles(*SIZES[ci % 3], scale, x, y, w, h) for ci, x, y, w, h in rects) > 20 * stats[0]
    for (ci, x, y, w, h), g in zip(rects, got):
        assert g.shape == (h, w, 3) and g.dtype == np.uint8
        assert np.array_equal(g, world.full[scale][ci][y:y + h, x:x + w]), (scale, ci, x, y, w, h)
    # two pictures assembled by the test from the scaled decode of their tile files: 500 x 375 at the low quality, 1023 x 1025 at the high one
    for ci in (1, BIG):
        W, H, files = parse_container(world.containers[ci])
        nx = -(-W // 512)
        dec = world.dec.decode_scaled(files, scale)[0]
        assert dec.shape == (len(files), T, T, 3)
        whole = np.concatenate([np.concatenate(list(dec[r * nx:(r + 1) * nx]), axis=1) for r in range(len(files) // nx)], axis=0)[:-(-H // scale), :-(-W // scale)]
        assert np.array_equal(whole, world.full[scale][ci])
        n = 0
        for (c, x, y, w, h), g in zip(rects, got):
            if c == ci:
                assert np.array_equal(g, whole[y:y + h, x:x + w]), (scale, ci, x, y, w, h)
                n += 1
        assert n > 100
    # the rects in another order: the same pictures in that order
    perm = rng.permutation(len(rects))
    again = world.dec.decode_windows(world.containers, [rects[i] for i in perm], scale)
    assert world.dec.region_stats() == stats
    for i, g in zip(perm, again):
        assert np.array_equal(g, got[i]), (scale, rects[i])


@pytest.mark.gpu
def test_a_tile_selected_twice_is_decoded_once_by_windows_and_twice_by_regions(world):
    ci = 3 + 1                                                       # 500 x 375 at the high quality: one tile
    size = len(parse_container(world.containers[ci])[2][0])
    rects = [(ci, 10, 20, 200, 100), (ci, 100, 60, 300, 200)]
    full = world.full[1][ci]
    got = world.dec.decode_windows(world.containers, rects)
    assert world.dec.region_stats() == (1, size)
    old = world.dec.decode_regions(world.containers, rects)
    assert world.dec.region_stats() == (2, 2 * size)                 # the old family is unchanged
    for (c, x, y, w, h), g, o in zip(rects, got, old):
        assert np.array_equal(g, full[y:y + h, x:x + w]) and np.array_equal(o, g)
    for scale in (2, 4):
        half = [(ci, x // scale, y // scale, w // scale, h // scale) for _, x, y, w, h in rects]
        for (c, x, y, w, h), g in zip(half, world.dec.decode_windows(world.containers, half, scale)):
            assert np.array_equal(g, world.full[scale][ci][y:y + h, x:x + w])
        assert world.dec.region_stats() == (1, size)


def _pitch(v):
    return v.stride(0) if v.shape[0] > 1 else 3 * v.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_whole_picture_windows_write_what_the_picture_crop_writes(scale):
    """the crop kernels against each other, no decode: random bytes as the tiles of four scaled pictures -- 1 x 1, 5 x 3, a 2 x 1 grid with a
    one-pixel last column, a 3 x 2 grid -- written by nhw_untile_pictures_scaled_device, by nhw_untile_windows_device (window = the whole
    picture, uses in slot order) and, at T = 512, by nhw_untile_regions_device, each into its own canary-filled buffer at the same
    misalignments and pitches: the buffers are equal byte for byte and hold the numpy crop of the tiles"""
    import nhwcodec_amd as na
    import torch
    T = 512 // scale
    sizes = [(1, 1), (5, 3), (T + 1, T // 2 + 1), (2 * T + 1, T + 1)]   # W, H
    grids = [(-(-w // T), -(-h // T)) for w, h in sizes]
    assert grids == [(1, 1), (1, 1), (2, 1), (3, 2)]
    first = np.concatenate([[0], np.cumsum([nx * ny for nx, ny in grids])])
    n_tiles = int(first[-1])
    tiles_h = np.random.default_rng(90 + scale).integers(0, 256, (n_tiles, T, T, 3), dtype=np.uint8)
    tiles = torch.from_numpy(tiles_h).cuda()
    want = [np.concatenate([np.concatenate(list(tiles_h[f + r * nx:f + (r + 1) * nx]), axis=1) for r in range(ny)], axis=0)[:h, :w]
            for (w, h), (nx, ny), f in zip(sizes, grids, first)]
    lib = na._library()
    keep = []                                                        # the tables, until the launches have run

    def filled(launch):
        """launch(views) writes the pictures; -> the whole buffer, checked against the numpy crop"""
        buf, views = dest_views(sizes)
        assert launch(views) == 0
        torch.cuda.synchronize()
        for v, w in zip(views, want):
            assert np.array_equal(v.cpu().numpy(), w)
        assert bool((buf[~views_mask(buf, views)] == CANARY).all()), "a byte outside the pictures was written"
        return buf

    def regions(views, numbered):
        table = (Region * len(sizes))(*[Region(v.data_ptr(), _pitch(v), 0, 0, w, h, w, h, int(f) if numbered else 0xDEAD, 0)
                                        for v, (w, h), f in zip(views, sizes, first)])
        keep.append(torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda())
        return keep[-1]

    def by_pictures(views):
        table = np.zeros(len(sizes), na.PICTURE_DTYPE)
        for k, (v, (w, h)) in enumerate(zip(views, sizes)):
            table[k] = (v.data_ptr(), _pitch(v), w, h, first[k], 0)
        keep.append(torch.from_numpy(table.view(np.uint8).copy()).cuda())
        return lib.nhw_untile_pictures_scaled_device(tiles.data_ptr(), keep[-1].data_ptr(), len(sizes), 0, n_tiles, scale, None)

    def by_windows(views):
        uses = [Use(k, int(first[k]) + ty * nx + tx, tx, ty) for k, (nx, ny) in enumerate(grids) for ty in range(ny) for tx in range(nx)]
        assert [u.slot for u in uses] == list(range(n_tiles))
        d_uses = torch.from_numpy(np.frombuffer(bytes((Use * len(uses))(*uses)), np.uint8).copy()).cuda()
        keep.append(d_uses)
        return lib.nhw_untile_windows_device(tiles.data_ptr(), regions(views, False).data_ptr(), len(sizes), d_uses.data_ptr(), len(uses), 0, n_tiles, scale, None)

    def by_regions(views):
        return lib.nhw_untile_regions_device(tiles.data_ptr(), regions(views, True).data_ptr(), len(sizes), 0, n_tiles, None)

    a, b = filled(by_pictures), filled(by_windows)
    assert torch.equal(a, b)
    if scale == 1:
        assert torch.equal(a, filled(by_regions))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_untile_windows_device_writes_only_the_windows(scale):
    """the kernel on its own, no decode: six tiles of random bytes as the 2 x 3 grid of a picture with odd sides, destinations at every
    misalignment, the launch split into two chunks that both see the whole use table, and uses that must store nothing"""
    import nhwcodec_amd as na
    import torch
    T = 512 // scale
    W, H = -(-1023 // scale), -(-1025 // scale)                      # 1023 x 1025, 512 x 513, 256 x 257
    nx, ny = -(-W // T), -(-H // T)
    assert (nx, ny) == (2, 3)
    rng = np.random.default_rng(60 + scale)
    tiles_h = rng.integers(0, 256, (nx * ny, T, T, 3), dtype=np.uint8)
    whole = np.concatenate([np.concatenate(list(tiles_h[r * nx:(r + 1) * nx]), axis=1) for r in range(ny)], axis=0)[:H, :W]
    tiles = torch.from_numpy(tiles_h).cuda()
    rects = [r for r in fixed_rects(W, H, T, residues=True) + random_rects(W, H, 40, rng, 400, 24)]
    # descriptors that are no windows of a picture, each with a destination of its own that must stay as it is: a zero width, a zero
    # height, a side above the largest scaled side, x + w and y + h beyond the side
    side_max = -(-65535 // scale)
    traps = [(0, 0, 0, 4, W, H), (0, 0, 4, 0, W, H), (0, 0, 4, 4, side_max + 1, H), (0, 0, 4, 4, W, side_max + 1), (W - 1, 0, 2, 1, W, H), (0, H - 1, 1, 2, W, H)]
    buf, views = dest_views([(w, h) for _, _, w, h in rects] + [(8, 8)] * len(traps))
    assert {v.data_ptr() % 16 for v in views} == set(range(16))
    table = (Region * (len(rects) + len(traps) + 1))()
    uses = []
    for i, ((x, y, w, h), v) in enumerate(zip(rects, views)):
        table[i] = Region(v.data_ptr(), _pitch(v), x, y, w, h, W, H, 0xDEAD, 0)     # (first_tile is not read)
        uses += [Use(i, ty * nx + tx, tx, ty) for ty in range(y // T, (y + h - 1) // T + 1) for tx in range(x // T, (x + w - 1) // T + 1)]
    good = len(uses)
    for j, (x, y, w, h, pw, ph) in enumerate(traps):
        v = views[len(rects) + j]
        table[len(rects) + j] = Region(v.data_ptr(), _pitch(v), x, y, w, h, pw, ph, 0, 0)
        uses.append(Use(len(rects) + j, 0, 0, 0))
    n_regs = len(rects) + len(traps)
    table[n_regs] = Region(views[-1].data_ptr(), 24, 0, 0, 8, 8, W, H, 0, 0)      # behind the table's end: a good window no use may reach
    uses += [Use(n_regs, 0, 0, 0), Use(0xFFFFFFFF, 0, 0, 0),                        # a region index >= n_regs
             Use(0, 6, 0, 0), Use(0, 0xFFFFFFFF, 0, 0),                             # a slot outside both chunks
             Use(1, 1, 1, 0), Use(1, 2, 0, 1), Use(1, 0, 0xFFFFFFFF, 0),            # rect 1 is the pixel (0, 0): tile (0, 0) alone
             Use(4, 0, 0, 0)]                                                       # rect 4 is the last pixel: tile (ny - 1, nx - 1) alone
    order = rng.permutation(len(uses))                                              # the kernel asks no order of the table
    uses = [uses[i] for i in order]
    shared = np.bincount([u.slot for u in uses if u.slot < 6], minlength=6)
    assert (shared >= 2).all() and shared[0] > 10                                   # several uses share every slot
    d_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    d_uses = torch.from_numpy(np.frombuffer(bytes((Use * len(uses))(*uses)), np.uint8).copy()).cuda()
    lib = na._library()
    per = 3 * T * T
    for t0, m in ((4, 2), (0, 4)):                                   # the second chunk first; each launch sees the uses of both
        assert lib.nhw_untile_windows_device(tiles.data_ptr() + t0 * per, d_table.data_ptr(), n_regs, d_uses.data_ptr(), len(uses), t0, m, scale, None) == 0
    torch.cuda.synchronize()
    full = torch.from_numpy(whole).cuda()
    for (x, y, w, h), v in zip(rects, views):
        assert torch.equal(v, full[y:y + h, x:x + w]), (scale, x, y, w, h)
    mask = views_mask(buf, views[:len(rects)])
    assert int(mask.sum()) == sum(3 * w * h for _, _, w, h in rects) and good > len(rects)
    assert bool((buf[~mask] == CANARY).all()), "a byte outside the windows was written"
    # what the host can check is refused
    args = [tiles.data_ptr(), d_table.data_ptr(), n_regs, d_uses.data_ptr(), len(uses), 0, 4, scale, None]
    for at, bad in ((0, None), (0, tiles.data_ptr() + 4), (1, None), (2, 0), (3, None), (4, 0), (5, -1), (6, 0), (7, 3), (7, 0), (7, 8)):
        a = list(args)
        a[at] = bad
        assert lib.nhw_untile_windows_device(*a) == na.NHW_E_ARG, (at, bad)
    torch.cuda.synchronize()
    assert bool((buf[~mask] == CANARY).all())


@pytest.mark.gpu
def test_decode_windows_device_writes_only_the_windows(world):
    import nhwcodec_amd as na
    import torch
    scale, T = 2, 256
    rng = np.random.default_rng(6)
    rects = []
    for ci in (0, 1, BIG, 2):
        H, W = world.full[scale][ci].shape[:2]
        rects += [(ci, *r) for r in fixed_rects(W, H, T, residues=True) + random_rects(W, H, 30, rng, 400, 24)]
    buf, views = dest_views([(w, h) for _, _, _, w, h in rects])
    got = world.dec.decode_windows_device(world.containers, rects, scale, out=views)
    assert world.dec.region_stats() == expected_stats(world.containers, rects, scale, unique=True) and world.dec.region_stats()[0] == 2 + 1 + 6 + 6
    for (ci, x, y, w, h), v, g in zip(rects, views, got):
        assert g is v and np.array_equal(v.cpu().numpy(), world.full[scale][ci][y:y + h, x:x + w]), (ci, x, y, w, h)
    assert bool((buf[~views_mask(buf, views)] == CANARY).all()), "a byte outside the windows was written"
    # without `out`: fresh tensors on the decoder's device; crops straight into the slots of a batch tensor, the others left alone
    crops = [(BIG, x, y, 64, 64) for x, y in ((0, 0), (224, 224), (448, 449), (255, 255))]
    fresh = world.dec.decode_windows_device(world.containers, crops, scale)
    batch = torch.full((6, 64, 64, 3), CANARY, dtype=torch.uint8, device="cuda")
    world.dec.decode_windows_device(world.containers, crops, scale, out=[batch[i] for i in (4, 0, 3, 1)])
    for i, (ci, x, y, w, h) in zip((4, 0, 3, 1), crops):
        k = (4, 0, 3, 1).index(i)
        assert fresh[k].is_cuda and fresh[k].dtype == torch.uint8 and tuple(fresh[k].shape) == (64, 64, 3)
        assert np.array_equal(fresh[k].cpu().numpy(), world.full[scale][ci][y:y + h, x:x + w]) and torch.equal(fresh[k], batch[i])
    assert bool((batch[2] == CANARY).all()) and bool((batch[5] == CANARY).all())
    assert world.dec.region_stats()[0] == 5                          # the four-tile corner twice, (0, 0) again and (ty 2, tx 1): five of the six
    # arguments the wrapper refuses
    with pytest.raises(na.NhwError):
        world.dec.decode_windows_device(world.containers, crops, scale, out=[batch[i] for i in range(3)])
    with pytest.raises(na.NhwError):
        world.dec.decode_windows_device(world.containers, crops[:1], scale, out=[batch[0].transpose(0, 1)])
    with pytest.raises(na.NhwError):
        world.dec.decode_windows_device(world.containers, crops[:1], 3)
    with pytest.raises(na.NhwError):
        world.dec.decode_windows(world.containers, crops[:1], True)
    with pytest.raises(na.NhwError):
        world.dec.decode_windows(world.containers, [(BIG, 0, 0, 1)], 2)


def _call_windows(dec, containers, rects, scale, dst=None):
    """nhw_dec_windows (or, with dst = (addresses, pitches), nhw_dec_windows_to_device) by ctypes: the wrappers raise on a status
    -> (rc, status, the host buffer, its offsets)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    if dst is not None:
        addr, pitch = (np.array(a, np.uint64) for a in dst)
        rc = dec.lib.nhw_dec_windows_to_device(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale,
                                               addr.ctypes.data, pitch.ctypes.data, status.ctypes.data)
        return rc, status, None, None
    out_off = np.zeros(len(rects) + 1, np.uint64)
    out_off[1:] = np.cumsum([3 * r[3] * r[4] + 7 for r in rects])     # 7 bytes of slack behind every window
    out = np.full(int(out_off[-1]) + 16, CANARY, np.uint8)
    rc = dec.lib.nhw_dec_windows(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out.ctypes.data,
                                 out_off.ctypes.data, status.ctypes.data)
    return rc, status, out, out_off


@pytest.mark.gpu
@pytest.mark.parametrize("scale", (2, 4))
def test_a_refused_tile_fails_exactly_the_windows_that_select_it(world, scale):
    import nhwcodec_amd as na
    import torch
    ci, k, T = BIG, 3, 512 // scale                                  # 1023 x 1025, 2 x 3 tiles: tile (ty 1, tx 1)
    W, H, files = parse_container(world.containers[ci])
    bad = list(files)
    bad[k] = b"\x07" + files[k][1:]                                  # res_high 7: the decoder refuses the tile
    broken = make_container(W, H, bad)
    assert na.picture_info(broken) == (W, H)                         # the directory is consistent: the container is well-formed
    full = world.full[scale][ci]
    rng = np.random.default_rng(90 + scale)
    rects = [(0, *r) for r in fixed_rects(full.shape[1], full.shape[0], T, residues=True) + random_rects(full.shape[1], full.shape[0], 60, rng, 400, 24)]
    hit = [k in [n for n, _, _ in selected(W, scale, *r[1:])] for r in rects]
    assert 10 < sum(hit) < len(rects) - 10
    rc, status, out, out_off = _call_windows(world.dec, [broken], rects, scale)
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    check_host_result(rects, status, out, out_off, lambda c: full)   # the failed windows' host bytes are untouched, the others right
    assert world.dec.region_stats() == (6, sum(len(f) for f in bad))
    with pytest.raises(na.NhwError):
        world.dec.decode_windows([broken], rects, scale)
    ok = [r for r, h in zip(rects, hit) if not h]
    for (c, x, y, w, h), g in zip(ok, world.dec.decode_windows([broken], ok, scale)):
        assert np.array_equal(g, full[y:y + h, x:x + w])
    # on the device: a failed rect may have bytes of its own rows written, nothing else is touched
    buf, views = dest_views([(w, h) for _, _, _, w, h in rects])
    rc, status, _, _ = _call_windows(world.dec, [broken], rects, scale, dst=([v.data_ptr() for v in views], [_pitch(v) for v in views]))
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_FORMAT if h else 0 for h in hit]
    for (c, x, y, w, h), v, h_ in zip(rects, views, hit):
        if not h_:
            assert np.array_equal(v.cpu().numpy(), full[y:y + h, x:x + w])
    assert bool((buf[~views_mask(buf, views)] == CANARY).all())


@pytest.mark.gpu
def test_window_statuses_are_per_rect(world):
    import nhwcodec_amd as na
    import torch
    scale = 2
    containers = [world.containers[1], world.containers[BIG][:-1], world.containers[2]]   # 500 x 375 -> 250 x 188; truncated; 1023 x 1025 -> 512 x 513
    rects = [(0, 10, 20, 100, 50),
             (3, 0, 0, 1, 1),                                        # container index out of range
             (2, 500, 0, 13, 5),                                     # x + w > W'
             (1, 0, 0, 5, 5),                                        # a malformed container
             (2, 250, 250, 30, 30),
             (0, 0, 0, 0, 5),                                        # w = 0
             (0, 0, 184, 5, 5),                                      # y + h > H'
             (1, 300, 300, 10, 10),
             (2, 0, 0, 512, 513),
             (0xFFFFFFFF, 0, 0, 1, 1),
             (0, 0, 0, 5, 0),
             (0, 249, 187, 1, 1)]
    want = [0, NHW_E_ARG, NHW_E_ARG, NHW_E_FORMAT, 0, NHW_E_ARG, NHW_E_ARG, NHW_E_FORMAT, 0, NHW_E_ARG, NHW_E_ARG, 0]
    full = {0: world.full[scale][1], 2: world.full[scale][2]}
    rc, status, out, out_off = _call_windows(world.dec, containers, rects, scale)
    assert rc == 0 and status.tolist() == want
    check_host_result(rects, status, out, out_off, lambda c: full[c])
    good = [r for r, s in zip(rects, want) if s == 0]
    assert world.dec.region_stats() == expected_stats(containers, good, scale, unique=True)   # only the good rects reached the decoder
    with pytest.raises(na.NhwError):
        world.dec.decode_windows(containers, rects, scale)
    # the same on the device: the rects that are not NHW_OK leave their destinations untouched
    buf, views = dest_views([(max(w, 1), max(h, 1)) for _, _, _, w, h in rects])
    dst = ([v.data_ptr() for v in views], [_pitch(v) for v in views])
    rc, status, _, _ = _call_windows(world.dec, containers, rects, scale, dst=dst)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == want
    for (ci, x, y, w, h), v, st in zip(rects, views, want):
        if st == 0:
            assert np.array_equal(v.cpu().numpy(), full[ci][y:y + h, x:x + w])
    assert bool((buf[~views_mask(buf, [v for v, st in zip(views, want) if st == 0])] == CANARY).all())
    # the call as a whole fails only for what no rect can answer for
    before = buf.clone()
    assert _call_windows(world.dec, containers, rects[:1], scale, dst=([views[0].data_ptr()], [3 * 100 - 1]))[0] == na.NHW_E_ARG
    assert _call_windows(world.dec, containers, rects[:1], scale, dst=([0], [3 * 100]))[0] == na.NHW_E_ARG
    for s in (0, 3, 8, -1):
        assert _call_windows(world.dec, containers, rects[:1], s)[0] == na.NHW_E_ARG
        assert _call_windows(world.dec, containers, rects[:1], s, dst=([views[0].data_ptr()], [3 * 100]))[0] == na.NHW_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    blob = np.frombuffer(containers[0], np.uint8)
    off = np.array([0, blob.size], np.uint64)
    table = (Rect * 1)(Rect(0, 0, 0, 1, 1))
    st, oo, px = np.zeros(1, np.int32), np.zeros(1, np.uint64), np.zeros(3, np.uint8)
    L, h = world.dec.lib, world.dec.h
    a = ctypes.addressof(table)
    assert L.nhw_dec_windows(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, 2, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == 0 and st[0] == 0
    assert px.tolist() == full[0][0, 0].tolist()
    assert L.nhw_dec_windows(h, blob.ctypes.data, off.ctypes.data, 1, a, 0, 2, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_windows(h, blob.ctypes.data, off.ctypes.data, 0, a, 1, 2, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_windows(h, None, off.ctypes.data, 1, a, 1, 2, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_windows(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, 2, None, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_windows(h, blob.ctypes.data, np.array([5, 0], np.uint64).ctypes.data, 1, a, 1, 2, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    assert L.nhw_dec_windows_to_device(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, 2, None, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    # a handle with a debug stop: no scaled call of any kind (section 14), the full scale still served
    L.nhw_dec_debug_stop_after(h, 3)
    try:
        for s in (2, 4):
            assert L.nhw_dec_windows(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, s, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == na.NHW_E_ARG
    finally:
        L.nhw_dec_debug_stop_after(h, 0)
    assert L.nhw_dec_windows(h, blob.ctypes.data, off.ctypes.data, 1, a, 1, 4, px.ctypes.data, oo.ctypes.data, st.ctypes.data) == 0 and st[0] == 0
    assert px.tolist() == world.full[4][1][0, 0].tolist()


@pytest.mark.gpu
def test_one_handle_serves_files_pictures_regions_and_windows_at_every_scale(world):
    import nhwcodec_amd as na
    cs = [world.containers[1], world.containers[BIG]]
    files = parse_container(cs[1])[2]
    rects = {1: [(1, 500, 500, 100, 100), (0, 0, 0, 500, 375), (1, 0, 0, 1023, 1025), (0, 499, 374, 1, 1), (1, 400, 400, 200, 200)]}
    rects[2] = [(1, 250, 250, 50, 50), (0, 0, 0, 250, 188), (1, 0, 0, 512, 513), (0, 249, 187, 1, 1), (1, 200, 200, 100, 100)]
    rects[4] = [(1, 125, 125, 25, 25), (0, 0, 0, 125, 94), (1, 0, 0, 256, 257), (0, 124, 93, 1, 1), (1, 100, 100, 50, 50)]
    steps = [("files", lambda d: d.decode(files[:4])[0]), ("pictures", lambda d: d.decode_pictures(cs)), ("regions", lambda d: d.decode_regions(cs, rects[1]))]
    for s in SCALES:
        steps += [(f"scaled {s}", lambda d, s=s: d.decode_pictures_scaled(cs, s)), (f"windows {s}", lambda d, s=s: d.decode_windows(cs, rects[s], s))]
    fresh = []
    for name, step in steps:                                         # every step on a handle of its own
        d = na.Decoder(0, max_batch=4)
        fresh.append([np.array(a) for a in step(d)])
        d.close()
    one = na.Decoder(0, max_batch=4)
    for _ in range(2):
        for (name, step), want in zip(steps, fresh):
            got = step(one)
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), name
            if name.startswith("windows"):
                s = int(name.split()[1])
                assert one.region_stats() == expected_stats(cs, rects[s], s, unique=True) and one.region_stats()[0] == 7
                for (ci, x, y, w, h), g in zip(rects[s], got):
                    assert np.array_equal(g, world.full[s][(1, BIG)[ci]][y:y + h, x:x + w])
    one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
def test_cli_window_equals_the_rectangle_of_the_scaled_bmp(cli, world, tmp_path, scale):
    """X, Y count from the top left of the scaled picture as a viewer shows the (bottom-up) BMP"""
    ci = BIG
    H, W = world.full[scale][ci].shape[:2]
    (tmp_path / "p.nhwp").write_bytes(world.containers[ci])
    rc, out, err = run(cli, "--scale", str(scale), "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "full.bmp"))
    assert rc == 0, err
    whole = (tmp_path / "full.bmp").read_bytes()
    stride = (3 * W + 3) & ~3
    rows = np.frombuffer(whole[54:], np.uint8).reshape(H, stride)
    assert np.array_equal(rows[:, :3 * W].reshape(H, W, 3), world.full[scale][ci])
    for x, y, w, h in ((0, 0, W, 3), (W // 2 - 10, H - 25, 30, 25), (W // 2 - 2, H // 4, 5, H // 2), (W - 1, H - 1, 1, 1)):   # the top rows; the bottom rows; ...
        rc, out, err = run(cli, "--picture", str(tmp_path / "p.nhwp"), str(tmp_path / "r.bmp"), "--window", f"{scale},{x},{y},{w},{h}")
        assert rc == 0 and f"{w} x {h}" in out, err
        b = (tmp_path / "r.bmp").read_bytes()
        rs = (3 * w + 3) & ~3
        assert len(b) == 54 + rs * h
        hdr = bytearray(b[:54])
        assert struct.unpack_from("<ii", hdr, 18) == (w, h) and struct.unpack_from("<I", hdr, 2)[0] == len(b) and struct.unpack_from("<I", hdr, 34)[0] == rs * h
        ref = bytearray(whole[:54])
        for o in (2, 18, 22, 34):
            hdr[o:o + 4] = ref[o:o + 4]
        assert hdr == ref                                           # the scaled picture's header but for the size fields
        got = np.frombuffer(b[54:], np.uint8).reshape(h, rs)
        assert (got[:, 3 * w:] == 0).all()
        assert np.array_equal(got[:, :3 * w], rows[H - y - h:H - y, 3 * x:3 * (x + w)]), (scale, x, y, w, h)
