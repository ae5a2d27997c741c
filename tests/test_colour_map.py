"""A colour map a sample in the crop, resample and warp stores, on the MI355X: the mapped forms of k_resize_to_tensor,
k_area_to_tensor, k_cubic_to_tensor and k_warp_to_tensor at three and at one byte a pixel behind nhw_resample_mapped_to_tensor_device and
nhw_warp_mapped_to_tensor_device, and the decoder's nhw_dec_crops_mapped_to_device and nhw_dec_warps_mapped_to_device with the Python layer's
`colours`.  The expected value never comes from the code under test: it is the existing UNMAPPED call's bytes (U8 / HWC / BGR / file rows, pinned
by the resamplers' and the warp's own tests) put through the rule in numpy int64 (colour_cases.apply_map) and then through the exact value rule
(tensor_cases.expected_tensor, grey_cases.expected_grey_tensor), compared as bit patterns.  Every batch lies between guards, and an entry that
must store nothing keeps its canary."""
import ctypes
import math

import numpy as np
import pytest

from tests.colour_cases import (GAIN, MAPS, NHW_E_ARG, OFFSET, apply_grey, apply_map, colour_views, drawn, launch, map_table, picture_table, slot_bits,
                                untouched)
from tests.grey_cases import GREY_FORMATS, expected_grey_tensor, grey_format
from tests.grey_picture_cases import grey_views
from tests.picture_cases import Rect, World, expected_stats
from tests.support import CANARY
from tests.tensor_cases import ALL_FORMATS, expected_tensor, tensor_bits, tensor_format

pytestmark = pytest.mark.gpu
# W, H, pitch extra, misalignment: one pixel; an odd address; a padded pitch; and one that holds every byte value
SOURCES = [(1, 1, 0, 0), (37, 23, 0, 1), (517, 301, 11, 4), (32, 24, 0, 0)]
OUTPUTS = [(1, 1), (5, 7), (224, 224), (300, 3)]                     # out_w, out_h; 300 is wider than a pass's 256 lanes
ALL_FORMATS_AT = (5, 7)
LIMITS = {"two_tap": 0, "area": 128, "cubic": 32}
NUMBER = {"two_tap": 0, "area": 1, "cubic": 2}
SIZES = [(1, 700), (500, 375), (1023, 1025)]
SMALL, BIG = 1, 2


def _byte_format(channels):
    return tensor_format("uint8", "HWC", "BGR", "file") if channels == 3 else grey_format("uint8", "HWC", "file")


def _formats(out, channels):
    if channels == 3:
        return [tensor_format(*f) for f in ALL_FORMATS] if out == ALL_FORMATS_AT else [tensor_format("uint8", "HWC", "BGR", "file"), tensor_format("float16", "CHW", "RGB", "reversed")]
    return [grey_format(*f) for f in GREY_FORMATS] if out == ALL_FORMATS_AT else [grey_format("uint8", "HWC", "file"), grey_format("float16", "CHW", "reversed")]


class Sources:
    pass


@pytest.fixture(scope="module")
def sources():
    import torch
    import nhwcodec_amd as na
    s = Sources()
    s.buf3, s.views3 = colour_views(SOURCES, 2401)
    s.buf1, s.views1, _ = grey_views(SOURCES, 2402)
    ramp = (np.arange(32 * 24) % 256).astype(np.uint8).reshape(24, 32)
    s.views1[-1].copy_(torch.from_numpy(ramp).cuda())
    for v in (s.views3[-1], s.views1[-1]):
        assert len(np.unique(v.cpu().numpy())) == 256
    assert s.views3[1].data_ptr() % 2 == 1 and s.views1[1].data_ptr() % 2 == 1 and s.views3[2].stride(0) == 3 * 517 + 11
    s.tables = {3: lambda which: picture_table([s.views3[k] for k in which], na), 1: lambda which: picture_table([s.views1[k] for k in which], na)}
    return s


def _pixels(slot, out_h, out_w, channels):
    return slot.reshape((out_h, out_w, 3) if channels == 3 else (out_h, out_w))


def _expect(px, twelve, fmt, channels):
    """the unmapped call's bytes through the rule and the value rule"""
    return expected_tensor(apply_map(px, twelve), fmt) if channels == 3 else expected_grey_tensor(apply_grey(px, twelve), fmt)


def _assert_slot(slot, px, twelve, fmt, out_h, out_w, channels, what):
    got, want = slot_bits(slot, fmt, out_h, out_w), _expect(px, twelve, fmt, channels)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


def _within(filter, k, out_w, out_h):
    return not LIMITS[filter] or (SOURCES[k][0] <= LIMITS[filter] * out_w and SOURCES[k][1] <= LIMITS[filter] * out_h)


@pytest.mark.parametrize("out", OUTPUTS, ids=lambda o: f"{o[0]}x{o[1]}")
@pytest.mark.parametrize("filter", ("two_tap", "area", "cubic"))
@pytest.mark.parametrize("channels", (3, 1))
def test_mapped_resamplers_equal_the_rule_on_the_unmapped_bytes(sources, channels, filter, out):
    out_w, out_h = out
    which = [k for k in range(len(SOURCES)) for _ in (0, 1)]         # every source plain and mirrored
    flags = [j % 2 for j in range(len(which))]
    ok = [_within(filter, k, out_w, out_h) for k in which]
    assert any(ok)
    table = sources.tables[channels](which)
    twelves = drawn(len(which), first=OUTPUTS.index(out) + 4 * NUMBER[filter])
    maps = map_table(twelves)
    for fl in (flags, None):                                         # with a flag table, and without one: nothing is mirrored
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, filter=NUMBER[filter], flags=fl)
        assert rc == 0 and intact
        for fmt in _formats(out, channels) if fl is not None else _formats(out, channels)[:1]:
            rc, slots, intact = launch(table, out_w, out_h, fmt, channels, filter=NUMBER[filter], flags=fl, maps=maps)
            assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
            for i, good in enumerate(ok):
                if good:
                    _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, channels), twelves[i], fmt, out_h, out_w, channels, f"{filter} to {out_w} x {out_h}, entry {i}, {fmt}")
                else:
                    assert untouched(slots[i]) and untouched(ref[i]), f"{filter}: entry {i} beyond the limit was written"


def _rotation(w, h, out_w, out_h, degrees):
    """output pixel centres to source coordinates: a turn about both centres, the output's grid a fifth larger than the picture, so that taps
    fall outside it; a step stays below the warp's limit of 64"""
    s = min(1.2 * max(w / out_w, h / out_h), 60.0)
    c, n = s * math.cos(math.radians(degrees)), s * math.sin(math.radians(degrees))
    return [[c, -n, w / 2 - (c * out_w / 2 - n * out_h / 2)], [n, c, h / 2 - (n * out_w / 2 + c * out_h / 2)]]


def _warp_table(na, fixed, fill, replicate):
    t = np.zeros(len(fixed), na.WARP_DTYPE)
    for i, (a, b, c, d, e, f) in enumerate(fixed):
        t[i] = (c, f, a, b, d, e, fill, int(replicate), 0)
    return t


@pytest.fixture
def walks():
    """nhw_debug_warp_row_limit for the test, the rule's own limit back behind it"""
    import nhwcodec_amd as na
    L = na._library()
    yield {"blocks": lambda: L.nhw_debug_warp_row_limit(-1), "rows": lambda: L.nhw_debug_warp_row_limit(1 << 22), "rule": lambda: L.nhw_debug_warp_row_limit(-2)}
    L.nhw_debug_warp_row_limit(-2)


@pytest.mark.parametrize("out", OUTPUTS, ids=lambda o: f"{o[0]}x{o[1]}")
@pytest.mark.parametrize("channels", (3, 1))
def test_mapped_warp_equals_the_rule_on_the_unmapped_bytes(sources, walks, channels, out):
    import nhwcodec_amd as na
    out_w, out_h = out
    which = [k for k in range(len(SOURCES)) for _ in (0, 10, 30)]
    fixed = [na.warp_fixed(_rotation(SOURCES[k][0], SOURCES[k][1], out_w, out_h, deg)) for k in range(len(SOURCES)) for deg in (0, 10, 30)]
    table = sources.tables[channels](which)
    twelves = drawn(len(which), first=7 + OUTPUTS.index(out))
    maps = map_table(twelves)
    for border, fill in (("fill", (201, 17, 94)), ("replicate", (9, 8, 7))):
        warps = _warp_table(na, fixed, fill, border == "replicate")
        walks["rule"]()
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, warps=warps)
        assert rc == 0 and intact
        if border == "fill" and out_w * out_h > 1:                   # the border colour went through the blend and is mapped like any pixel
            assert any((_pixels(r, out_h, out_w, channels).reshape(out_h * out_w, -1) == np.array(fill[:channels])).all(axis=1).any() for r in ref), "no tap fell outside a picture"
        for walk in ("blocks", "rows"):
            walks[walk]()
            for fmt in _formats(out, channels) if walk == "blocks" else _formats(out, channels)[-1:]:
                rc, slots, intact = launch(table, out_w, out_h, fmt, channels, warps=warps, maps=maps)
                assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
                for i in range(len(which)):
                    _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, channels), twelves[i], fmt, out_h, out_w, channels, f"warp to {out_w} x {out_h}, {border}, {walk}, entry {i}, {fmt}")


@pytest.mark.parametrize("channels", (3, 1))
def test_identity_maps_give_the_unmapped_tensor(sources, channels):
    import nhwcodec_amd as na
    out_w, out_h = ALL_FORMATS_AT
    which = [0, 1, 2, 3]
    table = sources.tables[channels](which)
    maps = map_table([MAPS["identity"]] * len(which))
    warps = _warp_table(na, [na.warp_fixed(_rotation(SOURCES[k][0], SOURCES[k][1], out_w, out_h, 20)) for k in which], (5, 6, 7), False)
    for fmt in _formats(ALL_FORMATS_AT, channels):
        for kw in (dict(filter=0, flags=[0, 1, 1, 0]), dict(filter=1, flags=[1, 0, 0, 1]), dict(filter=2), dict(warps=warps)):
            rc0, plain, ok0 = launch(table, out_w, out_h, fmt, channels, **kw)
            rc1, mapped, ok1 = launch(table, out_w, out_h, fmt, channels, maps=maps, **kw)
            assert rc0 == 0 and rc1 == 0 and ok0 and ok1
            for i, (a, b) in enumerate(zip(plain, mapped)):
                assert np.array_equal(a, b), (fmt, kw.get("filter", "warp"), i)
            assert any(not untouched(s) for s in mapped)


@pytest.mark.parametrize("channels", (3, 1))
def test_entries_that_store_nothing(sources, channels):
    import nhwcodec_amd as na
    out_w, out_h = 5, 7
    which = [1, 3, 1, 3, 1, 3, 2, 3]                                 # entry 6, 517 x 301, is beyond the cubic filter's 32 x and within the area filter's 128 x
    table = sources.tables[channels](which)
    twelves = drawn(len(which), first=2)
    twelves[0] = (GAIN + 1,) + twelves[0][1:]                        # a matrix entry beyond 2^20
    twelves[2] = twelves[2][:10] + (-OFFSET - 1,) + twelves[2][11:]  # an offset beyond 2^28
    maps = map_table(twelves, reserved={4: (3, 1)})                  # a reserved word set
    other = {5: lambda s: 0}                                         # a zero address
    fmt = _formats((0, 0), channels)[1]
    for name, kw in (("two_tap", dict(filter=0)), ("area", dict(filter=1)), ("cubic", dict(filter=2)),
                     ("warp", dict(warps=_warp_table(na, [na.warp_fixed([[2, 0, 0], [0, 2, 0]])] * len(which), (1, 2, 3), False)))):
        dead = {0, 2, 4, 5} | ({6} if name == "cubic" else set())
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, **kw)
        assert rc == 0 and intact
        rc, slots, intact = launch(table, out_w, out_h, fmt, channels, maps=maps, other_addr=other, **kw)
        assert rc == 0 and intact, name
        for i in range(len(which)):
            if i in dead:
                assert untouched(slots[i]), f"{name}: entry {i} was written"
            else:
                _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, channels), twelves[i], fmt, out_h, out_w, channels, f"{name}: entry {i} beside the dead ones")


def test_call_level_refusals(sources):
    import nhwcodec_amd as na
    out_w, out_h = 5, 7
    which = [1, 3]
    twelves = drawn(2, first=1)
    maps = map_table(twelves)
    warps = _warp_table(na, [na.warp_fixed([[2, 0, 0], [0, 2, 0]])] * 2, (1, 2, 3), False)
    for channels in (3, 1):
        table = sources.tables[channels](which)
        fmt = _formats((0, 0), channels)[1]
        for kw in (dict(filter=0), dict(filter=2, flags=[1, 0]), dict(warps=warps)):
            rc, slots, intact = launch(table, out_w, out_h, fmt, channels, null_maps=True, **kw)     # a NULL table of maps
            assert rc == NHW_E_ARG and intact and all(untouched(s) for s in slots), kw
            for spoil in (dict(reserved=1), dict(dtype=4), dict(layout=2), dict(channels=3), dict(rows=2)):
                class Spoilt:
                    dtype, shape = fmt.dtype, fmt.shape

                    @staticmethod
                    def c_struct():
                        c = fmt.c_struct()
                        for k, v in spoil.items():
                            setattr(c, k, v)
                        return c
                rc, slots, intact = launch(table, out_w, out_h, Spoilt, channels, maps=maps, **kw)
                assert rc == NHW_E_ARG and intact and all(untouched(s) for s in slots), (kw, spoil)
            for o in ((0, 7), (5, 4097)):
                rc, slots, intact = launch(table, o[0], o[1], fmt, channels, maps=maps, **kw)
                assert rc == NHW_E_ARG and intact and all(untouched(s) for s in slots)
        rc, slots, intact = launch(table, out_w, out_h, fmt, channels, filter=3, maps=maps)
        assert rc == NHW_E_ARG and all(untouched(s) for s in slots)
    # a GREY format over three-byte pictures is simply the grey call: the first W bytes of each row are its pixels
    table = sources.tables[3](which)
    grey = grey_format("bfloat16", "CHW", "reversed")
    for kw in (dict(filter=1, flags=[0, 1]), dict(warps=warps)):
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(1), 1, **kw)
        assert rc == 0 and intact
        rc, slots, intact = launch(table, out_w, out_h, grey, 1, maps=maps, **kw)
        assert rc == 0 and intact
        for i in range(2):
            _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, 1), twelves[i], grey, out_h, out_w, 1, f"a grey format over three-byte pictures, entry {i}")


# ---------------------------------------------------------------- through the decoder
@pytest.fixture(scope="module")
def world():
    """test_warp.py's world: pictures of SIZES cut from one seeded scene as containers at q20, and a decoder of 4 tiles a chunk"""
    import nhwcodec_amd as na
    w = World()
    enc = na.Encoder(0, max_batch=24)
    scene = na.untile_images(enc.synth_device(24, 1300).cpu().numpy(), 4, 6)
    w.containers = enc.encode_pictures([np.ascontiguousarray(scene[17:17 + h, 29:29 + wd]) for wd, h in SIZES], 20)
    enc.close()
    w.dec = na.Decoder(0, max_batch=4)
    yield w
    w.dec.close()


CROPS = [(BIG, 10, 20, 40, 30), (BIG, 500, 490, 70, 50), (BIG, 300, 200, 140, 100), (SMALL, 0, 0, 64, 48), (SMALL, 100, 50, 33, 27), (BIG, 511, 511, 150, 130)]
OUT = (24, 32)                                                       # out_h, out_w: the crops above take the scales 1, 2 and 4


def _float_maps(twelves):
    """the twelve integers as the Python layer takes them: an integer array [12]"""
    return [np.array(t, np.int64) for t in twelves]


@pytest.mark.parametrize("filter", ("two_tap", "area", "cubic"))
@pytest.mark.parametrize("channels", (3, 1))
def test_decode_crops_with_colours(world, channels, filter):
    twelves = drawn(len(CROPS), first=3 + NUMBER[filter])
    flips = [i % 2 == 1 for i in range(len(CROPS))]
    colours = _float_maps(twelves) if channels == 3 else [(t[0] / 65536, t[9] / 65536) for t in twelves]
    call = world.dec.decode_crops_device if channels == 3 else world.dec.decode_crops_grey_device
    ref, scales = call(world.containers, CROPS, OUT, _byte_format(channels), flips=flips, filter=filter)
    assert sorted(set(scales)) == [1, 2, 4]                           # scale=None: mixed scales take part
    ref = ref.cpu().numpy()
    for fmt in _formats((0, 0), channels):
        got, again = call(world.containers, CROPS, OUT, fmt, flips=flips, filter=filter, colours=colours)
        assert again == scales and got.dtype == fmt.dtype and tuple(got.shape) == (len(CROPS),) + fmt.shape(*OUT)
        bits = tensor_bits(got)
        for i in range(len(CROPS)):
            px = ref[i] if channels == 3 else ref[i].reshape(OUT)
            want = _expect(px, twelves[i], fmt, channels)
            assert np.array_equal(bits[i], want), (filter, fmt, i)


@pytest.mark.parametrize("channels", (3, 1))
def test_decode_warps_with_colours(world, channels):
    import nhwcodec_amd as na
    which = [c[0] for c in CROPS]
    mats = [na.crop_warp(x - 3, y - 3, w, h, OUT, angle=0.3 * i, flip=i % 2 == 0) for i, (_, x, y, w, h) in enumerate(CROPS)]    # the first ones reach outside their picture
    twelves = drawn(len(CROPS), first=6)
    colours = _float_maps(twelves) if channels == 3 else [(t[0] / 65536, t[9] / 65536) for t in twelves]
    call = world.dec.decode_warps_device if channels == 3 else world.dec.decode_warps_grey_device
    for border, fill in (("fill", (201, 17, 94)), ("replicate", (0, 0, 0))):
        fill = fill if channels == 3 else fill[0]
        ref, scales = call(world.containers, which, mats, OUT, _byte_format(channels), fill=fill, border=border)
        ref = ref.cpu().numpy()
        fmt = _formats((0, 0), channels)[1]
        got, again = call(world.containers, which, mats, OUT, fmt, fill=fill, border=border, colours=colours)
        assert again == scales and len(set(scales)) > 1
        bits = tensor_bits(got)
        for i in range(len(CROPS)):
            px = ref[i] if channels == 3 else ref[i].reshape(OUT)
            assert np.array_equal(bits[i], _expect(px, twelves[i], fmt, channels)), (border, i)


def _call_crops_mapped(dec, containers, rects, scale, out_w, out_h, fmt, maps, addrs, filter=0, null_maps=False):
    """nhw_dec_crops_mapped_to_device by ctypes -> (rc, status)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    addr = np.array(addrs, np.uint64)
    maps = np.ascontiguousarray(maps)
    c = fmt.c_struct()
    rc = dec.lib.nhw_dec_crops_mapped_to_device(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out_w, out_h,
                                                ctypes.byref(c), None, None if null_maps else maps.ctypes.data, addr.ctypes.data, status.ctypes.data, filter)
    return rc, status


def test_a_rect_with_a_map_beyond_the_limits(world):
    """through the C entry: NHW_E_ARG for the rect, no tile selected for it -- alone it reports 0 tiles --, its destination keeps the canary
    and the other rects are right; a NULL table of maps is a call-level refusal"""
    import torch
    fmt = tensor_format("float16", "CHW", "RGB", "reversed")
    out_h, out_w = 6, 8
    per, es = 3 * out_w * out_h, 2
    rects = [(BIG, 0, 0, 60, 50), (BIG, 600, 1024, 65, 1), (SMALL, 10, 10, 64, 64), (BIG, 3, 3, 30, 30)]
    twelves = drawn(len(rects), first=9)
    maps = map_table(twelves)
    maps[1]["m"][2, 1] = -GAIN - 1
    ok = [r for i, r in enumerate(rects) if i != 1]
    ref, _ = world.dec.decode_crops_device(world.containers, ok, (out_h, out_w), _byte_format(3), scale=1)
    ref = ref.cpu().numpy()
    guard = 4096
    buf = torch.full((2 * guard + len(rects) * per * es,), CANARY, dtype=torch.uint8, device="cuda")
    addrs = [buf.data_ptr() + guard + i * per * es for i in range(len(rects))]
    rc, status = _call_crops_mapped(world.dec, world.containers, rects, 1, out_w, out_h, fmt, maps, addrs)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [0, NHW_E_ARG, 0, 0]
    assert world.dec.region_stats() == expected_stats(world.containers, ok, 1, unique=True)
    assert expected_stats(world.containers, rects, 1, unique=True)[0] == world.dec.region_stats()[0] + 1     # rect 1 would have brought a tile of its own
    host = buf.cpu().numpy()
    assert (host[:guard] == CANARY).all() and (host[guard + len(rects) * per * es:] == CANARY).all()
    good = iter(range(len(ok)))
    for i in range(len(rects)):
        slot = host[guard + i * per * es: guard + (i + 1) * per * es]
        if i == 1:
            assert untouched(slot)
        else:
            _assert_slot(slot, ref[next(good)], twelves[i], fmt, out_h, out_w, 3, f"rect {i}")
    buf.fill_(CANARY)
    rc, status = _call_crops_mapped(world.dec, world.containers, rects[1:2], 1, out_w, out_h, fmt, maps[1:2], addrs[1:2])      # only that rect
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [NHW_E_ARG] and world.dec.region_stats() == (0, 0) and bool((buf == CANARY).all())
    rc, status = _call_crops_mapped(world.dec, world.containers, ok, 1, out_w, out_h, fmt, maps[[0, 2, 3]], addrs[:3], null_maps=True)
    assert rc == NHW_E_ARG and (status == 99).all() and b"bad argument" in world.dec.lib.nhw_dec_last_error()
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())


def test_one_handle_serves_unmapped_and_mapped_calls_in_turn(world):
    fmt = tensor_format("float32", "HWC", "RGB", "file")
    twelves = drawn(len(CROPS), first=11)
    first, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic")
    first = tensor_bits(first).copy()
    mapped, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic", colours=_float_maps(twelves))
    last, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic")
    assert np.array_equal(first, tensor_bits(last)) and not np.array_equal(first, tensor_bits(mapped))


def test_colour_matrix_through_the_python_layer(sources):
    """a float matrix on (R, G, B, 1) reaches the kernel as colour_fixed of it: saturation 0 makes the three channels one"""
    import nhwcodec_amd as na
    fmt = tensor_format("uint8", "HWC", "RGB", "file")
    pics = [sources.views3[2], sources.views3[3]]
    m = [na.colour_matrix(saturation=0), na.colour_compose(na.colour_matrix(brightness=1.3, hue=0.1), -np.eye(3, 4) + np.array([[0, 0, 0, 255.0]] * 3))]
    ref = na.resize_to_tensor_device(pics, (9, 11), _byte_format(3), flips=[True, False], filter="area").cpu().numpy()
    got = na.resize_to_tensor_device(pics, (9, 11), fmt, flips=[True, False], filter="area", colours=m).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], expected_tensor(apply_map(ref[i], na.colour_fixed(m[i])), fmt)), i
    assert (got[0][..., 0] == got[0][..., 1]).all() and (got[0][..., 1] == got[0][..., 2]).all()
    grey = grey_format("float32", "CHW", "file")
    ref = na.warp_grey_to_tensor_device([sources.views1[2]], [_rotation(517, 301, 11, 9, 12)], (9, 11), _byte_format(1), fill=40).cpu().numpy()
    got = na.warp_grey_to_tensor_device([sources.views1[2]], [_rotation(517, 301, 11, 9, 12)], (9, 11), grey, fill=40, colours=[(-1.0, 255.0)])
    assert np.array_equal(tensor_bits(got)[0], expected_grey_tensor(255 - ref[0].reshape(9, 11), grey))
