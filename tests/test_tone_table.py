"""A tone table a sample in the crop, resample and warp stores, on the MI355X: the toned forms of k_resize_to_tensor,
k_area_to_tensor, k_cubic_to_tensor and k_warp_to_tensor at three and at one byte a pixel behind nhw_resample_toned_to_tensor_device and
nhw_warp_toned_to_tensor_device, and the decoder's nhw_dec_crops_toned_to_device and nhw_dec_warps_toned_to_device with the Python layer's
`tones`.  The expected value never comes from the code under test: it is the existing UNMAPPED call's bytes -- the MAPPED call's where the toned
call has maps -- in U8 / HWC / BGR / file rows (pinned by the resamplers', the warp's and the colour map's own tests) put through the table in
numpy (tone_cases.apply_tone) and then through the exact value rule (tensor_cases.expected_tensor, grey_cases.expected_grey_tensor), compared as
bit patterns.  Every batch lies between guards, and an entry that must store nothing keeps its canary."""
import ctypes
import math

import numpy as np
import pytest

from tests.colour_cases import GAIN, colour_views, map_table, picture_table, slot_bits, untouched
from tests.colour_cases import drawn as drawn_maps
from tests.grey_cases import GREY_FORMATS, expected_grey_tensor, grey_format
from tests.grey_picture_cases import grey_views
from tests.picture_cases import Rect, World
from tests.support import CANARY
from tests.tensor_cases import ALL_FORMATS, expected_tensor, tensor_bits, tensor_format
from tests.tone_cases import NHW_E_ARG, TABLES, apply_tone, apply_tone_grey, drawn, launch, tone_table

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
    s.buf3, s.views3 = colour_views(SOURCES, 2511)
    s.buf1, s.views1, _ = grey_views(SOURCES, 2512)
    ramp = (np.arange(32 * 24) % 256).astype(np.uint8).reshape(24, 32)
    s.views1[-1].copy_(torch.from_numpy(ramp).cuda())
    for v in (s.views3[-1], s.views1[-1]):
        assert len(np.unique(v.cpu().numpy())) == 256
    assert s.views3[1].data_ptr() % 2 == 1 and s.views1[1].data_ptr() % 2 == 1 and s.views3[2].stride(0) == 3 * 517 + 11
    s.tables = {3: lambda which: picture_table([s.views3[k] for k in which], na), 1: lambda which: picture_table([s.views1[k] for k in which], na)}
    return s


def _pixels(slot, out_h, out_w, channels):
    return slot.reshape((out_h, out_w, 3) if channels == 3 else (out_h, out_w))


def _expect(px, table, fmt, channels):
    """the reference call's bytes through the table and the value rule"""
    return expected_tensor(apply_tone(px, table), fmt) if channels == 3 else expected_grey_tensor(apply_tone_grey(px, table), fmt)


def _assert_slot(slot, px, table, fmt, out_h, out_w, channels, what):
    got, want = slot_bits(slot, fmt, out_h, out_w), _expect(px, table, fmt, channels)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


def _within(filter, k, out_w, out_h):
    return not LIMITS[filter] or (SOURCES[k][0] <= LIMITS[filter] * out_w and SOURCES[k][1] <= LIMITS[filter] * out_h)


@pytest.mark.parametrize("out", OUTPUTS, ids=lambda o: f"{o[0]}x{o[1]}")
@pytest.mark.parametrize("filter", ("two_tap", "area", "cubic"))
@pytest.mark.parametrize("channels", (3, 1))
def test_toned_resamplers_equal_the_table_on_the_reference_bytes(sources, channels, filter, out):
    out_w, out_h = out
    which = [k for k in range(len(SOURCES)) for _ in (0, 1)]         # every source plain and mirrored
    flags = [j % 2 for j in range(len(which))]
    ok = [_within(filter, k, out_w, out_h) for k in which]
    assert any(ok)
    table = sources.tables[channels](which)
    tabs = drawn(len(which), first=OUTPUTS.index(out) + 4 * NUMBER[filter])      # a different table for every sample of the batch
    assert len({t.tobytes() for t in tabs}) == len(tabs)
    tones = tone_table(tabs)
    twelves = drawn_maps(len(which), first=OUTPUTS.index(out) + NUMBER[filter])
    maps = map_table(twelves)
    for fl in (flags, None):                                         # with a flag table, and without one: nothing is mirrored
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, filter=NUMBER[filter], flags=fl)
        assert rc == 0 and intact
        rc, mref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, filter=NUMBER[filter], flags=fl, maps=maps)
        assert rc == 0 and intact
        formats = _formats(out, channels) if fl is not None else _formats(out, channels)[:1]
        for fmt, with_maps in [(f, False) for f in formats] + [(formats[-1], True)]:
            rc, slots, intact = launch(table, out_w, out_h, fmt, channels, filter=NUMBER[filter], flags=fl, maps=maps if with_maps else None, tones=tones)
            assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
            for i, good in enumerate(ok):
                if good:
                    _assert_slot(slots[i], _pixels((mref if with_maps else ref)[i], out_h, out_w, channels), tabs[i], fmt, out_h, out_w, channels,
                                 f"{filter} to {out_w} x {out_h}, entry {i}, {fmt}, {'with' if with_maps else 'no'} maps")
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
def test_toned_warp_equals_the_table_on_the_reference_bytes(sources, walks, channels, out):
    import nhwcodec_amd as na
    out_w, out_h = out
    which = [k for k in range(len(SOURCES)) for _ in (0, 10, 30)]
    fixed = [na.warp_fixed(_rotation(SOURCES[k][0], SOURCES[k][1], out_w, out_h, deg)) for k in range(len(SOURCES)) for deg in (0, 10, 30)]
    table = sources.tables[channels](which)
    tabs = drawn(len(which), first=7 + OUTPUTS.index(out))
    tones = tone_table(tabs)
    twelves = drawn_maps(len(which), first=5 + OUTPUTS.index(out))
    maps = map_table(twelves)
    for border, fill in (("fill", (201, 17, 94)), ("replicate", (9, 8, 7))):
        warps = _warp_table(na, fixed, fill, border == "replicate")
        walks["rule"]()
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, warps=warps)
        assert rc == 0 and intact
        rc, mref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, warps=warps, maps=maps)
        assert rc == 0 and intact
        if border == "fill" and out_w * out_h > 1:                   # the border colour went through the blend and goes through the table like any pixel
            assert any((_pixels(r, out_h, out_w, channels).reshape(out_h * out_w, -1) == np.array(fill[:channels])).all(axis=1).any() for r in ref), "no tap fell outside a picture"
        for walk in ("blocks", "rows"):
            walks[walk]()
            formats = _formats(out, channels) if walk == "blocks" else _formats(out, channels)[-1:]
            for fmt, with_maps in [(f, False) for f in formats] + [(formats[-1], True)]:
                rc, slots, intact = launch(table, out_w, out_h, fmt, channels, warps=warps, maps=maps if with_maps else None, tones=tones)
                assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
                for i in range(len(which)):
                    _assert_slot(slots[i], _pixels((mref if with_maps else ref)[i], out_h, out_w, channels), tabs[i], fmt, out_h, out_w, channels,
                                 f"warp to {out_w} x {out_h}, {border}, {walk}, entry {i}, {fmt}, {'with' if with_maps else 'no'} maps")


@pytest.mark.parametrize("name", list(TABLES))
@pytest.mark.parametrize("channels", (3, 1))
def test_each_named_table(sources, channels, name):
    """one table for the whole batch, over the picture that holds every byte value in every channel, each kernel"""
    import nhwcodec_amd as na
    out_w, out_h = 32, 24                                            # the ramp to its own size: the identity resample, every byte value reaches the table
    which = [3, 1]
    table = sources.tables[channels](which)
    tones = tone_table([TABLES[name]] * 2)
    fmt = _formats((0, 0), channels)[1]
    warps = _warp_table(na, [na.warp_fixed(_rotation(SOURCES[k][0], SOURCES[k][1], out_w, out_h, 20)) for k in which], (5, 6, 7), False)
    for kw in (dict(filter=0, flags=[0, 1]), dict(filter=1), dict(filter=2), dict(warps=warps)):
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, **kw)
        assert rc == 0 and intact
        if "filter" in kw and kw["filter"] < 2:
            assert len(np.unique(_pixels(ref[0], out_h, out_w, channels).reshape(out_h * out_w, -1)[:, 0])) == 256
        rc, slots, intact = launch(table, out_w, out_h, fmt, channels, tones=tones, **kw)
        assert rc == 0 and intact
        for i in range(2):
            _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, channels), TABLES[name], fmt, out_h, out_w, channels, f"{name}, {kw.get('filter', 'warp')}, entry {i}")


def test_a_grey_call_ignores_the_other_two_rows(sources):
    out_w, out_h = 32, 24
    which = [3, 2]
    table = sources.tables[1](which)
    rng = np.random.default_rng(2513)
    tabs = [np.stack([TABLES["permutations"][1], rng.integers(0, 256, 256, dtype=np.uint8), rng.integers(0, 256, 256, dtype=np.uint8)]) for _ in which]
    fmt = grey_format("float32", "CHW", "file")
    rc, ref, intact = launch(table, out_w, out_h, _byte_format(1), 1, filter=0)
    assert rc == 0 and intact
    rc, slots, intact = launch(table, out_w, out_h, fmt, 1, filter=0, tones=tone_table(tabs))
    assert rc == 0 and intact
    clean = [np.stack([t[0], t[0] * 0, t[0] * 0]) for t in tabs]
    rc, again, intact = launch(table, out_w, out_h, fmt, 1, filter=0, tones=tone_table(clean))
    assert rc == 0 and intact
    for i in range(2):
        _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, 1), tabs[i], fmt, out_h, out_w, 1, f"entry {i}")
        assert np.array_equal(slots[i], again[i])


@pytest.mark.parametrize("channels", (3, 1))
def test_identity_tables_give_the_unmapped_and_the_mapped_tensor(sources, channels):
    import nhwcodec_amd as na
    out_w, out_h = ALL_FORMATS_AT
    which = [0, 1, 2, 3]
    table = sources.tables[channels](which)
    tones = tone_table([TABLES["identity"]] * len(which))
    maps = map_table(drawn_maps(len(which), first=3))
    warps = _warp_table(na, [na.warp_fixed(_rotation(SOURCES[k][0], SOURCES[k][1], out_w, out_h, 20)) for k in which], (5, 6, 7), False)
    for fmt in _formats(ALL_FORMATS_AT, channels):
        for kw in (dict(filter=0, flags=[0, 1, 1, 0]), dict(filter=1, flags=[1, 0, 0, 1]), dict(filter=2), dict(warps=warps)):
            for m in (None, maps):                                   # a NULL map: the unmapped call; a map: the mapped call
                rc0, plain, ok0 = launch(table, out_w, out_h, fmt, channels, maps=m, **kw)
                rc1, toned, ok1 = launch(table, out_w, out_h, fmt, channels, maps=m, tones=tones, **kw)
                assert rc0 == 0 and rc1 == 0 and ok0 and ok1
                for i, (a, b) in enumerate(zip(plain, toned)):
                    assert np.array_equal(a, b), (fmt, kw.get("filter", "warp"), m is not None, i)
                assert any(not untouched(s) for s in toned)


@pytest.mark.parametrize("channels", (3, 1))
def test_entries_that_store_nothing(sources, channels):
    import nhwcodec_amd as na
    out_w, out_h = 5, 7
    which = [1, 3, 1, 3, 1, 3, 2, 3]                                 # entry 6, 517 x 301, is beyond the cubic filter's 32 x and within the area filter's 128 x
    table = sources.tables[channels](which)
    tabs = drawn(len(which), first=2)
    tones = tone_table(tabs)
    twelves = drawn_maps(len(which), first=2)
    twelves[0] = (GAIN + 1,) + twelves[0][1:]                        # a matrix entry beyond 2^20
    maps = map_table(twelves, reserved={4: (3, 1)})                  # a reserved word set
    other = {5: lambda s: 0}                                         # a zero address
    fmt = _formats((0, 0), channels)[1]
    for name, kw in (("two_tap", dict(filter=0)), ("area", dict(filter=1)), ("cubic", dict(filter=2)),
                     ("warp", dict(warps=_warp_table(na, [na.warp_fixed([[2, 0, 0], [0, 2, 0]])] * len(which), (1, 2, 3), False)))):
        beyond = {6} if name == "cubic" else set()
        # with maps: the two entries whose map is beyond the limits store nothing, beside the zero address and the reduction limit
        rc, mref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, maps=maps, **kw)
        assert rc == 0 and intact
        rc, slots, intact = launch(table, out_w, out_h, fmt, channels, maps=maps, tones=tones, other_addr=other, **kw)
        assert rc == 0 and intact, name
        for i in range(len(which)):
            if i in {0, 4, 5} | beyond:
                assert untouched(slots[i]), f"{name}: entry {i} was written"
            else:
                _assert_slot(slots[i], _pixels(mref[i], out_h, out_w, channels), tabs[i], fmt, out_h, out_w, channels, f"{name}: entry {i} beside the dead ones")
        # without maps: the zero address and the reduction limit alone
        rc, ref, intact = launch(table, out_w, out_h, _byte_format(channels), channels, **kw)
        assert rc == 0 and intact
        rc, slots, intact = launch(table, out_w, out_h, fmt, channels, tones=tones, other_addr=other, **kw)
        assert rc == 0 and intact, name
        for i in range(len(which)):
            if i in {5} | beyond:
                assert untouched(slots[i]), f"{name}: entry {i} was written"
            else:
                _assert_slot(slots[i], _pixels(ref[i], out_h, out_w, channels), tabs[i], fmt, out_h, out_w, channels, f"{name}: entry {i}, no maps")


def test_call_level_refusals(sources):
    import nhwcodec_amd as na
    out_w, out_h = 5, 7
    which = [1, 3]
    tabs = drawn(2, first=1)
    tones = tone_table(tabs)
    maps = map_table(drawn_maps(2, first=1))
    warps = _warp_table(na, [na.warp_fixed([[2, 0, 0], [0, 2, 0]])] * 2, (1, 2, 3), False)
    for channels in (3, 1):
        table = sources.tables[channels](which)
        fmt = _formats((0, 0), channels)[1]
        for kw in (dict(filter=0), dict(filter=2, flags=[1, 0]), dict(warps=warps)):
            for m in (None, maps):
                rc, slots, intact = launch(table, out_w, out_h, fmt, channels, maps=m, null_tones=True, **kw)     # a NULL table of tone tables
                assert rc == NHW_E_ARG and intact and all(untouched(s) for s in slots), kw
                assert b"bad argument" in na._library().nhw_last_error()
            for spoil in (dict(reserved=1), dict(dtype=4), dict(layout=2), dict(channels=3), dict(rows=2)):
                class Spoilt:
                    dtype, shape = fmt.dtype, fmt.shape

                    @staticmethod
                    def c_struct():
                        c = fmt.c_struct()
                        for k, v in spoil.items():
                            setattr(c, k, v)
                        return c
                rc, slots, intact = launch(table, out_w, out_h, Spoilt, channels, tones=tones, **kw)
                assert rc == NHW_E_ARG and intact and all(untouched(s) for s in slots), (kw, spoil)
            for o in ((0, 7), (5, 4097)):
                rc, slots, intact = launch(table, o[0], o[1], fmt, channels, tones=tones, **kw)
                assert rc == NHW_E_ARG and intact and all(untouched(s) for s in slots)
        rc, slots, intact = launch(table, out_w, out_h, fmt, channels, filter=3, tones=tones)
        assert rc == NHW_E_ARG and all(untouched(s) for s in slots)
        assert b"nhw_resample_toned_to_tensor_device" in na._library().nhw_last_error()


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


def _python_tones(tabs, channels):
    """the tables as the Python layer takes them: [3, 256] on R, G, B, or the one row of a grey call"""
    return [t[::-1].copy() for t in tabs] if channels == 3 else [t[0].copy() for t in tabs]


@pytest.mark.parametrize("filter", ("two_tap", "area", "cubic"))
@pytest.mark.parametrize("channels", (3, 1))
def test_decode_crops_with_tones(world, channels, filter):
    tabs = drawn(len(CROPS), first=3 + NUMBER[filter])
    flips = [i % 2 == 1 for i in range(len(CROPS))]
    call = world.dec.decode_crops_device if channels == 3 else world.dec.decode_crops_grey_device
    ref, scales = call(world.containers, CROPS, OUT, _byte_format(channels), flips=flips, filter=filter)
    assert sorted(set(scales)) == [1, 2, 4]                           # scale=None: mixed scales take part
    ref = ref.cpu().numpy()
    for fmt in _formats((0, 0), channels):
        got, again = call(world.containers, CROPS, OUT, fmt, flips=flips, filter=filter, tones=_python_tones(tabs, channels))
        assert again == scales and got.dtype == fmt.dtype and tuple(got.shape) == (len(CROPS),) + fmt.shape(*OUT)
        bits = tensor_bits(got)
        for i in range(len(CROPS)):
            px = ref[i] if channels == 3 else ref[i].reshape(OUT)
            assert np.array_equal(bits[i], _expect(px, tabs[i], fmt, channels)), (filter, fmt, i)
    # colours and tones combine: the mapped call's bytes through the table
    twelves = drawn_maps(len(CROPS), first=2 + NUMBER[filter])
    colours = [np.array(t, np.int64) for t in twelves] if channels == 3 else [(t[0] / 65536, t[9] / 65536) for t in twelves]
    mref, _ = call(world.containers, CROPS, OUT, _byte_format(channels), flips=flips, filter=filter, colours=colours)
    mref = mref.cpu().numpy()
    fmt = _formats((0, 0), channels)[1]
    got, _ = call(world.containers, CROPS, OUT, fmt, flips=flips, filter=filter, colours=colours, tones=_python_tones(tabs, channels))
    bits = tensor_bits(got)
    for i in range(len(CROPS)):
        px = mref[i] if channels == 3 else mref[i].reshape(OUT)
        assert np.array_equal(bits[i], _expect(px, tabs[i], fmt, channels)), (filter, "with colours", i)
    # scale=None is not the only way in: one scale for all
    one, _ = call(world.containers, [(c[0], c[1] // 2, c[2] // 2, c[3] // 2 + 1, c[4] // 2 + 1) for c in CROPS], OUT, _byte_format(channels), scale=2, filter=filter)
    got, sc = call(world.containers, [(c[0], c[1] // 2, c[2] // 2, c[3] // 2 + 1, c[4] // 2 + 1) for c in CROPS], OUT, fmt, scale=2, filter=filter,
                   tones=_python_tones(tabs, channels))
    assert sc == [2] * len(CROPS)
    one, bits = one.cpu().numpy(), tensor_bits(got)
    for i in range(len(CROPS)):
        px = one[i] if channels == 3 else one[i].reshape(OUT)
        assert np.array_equal(bits[i], _expect(px, tabs[i], fmt, channels)), (filter, "scale 2", i)


@pytest.mark.parametrize("channels", (3, 1))
def test_decode_warps_with_tones(world, channels):
    import nhwcodec_amd as na
    which = [c[0] for c in CROPS]
    mats = [na.crop_warp(x - 3, y - 3, w, h, OUT, angle=0.3 * i, flip=i % 2 == 0) for i, (_, x, y, w, h) in enumerate(CROPS)]    # the first ones reach outside their picture
    tabs = drawn(len(CROPS), first=6)
    call = world.dec.decode_warps_device if channels == 3 else world.dec.decode_warps_grey_device
    for border, fill in (("fill", (201, 17, 94)), ("replicate", (0, 0, 0))):
        fill = fill if channels == 3 else fill[0]
        ref, scales = call(world.containers, which, mats, OUT, _byte_format(channels), fill=fill, border=border)
        ref = ref.cpu().numpy()
        fmt = _formats((0, 0), channels)[1]
        got, again = call(world.containers, which, mats, OUT, fmt, fill=fill, border=border, tones=_python_tones(tabs, channels))
        assert again == scales and len(set(scales)) > 1
        bits = tensor_bits(got)
        for i in range(len(CROPS)):
            px = ref[i] if channels == 3 else ref[i].reshape(OUT)
            assert np.array_equal(bits[i], _expect(px, tabs[i], fmt, channels)), (border, i)


def _call_crops_toned(dec, containers, rects, scale, out_w, out_h, fmt, tones, addrs, filter=0):
    """nhw_dec_crops_toned_to_device by ctypes, no maps -> (rc, status)"""
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = (Rect * len(rects))(*[Rect(*r) for r in rects])
    status = np.full(len(rects), 99, np.int32)
    addr = np.array(addrs, np.uint64)
    c = fmt.c_struct()
    rc = dec.lib.nhw_dec_crops_toned_to_device(dec.h, blob.ctypes.data, off.ctypes.data, len(containers), ctypes.addressof(table), len(rects), scale, out_w, out_h,
                                               ctypes.byref(c), None, None, tones.ctypes.data if tones is not None else None, addr.ctypes.data, status.ctypes.data, filter)
    return rc, status


def test_the_decoder_entry_refuses_a_null_table(world):
    import torch
    fmt = tensor_format("float16", "CHW", "RGB", "reversed")
    out_h, out_w = 6, 8
    per, es = 3 * out_w * out_h, 2
    rects = [(BIG, 0, 0, 60, 50), (SMALL, 10, 10, 64, 64)]
    buf = torch.full((len(rects) * per * es,), CANARY, dtype=torch.uint8, device="cuda")
    addrs = [buf.data_ptr() + i * per * es for i in range(len(rects))]
    rc, status = _call_crops_toned(world.dec, world.containers, rects, 1, out_w, out_h, fmt, None, addrs)
    assert rc == NHW_E_ARG and (status == 99).all() and b"bad argument" in world.dec.lib.nhw_dec_last_error()
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    tabs = drawn(2, first=4)
    rc, status = _call_crops_toned(world.dec, world.containers, rects, 1, out_w, out_h, fmt, tone_table(tabs), addrs)
    torch.cuda.synchronize()
    assert rc == 0 and status.tolist() == [0, 0]
    ref, _ = world.dec.decode_crops_device(world.containers, rects, (out_h, out_w), _byte_format(3), scale=1)
    ref, host = ref.cpu().numpy(), buf.cpu().numpy()
    for i in range(2):
        _assert_slot(host[i * per * es:(i + 1) * per * es], ref[i], tabs[i], fmt, out_h, out_w, 3, f"rect {i}")


def test_one_handle_serves_plain_toned_and_mapped_calls_in_turn(world):
    fmt = tensor_format("float32", "HWC", "RGB", "file")
    tabs = drawn(len(CROPS), first=11)
    twelves = drawn_maps(len(CROPS), first=11)
    colours = [np.array(t, np.int64) for t in twelves]
    first, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic")
    first = tensor_bits(first).copy()
    mapped0, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic", colours=colours)
    mapped0 = tensor_bits(mapped0).copy()
    toned, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic", tones=_python_tones(tabs, 3))
    mapped, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic", colours=colours)
    last, _ = world.dec.decode_crops_device(world.containers, CROPS, OUT, fmt, filter="cubic")
    assert np.array_equal(first, tensor_bits(last)) and np.array_equal(mapped0, tensor_bits(mapped))
    assert not np.array_equal(first, tensor_bits(toned)) and not np.array_equal(mapped0, tensor_bits(toned))


def test_builders_and_a_device_table_through_the_python_layer(sources):
    """the host builders' rows are R, G, B and reach the kernel exchanged; a uint8 CUDA tensor [n, 768] goes in as it is"""
    import torch
    import nhwcodec_amd as na
    fmt = tensor_format("uint8", "HWC", "RGB", "file")
    pics = [sources.views3[2], sources.views3[3]]
    t = [na.tone_posterize((1, 4, 8)), na.tone_compose(na.tone_solarize((0, 128, 256)), na.tone_gamma(0.5))]
    ref = na.resize_to_tensor_device(pics, (9, 11), _byte_format(3), flips=[True, False], filter="area").cpu().numpy()
    got = na.resize_to_tensor_device(pics, (9, 11), fmt, flips=[True, False], filter="area", tones=t).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], expected_tensor(apply_tone(ref[i], t[i][::-1]), fmt)), i
    assert (got[0][..., 0] % 128 == 0).all() and (got[0][..., 1] % 16 == 0).all()      # R kept one bit, G four
    fixed = torch.from_numpy(np.stack([na.tone_fixed(x) for x in t])).cuda()
    again = na.resize_to_tensor_device(pics, (9, 11), fmt, flips=[True, False], filter="area", tones=fixed).cpu().numpy()
    assert np.array_equal(again, got)
    m = [na.colour_matrix(saturation=0), na.colour_matrix(brightness=1.3)]
    mref = na.warp_to_tensor_device(pics, [_rotation(517, 301, 11, 9, 12), _rotation(32, 24, 11, 9, 40)], (9, 11), _byte_format(3), fill=(1, 2, 3), colours=m).cpu().numpy()
    got = na.warp_to_tensor_device(pics, [_rotation(517, 301, 11, 9, 12), _rotation(32, 24, 11, 9, 40)], (9, 11), fmt, fill=(1, 2, 3), colours=m, tones=fixed).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], expected_tensor(apply_tone(mref[i], t[i][::-1]), fmt)), i
    grey = grey_format("float32", "CHW", "file")
    row = na.tone_solarize(100)[0]
    ref = na.warp_grey_to_tensor_device([sources.views1[2]], [_rotation(517, 301, 11, 9, 12)], (9, 11), _byte_format(1), fill=40).cpu().numpy()
    got = na.warp_grey_to_tensor_device([sources.views1[2]], [_rotation(517, 301, 11, 9, 12)], (9, 11), grey, fill=40, tones=[row])
    assert np.array_equal(tensor_bits(got)[0], expected_grey_tensor(row[ref[0].reshape(9, 11)], grey))
    ref = na.resize_grey_to_tensor_device([sources.views1[3]], (24, 32), _byte_format(1), filter="cubic").cpu().numpy()
    got = na.resize_grey_to_tensor_device([sources.views1[3]], (24, 32), grey, tones=[row], filter="cubic")
    assert np.array_equal(tensor_bits(got)[0], expected_grey_tensor(row[ref[0].reshape(24, 32)], grey))
    for bad in (fixed[:1], fixed.cpu(), fixed.to(torch.int32), fixed.reshape(2, 3, 256)):
        with pytest.raises(na.NhwError):
            na.resize_to_tensor_device(pics, (9, 11), fmt, tones=bad)
