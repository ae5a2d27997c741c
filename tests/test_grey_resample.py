"""The one-channel resamplers and warp: k_resize_to_tensor, k_area_to_tensor, k_cubic_to_tensor and k_warp_to_tensor at
one byte a pixel, behind nhw_resample_grey_to_tensor_device and nhw_warp_grey_to_tensor_device, on random one-channel pictures.  The expected
bytes are the colour kernel's on the picture replicated into three channels (grey_picture_cases), the elements the exact value rule's; every
batch lies between guards, and an entry that must store nothing keeps its canary."""
import math

import numpy as np
import pytest

from tests.grey_cases import GREY_FORMATS, grey_format
from tests.grey_picture_cases import (NHW_E_ARG, assert_tensors, bits_of, grey_views, launch_grey, picture_table, reference_resize, reference_warp,
                                      slot_bits)
from tests.support import CANARY

pytestmark = pytest.mark.gpu
# W, H, pitch extra, misalignment
SOURCES = [(1, 1, 0, 0), (1, 700, 0, 1), (700, 1, 0, 3), (37, 23, 0, 2), (517, 301, 11, 5)]
OUTPUTS = [(1, 1), (5, 7), (224, 224), (300, 3)]                     # out_w, out_h; 300 is wider than a pass's 256 lanes
ALL_FORMATS_AT = (5, 7)
LIMITS = {"two_tap": 0, "area": 128, "cubic": 32}
NUMBER = {"two_tap": 0, "area": 1, "cubic": 2}
EXTRA = {"area": ((1280, 256, 3, 1), (10, 2)), "cubic": ((2048, 96, 5, 2), (64, 3))}   # a reduction of 128; of 32 on both axes: several column chunks and row passes


@pytest.fixture(scope="module")
def sources():
    return grey_views(SOURCES, 231)


def _formats(out):
    if out == ALL_FORMATS_AT:
        return [grey_format(*f) for f in GREY_FORMATS]                # four dtypes x two layouts (the same memory) x both row orders
    return [grey_format("uint8", "HWC", "file"), grey_format("float16", "CHW", "reversed")]


def _within(filter, w, h, out_w, out_h):
    return not LIMITS[filter] or (w <= LIMITS[filter] * out_w and h <= LIMITS[filter] * out_h)


def _untouched(slot):
    return bool((slot == CANARY).all())


@pytest.mark.parametrize("out", OUTPUTS, ids=lambda o: f"{o[0]}x{o[1]}")
@pytest.mark.parametrize("filter", ("two_tap", "area", "cubic"))
def test_grey_resamplers_equal_the_colour_kernels(sources, filter, out):
    out_w, out_h = out
    _, views, own = sources
    which = [k for k in range(len(SOURCES)) for _ in (0, 1)]         # every source plain and mirrored
    flags = [j % 2 for j in range(len(which))]
    ok = [_within(filter, SOURCES[k][0], SOURCES[k][1], out_w, out_h) for k in which]
    assert any(ok) and (filter == "two_tap" or out != (1, 1) or not all(ok))
    want = reference_resize([own[k] for k, good in zip(which, ok) if good], (out_h, out_w), [f for f, good in zip(flags, ok) if good], filter)
    table = picture_table([views[k] for k in which])
    for fmt in _formats(out):
        rc, slots, intact = launch_grey(table, out_w, out_h, fmt, filter=NUMBER[filter], flags=flags)
        assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
        good = [slot_bits(s, fmt, out_h, out_w) for s, g in zip(slots, ok) if g]
        assert_tensors(good, want, fmt, f"{filter} to {out_w} x {out_h} under {fmt}")
        assert all(_untouched(s) for s, g in zip(slots, ok) if not g), f"{filter}: an entry beyond the limit was written"
    fmt = _formats(out)[0]                                           # no flag table: nothing is mirrored, and a mirrored entry equals its plain twin in front of it
    rc, slots, intact = launch_grey(table, out_w, out_h, fmt, filter=NUMBER[filter], flags=None)
    assert rc == 0 and intact
    rank = np.cumsum(ok) - 1
    twins = [want[rank[i - i % 2]] for i, g in enumerate(ok) if g]
    assert_tensors([slot_bits(s, fmt, out_h, out_w) for s, g in zip(slots, ok) if g], twins, fmt, f"{filter} to {out_w} x {out_h} without flags")


@pytest.mark.parametrize("filter", ("area", "cubic"))
def test_grey_resamplers_at_their_reduction_limit(filter):
    (w, h, extra, mis), (out_w, out_h) = EXTRA[filter]
    assert w == LIMITS[filter] * out_w and h >= out_h
    _, views, own = grey_views([(w, h, extra, mis)] * 2, 232)
    want = reference_resize(own, (out_h, out_w), [0, 1], filter)
    for fmt in (grey_format("uint8", "HWC", "file"), grey_format("bfloat16", "CHW", "reversed")):
        rc, slots, intact = launch_grey(picture_table(views), out_w, out_h, fmt, filter=NUMBER[filter], flags=[0, 1])
        assert rc == 0 and intact
        assert_tensors([slot_bits(s, fmt, out_h, out_w) for s in slots], want, fmt, f"{filter} {w} x {h} to {out_w} x {out_h}")


def _rotation(w, h, out_w, out_h, degrees):
    """output pixel centres to source coordinates: a turn about both centres, the output's grid a fifth larger than the picture, so that taps
    fall outside it; a step stays below the warp's limit of 64"""
    s = min(1.2 * max(w / out_w, h / out_h), 60.0)
    c, n = s * math.cos(math.radians(degrees)), s * math.sin(math.radians(degrees))
    return [[c, -n, w / 2 - (c * out_w / 2 - n * out_h / 2)], [n, c, h / 2 - (n * out_w / 2 + c * out_h / 2)]]


def _warp_table(na, fixed, fill, replicate):
    t = np.zeros(len(fixed), na.WARP_DTYPE)
    for i, (a, b, c, d, e, f) in enumerate(fixed):
        t[i] = (c, f, a, b, d, e, (fill, 0xEE, 0x77), int(replicate), 0)     # fill[1] and fill[2] are not read
    return t


@pytest.mark.parametrize("out", OUTPUTS, ids=lambda o: f"{o[0]}x{o[1]}")
def test_grey_warp_equals_the_colour_kernel(sources, out):
    import nhwcodec_amd as na
    out_w, out_h = out
    _, views, own = sources
    which = [k for k in range(len(SOURCES)) for _ in (0, 10, 30)]
    mats = [_rotation(SOURCES[k][0], SOURCES[k][1], out_w, out_h, deg) for k in range(len(SOURCES)) for deg in (0, 10, 30)]
    fixed = [na.warp_fixed(m) for m in mats]
    steep = [abs(f[3]) > 16384 for f in fixed]                       # d: beyond it the kernel walks by 8 x 8 blocks, else by rows
    assert any(steep) and not all(steep)
    table = picture_table([views[k] for k in which])
    for border, fill in (("fill", 201), ("replicate", 9)):
        want = reference_warp([own[k] for k in which], mats, (out_h, out_w), fill, border)
        if border == "fill" and out_w * out_h > 1:
            assert (want == fill).any(), "no tap fell outside a picture"
        for fmt in _formats(out):
            rc, slots, intact = launch_grey(table, out_w, out_h, fmt, warps=_warp_table(na, fixed, fill, border == "replicate"))
            assert rc == 0 and intact, f"{fmt}: refused, or a byte outside the batch was written"
            assert_tensors([slot_bits(s, fmt, out_h, out_w) for s in slots], want, fmt, f"warp to {out_w} x {out_h}, {border}, under {fmt}")


def test_entries_that_store_nothing(sources):
    import nhwcodec_amd as na
    _, views, own = sources
    out_w, out_h = 5, 7
    good = picture_table([views[3]] * 7)
    table = good.copy()
    table[2]["width"] = 0
    table[3]["height"] = 0
    table[4]["width"] = 65536
    other = {0: lambda s: 0, 1: lambda s: s + 1}                      # a zero address; one that is no multiple of the element size
    dead = (0, 1, 2, 3, 4)
    fmt = grey_format("float16", "CHW", "file")
    want = reference_resize([own[3]], (out_h, out_w), None, "two_tap")
    for filter in (0, 1, 2):
        rc, slots, intact = launch_grey(table, out_w, out_h, fmt, filter=filter, other_addr=other)
        assert rc == 0 and intact and all(_untouched(slots[i]) for i in dead) and not _untouched(slots[5]) and not _untouched(slots[6]), filter
    assert_tensors([slot_bits(slots[5], fmt, out_h, out_w)], reference_resize([own[3]], (out_h, out_w), None, "cubic"), fmt, "the entry behind the dead ones")
    identity = na.warp_fixed([[1, 0, 0], [0, 1, 0]])
    fixed = [identity] * 7
    fixed[5] = ((1 << 22) + 1,) + tuple(identity[1:])                 # a beyond the limit of 64 pixels a step
    warps = _warp_table(na, fixed, 0, False)
    warps[6]["c"] = (1 << 40) + 1                                    # c beyond 2^40
    rc, slots, intact = launch_grey(good, out_w, out_h, fmt, warps=warps, other_addr=other)
    assert rc == 0 and intact and all(_untouched(slots[i]) for i in (0, 1, 5, 6)) and not any(_untouched(slots[i]) for i in (2, 3, 4))
    assert want.shape == (1, out_h, out_w)
    # what the host refuses, before anything is launched: a colour format, a side outside 1 .. 4096, a filter that does not exist
    for kw, o in ((dict(fmt=na.TensorFormat("float16", "CHW", "RGB")), (5, 7)), (dict(fmt=fmt), (0, 7)), (dict(fmt=fmt), (5, 4097))):
        for extra in (dict(filter=0), dict(warps=warps)):
            rc, slots, intact = launch_grey(good, o[0], o[1], **kw, **extra)
            assert rc == NHW_E_ARG and intact and all(_untouched(s) for s in slots)
    rc, slots, intact = launch_grey(good, 5, 7, fmt, filter=3)
    assert rc == NHW_E_ARG and all(_untouched(s) for s in slots)


def test_python_wrappers(sources):
    import nhwcodec_amd as na
    _, views, own = sources
    fmt = grey_format("float32", "HWC", "reversed")
    for filter in ("two_tap", "area", "cubic"):
        got = na.resize_grey_to_tensor_device([views[4], views[3]], (12, 20), fmt, flips=[True, False], filter=filter)
        assert got.dtype == fmt.dtype and tuple(got.shape) == (2, 12, 20, 1)
        assert_tensors(bits_of(got), reference_resize([own[4], own[3]], (12, 20), [1, 0], filter), fmt, f"resize_grey_to_tensor_device, {filter}")
    mats = [_rotation(517, 301, 11, 9, 20), _rotation(37, 23, 11, 9, -5)]
    for border in ("fill", "replicate"):
        got = na.warp_grey_to_tensor_device([views[4], views[3]], mats, (9, 11), grey_format("uint8", "CHW", "file"), fill=77, border=border)
        assert tuple(got.shape) == (2, 1, 9, 11)
        assert_tensors(bits_of(got), reference_warp([own[4], own[3]], mats, (9, 11), 77, border), grey_format("uint8", "CHW", "file"), f"warp_grey_to_tensor_device, {border}")
    with pytest.raises(na.NhwError):
        na.resize_grey_to_tensor_device([views[4].t()], (9, 11), fmt)     # strides (1, pitch)
