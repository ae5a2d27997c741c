"""Per-sample flip, colour map and tone table in the full-file decode on the GPU: nhw_dec_batch_device_tensor_ops,
nhw_dec_batch_device_grey_ops (the store policies NhwStoreTensorOps and NhwStoreGreyOps of k_dec_final and k_dec_scaled<2> / <4>) and the
keywords flips, colours, tones of Decoder.decode_tensor_device / decode_grey_device.

The expected values are tests/decode_ops_cases.py's: the oracle's bytes of a file, mirrored with numpy, through colour_cases' int64 map and
tone_cases' gather, under tensor_cases' exact value rule.  Bit patterns are compared as integers.

Batches (those of test_tensor_decode.py, the smallest that reach every path): THREE = q20_0 (eight pixels a thread; grey: the identity grey
table), q10_0 (four pixels a thread; grey: a table below quality 20) and a file truncated to 40 bytes (a refused slot); TWO = q23_0, q01_0.
Every call writes into a sentinel-filled buffer with tensor_cases.TAIL bytes behind it: a refused slot and the tail must stay as they were."""
import numpy as np
import pytest

from tests import colour_cases, tone_cases
from tests.decode_ops_cases import (FLAGS, FORMATS8, GREY_FORMATS, SCALES, assert_ops, batch, decode_ops, decode_ops_c, expected_ops_bytes, maps_for,
                                    python_colours, python_tones, tables_for, untouched)
from tests.grey_cases import decode_grey, grey_format
from tests.support import device_arena
from tests.tensor_cases import decode_tensor, expected_bytes, tensor_bits, tensor_format

pytestmark = pytest.mark.gpu
WHICH = ("flip", "map", "tone", "all")


@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=16)
    yield d
    d.close()


def _ops(which, n, flags, first):
    """(flags, twelves, tables) of a case: what `which` leaves out is None"""
    return (list(flags) if which in ("flip", "all") else None, maps_for(n, first) if which in ("map", "all") else None,
            tables_for(n, first) if which in ("tone", "all") else None)


def _grey_fmt(g):
    return None if g is None else grey_format(*g)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("flags", FLAGS, ids=["101", "010"])
@pytest.mark.parametrize("which", WHICH)
def test_colour_each_op_and_all_under_eight_formats(dec, oracle, which, flags, scale):
    """both thread shapes and a refused slot, each op alone and all three, a different map and table a file, under the eight dtype x layout pairs"""
    files, status, quality = batch("three")
    for k, four in enumerate(FORMATS8):
        fmt = tensor_format(*four)
        f, m, t = _ops(which, 3, flags, 3 * (k % 2))
        bits, st, qq = decode_ops(dec, files, fmt, scale, f, None if m is None else python_colours(m), None if t is None else python_tones(t))
        assert st.tolist() == status and qq.tolist()[:2] == quality
        assert_ops(oracle, bits, files, status, fmt, scale, f, m, t, what=f"{which} {flags}")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("flags", FLAGS, ids=["101", "010"])
@pytest.mark.parametrize("which", WHICH)
def test_grey_each_op_and_all(dec, oracle, which, flags, scale):
    """the same for the grey decode: a quality from 20 up (file 0) and one below (file 1), bytes and the four dtypes"""
    files, status, quality = batch("three")
    for k, g in enumerate(GREY_FORMATS):
        fmt = _grey_fmt(g)
        f, m, t = _ops(which, 3, flags, 3 * (k % 2))
        pairs = None if m is None else [(x[0] / 65536.0, x[9] / 65536.0) for x in m]      # exact: |m| <= 2^20, |o| <= 2^28 in 1/65536
        bits, st, qq = decode_ops(dec, files, fmt, scale, f, pairs, None if t is None else python_tones(t, grey=True), grey=True)
        assert st.tolist() == status and qq.tolist()[:2] == quality
        assert_ops(oracle, bits, files, status, fmt, scale, f, m, t, grey=True, what=f"grey {which} {flags}")


@pytest.mark.parametrize("scale", SCALES)
def test_the_other_batch_all_ops(dec, oracle, scale):
    """q23 (the level-1 corrections) and q1 (the low colour matrix), colour and grey"""
    files, status, _ = batch("two")
    m, t = maps_for(2, 8), tables_for(2, 2)
    for four in (FORMATS8[3], FORMATS8[6]):
        fmt = tensor_format(*four)
        bits, st, _ = decode_ops(dec, files, fmt, scale, [1, 1], python_colours(m), python_tones(t))
        assert st.tolist() == status
        assert_ops(oracle, bits, files, status, fmt, scale, [1, 1], m, t, what="two")
    fmt = _grey_fmt(GREY_FORMATS[2])
    bits, st, _ = decode_ops(dec, files, fmt, scale, [1, 0], None, python_tones(t, grey=True), grey=True)
    assert_ops(oracle, bits, files, status, fmt, scale, [1, 0], None, t, grey=True, what="two grey")


@pytest.mark.parametrize("scale", SCALES)
def test_identity_ops_are_the_plain_decode(dec, scale):
    """no flip, the identity map and tone_identity() equal the plain calls bit for bit; so do the new C entries with all three tables NULL"""
    import nhwcodec_amd as na
    files, status, _ = batch("three")
    ident = [na.tone_identity()] * 3
    for four in (FORMATS8[0], FORMATS8[3], FORMATS8[6]):
        fmt = tensor_format(*four)
        plain, st0, q0 = decode_tensor(dec, files, fmt, scale)
        same, st1, q1 = decode_ops(dec, files, fmt, scale, [0, 0, 0], np.eye(3, 4), ident)
        assert st0.tolist() == st1.tolist() == status and q0.tolist() == q1.tolist() and np.array_equal(plain, same), fmt
        rc, null, st2, q2 = decode_ops_c(dec, files, fmt, scale)
        assert rc == 0 and st2.tolist() == status and q2.tolist() == q0.tolist() and np.array_equal(null.reshape(plain.shape), plain), fmt
    for g in (GREY_FORMATS[0], GREY_FORMATS[2], GREY_FORMATS[3]):
        fmt = _grey_fmt(g)
        plain, st0, q0 = decode_grey(dec, files, scale, fmt)
        same, st1, q1 = decode_ops(dec, files, fmt, scale, [False] * 3, (1.0, 0.0), [na.tone_identity()[0]] * 3, grey=True)
        assert st0.tolist() == st1.tolist() == status and q0.tolist() == q1.tolist() and np.array_equal(plain, same), fmt
        rc, null, st2, q2 = decode_ops_c(dec, files, fmt, scale, grey=True)
        assert rc == 0 and st2.tolist() == status and q2.tolist() == q0.tolist() and np.array_equal(null.reshape(plain.shape), plain), fmt


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("grey", [False, True], ids=["colour", "grey"])
def test_a_map_beyond_the_limits_stores_nothing(dec, oracle, grey, scale):
    """file 1's map beyond a limit, then with a non-zero reserved word, through the C entry: its slot keeps the sentinel, the others are what they
    are without it, and status and quality are the plain decode's"""
    files, status, quality = batch("three")
    fmt = _grey_fmt(GREY_FORMATS[2]) if grey else tensor_format(*FORMATS8[3])
    good = maps_for(3, 0)
    over = list(good[1])
    over[4] = colour_cases.GAIN + 1
    flags, tabs = [1, 1, 0], tables_for(3, 0)
    for twelves, reserved in (([good[0], tuple(over), good[2]], None), (good, {1: (2, 1)})):
        table = colour_cases.map_table(twelves, reserved)
        rc, bits, st, qq = decode_ops_c(dec, files, fmt, scale, flags, table, tone_cases.tone_table(tabs), grey=grey)
        assert rc == 0 and st.tolist() == status and qq.tolist()[:2] == quality
        assert untouched(bits[1]) and untouched(bits[2])
        assert_ops(oracle, bits[:1], files[:1], status[:1], fmt, scale, flags, twelves, tabs, grey=grey, what="beside a refused map")
    rc, bits, st, _ = decode_ops_c(dec, files, fmt, scale, flags, colour_cases.map_table(good), tone_cases.tone_table(tabs), grey=grey)
    assert rc == 0 and st.tolist() == status and not untouched(bits[1]) and untouched(bits[2])      # ... and the same call with good maps stores slot 1
    assert_ops(oracle, bits, files, status, fmt, scale, flags, good, tabs, grey=grey, what="good maps")


@pytest.mark.parametrize("scale", SCALES)
def test_the_byte_format_with_ops_gives_the_opd_bytes(dec, oracle, scale):
    """U8 / HWC / BGR / file rows with any table present takes the new policy, not the byte path"""
    import nhwcodec_amd as na
    files, status, _ = batch("three")
    fmt = na.TensorFormat("uint8", "HWC", "BGR", "file")
    plain, _, _ = decode_tensor(dec, files, fmt, scale)
    for flags, tw, tb in (([1, 1, 1], None, None), (None, maps_for(3, 1), None), (None, None, tables_for(3, 1))):
        rc, bits, st, _ = decode_ops_c(dec, files, fmt, scale, flags, None if tw is None else colour_cases.map_table(tw), None if tb is None else tone_cases.tone_table(tb))
        assert rc == 0 and st.tolist() == status
        for i in range(2):
            want = expected_ops_bytes(oracle, files[i], scale, 0 if flags is None else flags[i], None if tw is None else tw[i], None if tb is None else tb[i])
            assert np.array_equal(bits[i], want) and not np.array_equal(bits[i], plain[i])
        assert untouched(bits[2])


@pytest.mark.parametrize("mode", [1, 2])
def test_under_forced_slice_orders(dec, oracle, mode):
    """the bands of the last kernels one a launch, ascending and descending: the same tensors, colour and grey"""
    files, status, _ = batch("three")
    m, t, flags = maps_for(3, 3), tables_for(3, 2), [1, 0, 1]
    assert dec.lib.nhw_dec_debug_slice_order(dec.h, mode) == 0
    try:
        fmt = tensor_format(*FORMATS8[5])
        bits, st, _ = decode_ops(dec, files, fmt, 1, flags, python_colours(m), python_tones(t))
        gfmt = _grey_fmt(GREY_FORMATS[3])
        gbits = [decode_ops(dec, files, gfmt, s, flags, None, python_tones(t, grey=True), grey=True) for s in (1, 2)]
    finally:
        assert dec.lib.nhw_dec_debug_slice_order(dec.h, 0) == 0
    assert st.tolist() == status
    assert_ops(oracle, bits, files, status, fmt, 1, flags, m, t, what=f"slice order {mode}")
    for s, (gb, gst, _) in zip((1, 2), gbits):
        assert gst.tolist() == status
        assert_ops(oracle, gb, files, status, gfmt, s, flags, None, t, grey=True, what=f"grey slice order {mode}")


def test_equals_the_existing_route_at_scale_1(dec):
    """decode_device, then resize_to_tensor_device at the picture's own size with the same flips, colours and tones: the same bits"""
    import torch
    import nhwcodec_amd as na
    files, _, _ = batch("two")
    m, t, flags = python_colours(maps_for(2, 3)), python_tones(tables_for(2, 1)), [True, False]
    px, st, _ = dec.decode_device(*device_arena(files))
    torch.cuda.synchronize()
    assert not bool(st.any())
    for four in (FORMATS8[2], FORMATS8[5], FORMATS8[7]):
        fmt = tensor_format(*four)
        want = na.resize_to_tensor_device([px[0], px[1]], (512, 512), fmt, flips=flags, colours=m, tones=t)
        got, st, _ = dec.decode_tensor_device(*device_arena(files), fmt, flips=flags, colours=m, tones=t)
        torch.cuda.synchronize()
        assert not bool(st.any()) and np.array_equal(tensor_bits(got), tensor_bits(want)), fmt


def test_a_tone_table_made_on_the_device(dec, oracle):
    """hist_device + tone_from_hist_device (equalize) on the plain decode's bytes, fed as tones=: expected from tone_cases.equalize_row on numpy
    histograms of the oracle's bytes"""
    import torch
    import nhwcodec_amd as na
    files, status, _ = batch("two")
    px, st, _ = dec.decode_device(*device_arena(files))
    tabs = na.tone_from_hist_device(na.hist_device([px[0], px[1]]), ["equalize"] * 2)
    fmt = tensor_format(*FORMATS8[3])
    bits, st, _ = decode_ops(dec, files, fmt, 1, [0, 1], None, tabs)
    del tabs, px
    assert st.tolist() == status
    want_tabs = []
    for f in files:
        b = expected_bytes(oracle, f, 1)
        want_tabs.append(np.stack([tone_cases.equalize_row(np.bincount(b[..., c].reshape(-1), minlength=256)) for c in range(3)]))
    assert_ops(oracle, bits, files, status, fmt, 1, [0, 1], None, want_tabs, what="equalize")
