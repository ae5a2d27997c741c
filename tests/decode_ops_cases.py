"""What a full-file decode with per-sample operations must produce, shared by test_decode_ops_rule.py and
test_decode_ops.py.  Nothing expected here comes from the code under test.  The bytes of a file are tensor_cases.expected_bytes (the oracle
decoder's picture at scale 1, section 14's at 2 and 4) or grey_cases.expected_grey; the mirror is numpy's [:, ::-1]; the map is
colour_cases.apply_map / apply_grey in int64; the table is tone_cases.apply_tone / apply_tone_grey, a gather; an element is
tensor_cases.expected_tensor's or grey_cases.expected_grey_tensor's exact value rule.  Bit patterns are compared as integers."""
import ctypes

import numpy as np

from tests import colour_cases, grey_cases, tensor_cases, tone_cases
from tests.support import device_arena, golden
from tests.tensor_cases import SENTINEL, TAIL

NHW_E_FORMAT = -6
SYMBOLS = ("nhw_dec_batch_device_tensor_ops", "nhw_dec_batch_device_grey_ops")
SCALES = (1, 2, 4)
# the eight dtype x layout pairs, channel order and row direction alternating: every enum value occurs, and the first is the byte format
FORMATS8 = [("uint8", "HWC", "BGR", "file"), ("uint8", "CHW", "RGB", "reversed"), ("float16", "HWC", "RGB", "file"), ("float16", "CHW", "BGR", "reversed"),
            ("bfloat16", "HWC", "BGR", "reversed"), ("bfloat16", "CHW", "RGB", "file"), ("float32", "HWC", "RGB", "reversed"), ("float32", "CHW", "BGR", "file")]
# the grey formats: None (bytes in file order) and the four dtypes, layout and rows alternating
GREY_FORMATS = [None, ("uint8", "CHW", "reversed"), ("float16", "HWC", "file"), ("bfloat16", "CHW", "reversed"), ("float32", "HWC", "file")]
FLAGS = ((1, 0, 1), (0, 1, 0))                   # file 0 of THREE has eight pixels a thread, file 1 four: both shapes are mirrored


def batch(name):
    """the batches of test_tensor_decode.py -> (files, expected statuses, qualities of the good files)"""
    if name == "three":
        return [golden("q20_0.nhw"), golden("q10_0.nhw"), golden("q20_0.nhw")[:40]], [0, 0, NHW_E_FORMAT], [20, 10]
    assert name == "two"
    return [golden("q23_0.nhw"), golden("q01_0.nhw")], [0, 0], [23, 1]


def maps_for(n, first=0):
    """n maps of colour_cases.MAPS as twelve integers each, a different one a file; `first` chooses where the walk starts.  Walks of 3 from 8, 9
    and 13 meet the clamping corners"""
    return colour_cases.drawn(n, first)


def tables_for(n, first=0):
    """n tables of tone_cases, uint8 [3, 256] in the struct's order B, G, R, a different one a file"""
    return tone_cases.drawn(n, first)


def python_colours(twelves):
    """the maps as the Python face takes them: integer arrays [12]"""
    return [np.array(m, np.int64) for m in twelves]


def python_tones(tables, grey=False):
    """the tables as the Python face takes them: [3, 256] on R, G, B; grey: [256], the struct's row 0"""
    return [np.asarray(t)[0] if grey else np.asarray(t)[::-1] for t in tables]


_OPS = {}


def expected_ops_bytes(oracle, nhw, scale, flag=0, twelve=None, table=None, grey=False):
    """the rule's steps 1 to 3 on a file's plain bytes: uint8 [S, S, 3] (grey: [S, S]), read-only, computed once"""
    key = (nhw, scale, flag & 1, twelve, None if table is None else np.asarray(table).tobytes(), grey)
    if key not in _OPS:
        px = grey_cases.expected_grey(oracle, nhw, scale) if grey else tensor_cases.expected_bytes(oracle, nhw, scale)
        if flag & 1:
            px = px[:, ::-1]
        if twelve is not None:
            px = colour_cases.apply_grey(px, twelve) if grey else colour_cases.apply_map(px, twelve)
        if table is not None:
            px = tone_cases.apply_tone_grey(px, np.asarray(table)) if grey else tone_cases.apply_tone(px, np.asarray(table))
        px = np.ascontiguousarray(px)
        px.setflags(write=False)
        _OPS[key] = px
    return _OPS[key]


def expected_ops(oracle, nhw, scale, fmt, flag=0, twelve=None, table=None, grey=False):
    """... and step 4: the tensor's bit patterns in fmt's own shape (grey with fmt None: the bytes)"""
    px = expected_ops_bytes(oracle, nhw, scale, flag, twelve, table, grey)
    if grey:
        return px if fmt is None else grey_cases.expected_grey_tensor(px, fmt)
    return tensor_cases.expected_tensor(px, fmt)


def decode_ops(dec, files, fmt, scale, flips=None, colours=None, tones=None, grey=False):
    """one decode_tensor_device / decode_grey_device call with the keywords into a sentinel-filled buffer -> (the output's bit patterns, status,
    quality) on the host; what lies behind the n slots is checked"""
    import torch
    n, s = len(files), 512 // scale
    dtype = torch.uint8 if fmt is None else fmt.dtype
    room = n * (1 if grey else 3) * s * s * dtype.itemsize
    buf = torch.full((room + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[:room].view(dtype)
    if grey:
        t, st, qq = dec.decode_grey_device(*device_arena(files), scale=scale, fmt=fmt, out=out, flips=flips, colours=colours, tones=tones)
    else:
        t, st, qq = dec.decode_tensor_device(*device_arena(files), fmt, scale=scale, out=out, flips=flips, colours=colours, tones=tones)
    torch.cuda.synchronize()
    assert t.dtype == dtype and t.data_ptr() == buf.data_ptr()
    assert bool((buf[room:] == SENTINEL).all()), "elements behind the n slots were written"
    return tensor_cases.tensor_bits(t), st.cpu().numpy(), qq.cpu().numpy()


def decode_ops_c(dec, files, fmt, scale, flags=None, maps=None, tones=None, grey=False, plain=False):
    """the C entries themselves: nhw_dec_batch_device_tensor_ops / _grey_ops (plain: the entries without tables) with flags (n bytes), maps (a
    colour_cases.COLOUR table) and tones (uint8 [n, 768]), each None for a null pointer -> (rc, the slots as bit patterns [n, ...], status,
    quality).  Every device table stays referenced until the synchronise."""
    import torch
    n, s = len(files), 512 // scale
    dtype = torch.uint8 if fmt is None else fmt.dtype
    per = (1 if grey else 3) * s * s
    room = n * per * dtype.itemsize
    buf = torch.full((room + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    qq = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    arena, offs, lens = device_arena(files)
    d_f = torch.from_numpy(np.asarray(flags, np.uint8)).cuda() if flags is not None else None
    d_m = torch.from_numpy(np.ascontiguousarray(maps).view(np.int64).copy()).cuda() if maps is not None else None
    d_t = torch.from_numpy(np.ascontiguousarray(tones)).cuda() if tones is not None else None
    c = fmt.c_struct() if fmt is not None else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    head = (dec.h, arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, scale, ctypes.byref(c) if c is not None else None)
    tail = (buf.data_ptr(), st.data_ptr(), qq.data_ptr(), None)
    if plain:
        assert flags is None and maps is None and tones is None
        rc = (dec.lib.nhw_dec_batch_device_grey if grey else dec.lib.nhw_dec_batch_device_tensor)(*head, *tail)
    else:
        rc = (dec.lib.nhw_dec_batch_device_grey_ops if grey else dec.lib.nhw_dec_batch_device_tensor_ops)(*head, ptr(d_f), ptr(d_m), ptr(d_t), *tail)
    torch.cuda.synchronize()
    del d_f, d_m, d_t
    host = buf.cpu().numpy()
    assert (host[room:] == SENTINEL).all(), "bytes behind the n slots were written"
    bits = host[:room].view({1: np.uint8, 2: np.uint16, 4: np.uint32}[dtype.itemsize])
    shape = ((s, s) if fmt is None else fmt.shape(s, s))
    return rc, bits.reshape((n,) + tuple(shape)), st.cpu().numpy(), qq.cpu().numpy()


def untouched(slot):
    return bool((slot.view(np.uint8) == SENTINEL).all())


def assert_ops(oracle, got, files, status, fmt, scale, flags=None, twelves=None, tables=None, grey=False, what=""):
    """every good file's slot is the rule's tensor under its own flag, map and table; every refused file's slot is still the sentinel"""
    for i, f in enumerate(files):
        if status[i]:
            assert untouched(got[i]), f"{what}: refused file {i}: its slot was written"
            continue
        want = expected_ops(oracle, f, scale, fmt, 0 if flags is None else int(flags[i]), None if twelves is None else twelves[i],
                            None if tables is None else tables[i], grey)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape, (got[i].dtype, got[i].shape, want.dtype, want.shape)
        bad = got[i] != want
        assert not bad.any(), f"{what} {fmt} scale {scale} file {i}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"
