"""The table behind the decoder's stage checks, shared by tests/test_decode_stages.py and tests/test_decode_values.py: nhw_dec_debug_stop_after ends a
batch behind one stage, nhw_dec_debug_read copies a workspace buffer out, and the oracle's decode_probe gives the same buffer at the same point of
decode_image.  STAGES is the table stop -> buffer -> probe id, every row bit for bit.  dec_batch is the whole decode by the C call, for
tests/test_decode_surgery.py and tests/test_decode_values.py."""
import numpy as np

from tests.support import CANARY

D = dict(MARKS=7, A=8, CA=10, CU=12)                                  # nhw_dec_debug_read's buffer indices
PROBES = (3, 4, 5, 50, 51, 6, 7, 30, 31, 40, 41, 42, 43, 44, 45, 46, 47)


def _rd(dec, what, img, nbytes, dtype):
    buf = np.empty(nbytes, np.uint8)
    assert dec.lib.nhw_dec_debug_read(dec.h, D[what], img, buf.ctypes.data, nbytes) == 0
    return buf.view(dtype)


def _luma(dec, img):
    return _rd(dec, "A", img, 8 * 65536 + 8192, np.int16)[2048:2048 + 262144].reshape(512, 512)


def _chroma(dec, img, comp):
    o = 1024 + comp * (65536 + 2048)
    return _rd(dec, "CA", img, 2 * (2 * 65536 + 4096), np.int16)[o:o + 65536].reshape(256, 256)


def _sharp(dec, img, comp):
    return _rd(dec, "CU", img, 131072, np.uint8)[65536 * comp:65536 * (comp + 1)].reshape(256, 256)


# stop -> [(what, GPU side (dec, file index, probe), oracle side (probe))]; probe(id) is the oracle's buffer as int16
STAGES = {
    # (the luma plane does not exist before the expansion: the walk leaves a list of values that k_dec_expand turns into rows)
    3: [("A after the expansion", lambda d, i, pr: _luma(d, i), lambda pr: pr(3).reshape(512, 512)),
        ("U after the expansion", lambda d, i, pr: _chroma(d, i, 0), lambda pr: pr(30).reshape(256, 256)),
        ("V after the expansion", lambda d, i, pr: _chroma(d, i, 1), lambda pr: pr(31).reshape(256, 256))],
    4: [("A after the shrink", lambda d, i, pr: _luma(d, i), lambda pr: pr(4).reshape(512, 512))],
    5: [("level-1 LL after the synthesis", lambda d, i, pr: _luma(d, i)[:256, :256], lambda pr: pr(5).reshape(512, 512)[:256, :256])],
    6: [("level-1 LL after the residuals", lambda d, i, pr: _luma(d, i)[:256, :256], lambda pr: pr(6).reshape(512, 512)[:256, :256])],
    7: [("marks", lambda d, i, pr: _rd(d, "MARKS", i, 2 * 65536, np.uint16)[:len(pr(7))], lambda pr: pr(7).view(np.uint16))],
    8: [("U after level 2", lambda d, i, pr: _chroma(d, i, 0)[:128, :128], lambda pr: pr(40).reshape(256, 256)[:128, :128]),
        ("V after level 2", lambda d, i, pr: _chroma(d, i, 1)[:128, :128], lambda pr: pr(41).reshape(256, 256)[:128, :128])],
    9: [("U after the corrections", lambda d, i, pr: _chroma(d, i, 0)[:128, :128], lambda pr: pr(42).reshape(256, 256)[:128, :128]),
        ("V after the corrections", lambda d, i, pr: _chroma(d, i, 1)[:128, :128], lambda pr: pr(43).reshape(256, 256)[:128, :128])],
    10: [("U before the sharpening", lambda d, i, pr: _chroma(d, i, 0), lambda pr: pr(44).reshape(256, 256)),
         ("V before the sharpening", lambda d, i, pr: _chroma(d, i, 1), lambda pr: pr(45).reshape(256, 256))],
    11: [("U sharpened", lambda d, i, pr: _sharp(d, i, 0), lambda pr: pr(46).reshape(256, 256).astype(np.uint8)),
         ("V sharpened", lambda d, i, pr: _sharp(d, i, 1), lambda pr: pr(47).reshape(256, 256).astype(np.uint8))],
}


def run_to(dec, files, stop, mode):
    assert dec.lib.nhw_dec_debug_slice_order(dec.h, mode) == 0
    dec.lib.nhw_dec_debug_stop_after(dec.h, stop)
    try:
        return dec.decode(files)
    finally:
        dec.lib.nhw_dec_debug_stop_after(dec.h, 0)
        assert dec.lib.nhw_dec_debug_slice_order(dec.h, 0) == 0


def dec_batch(dec, files):
    """nhw_dec_batch, max_batch files a call (the call takes no more), every output slot filled with the canary first"""
    n, mb = len(files), dec.max_batch
    out = np.full((n, 512, 512, 3), CANARY, np.uint8); status = np.full(n, 77, np.int32); quality = np.full(n, 77, np.int32)
    for i0 in range(0, n, mb):
        part = files[i0:i0 + mb]
        offs = np.zeros(len(part) + 1, np.uint64); offs[1:] = np.cumsum([len(f) for f in part])
        blob = np.frombuffer(b"".join(part), np.uint8)
        assert dec.lib.nhw_dec_batch(dec.h, blob.ctypes.data, offs.ctypes.data, len(part), out[i0:].ctypes.data, status[i0:].ctypes.data,
                                     quality[i0:].ctypes.data) == 0
    return out, status, quality
