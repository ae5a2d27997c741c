"""What a toned call and the two histogram kernels must produce, shared by test_tone_rule.py, test_tone_table.py and
test_tone_hist.py.  Nothing expected here comes from the code under test: the tables are written out here, the table's rule is a numpy gather,
the bytes it is applied to are those of the existing UNMAPPED or MAPPED call in the format U8 / HWC / BGR / file rows (pinned by the
resamplers', the warp's and the colour map's own tests), an element is tensor_cases.expected_tensor's or grey_cases.expected_grey_tensor's exact
value rule, a histogram is numpy.bincount, and the two rules that make a row from a histogram are restated here in numpy int64."""
import ctypes

import numpy as np

from tests.support import CANARY

GUARD = 4096
NHW_E_ARG = -4
KEEP, EQUALIZE, AUTOCONTRAST = 0, 1, 2
SYMBOLS = ("nhw_resample_toned_to_tensor_device", "nhw_warp_toned_to_tensor_device", "nhw_dec_crops_toned_to_device", "nhw_dec_warps_toned_to_device",
           "nhw_hist_device", "nhw_tone_from_hist_device")


def _tables():
    rng = np.random.default_rng(2501)
    x = np.arange(256, dtype=np.uint8)
    perms = np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)])
    assert not any(np.array_equal(perms[a], perms[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    return {
        "identity": np.stack([x, x, x]),
        "inversion": np.stack([255 - x] * 3),
        "permutations": perms,                                       # a different one a channel: a row read for the wrong channel, or B and R exchanged, shows
        "constants": np.stack([np.full(256, v, np.uint8) for v in (3, 141, 250)]),
        "posterize 1": np.stack([x & 128] * 3),
    }


# uint8 [3, 256] a table, rows in the struct's order B, G, R
TABLES = _tables()


def apply_tone(px, table):
    """the rule in numpy: px uint8 [..., 3] (B, G, R), table uint8 [3, 256] in the struct's order -> uint8 [..., 3]"""
    return np.stack([table[c][px[..., c]] for c in range(3)], axis=-1)


def apply_tone_grey(px, table):
    """the one-channel form: px uint8 [...] -> uint8 [...], from row 0 alone"""
    return table[0][px]


def tone_table(tables):
    """the nhw_tone_table table of a list of [3, 256] tables: uint8 [n, 768]"""
    return np.ascontiguousarray(np.stack([np.asarray(t, np.uint8).reshape(768) for t in tables]))


def drawn(n, first=0):
    """n tables, a different one for every sample of a batch up to 15, so that a table read for the wrong entry shows: the named ones walked from
    `first`, every third as it is, the others behind a seeded permutation of their own on every channel and shifted by 17 i + c (so that the
    constants differ too)"""
    names = list(TABLES)
    out = []
    for i in range(n):
        rng = np.random.default_rng(2600 + first + i)
        t = TABLES[names[(first + 2 * i) % len(names)]]
        out.append(np.stack([(t[c][rng.permutation(256)].astype(np.int64) + 17 * i + c) % 256 for c in range(3)]).astype(np.uint8) if i % 3 else t)
    assert len({t.tobytes() for t in out}) == n
    return out


def launch(table, out_w, out_h, fmt, channels, filter=None, flags=None, warps=None, maps=None, tones=None, null_tones=False, other_addr=None):
    """One launch over a host picture table into a canary-filled batch between two guards: the resamplers (filter: its number) or the warp
    (warps: the nhw_warp table).  With `tones` (uint8 [n, 768]) or null_tones the TONED entry, `maps` (a colour table) or a null pointer in front
    of it; else with `maps` the mapped entry; else the unmapped one of `channels` bytes a pixel.  other_addr: {entry: function of its slot's
    address} -> (rc, the slots as byte arrays, guards intact)"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    n, per, es = len(table), channels * out_w * out_h, fmt.dtype.itemsize
    buf = torch.full((2 * GUARD + n * per * es,), CANARY, dtype=torch.uint8, device="cuda")
    slots = [buf.data_ptr() + GUARD + i * per * es for i in range(n)]
    addr = torch.tensor([(other_addr or {}).get(i, int)(s) for i, s in enumerate(slots)], dtype=torch.int64, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    d_tab = dev(table)
    c = fmt.c_struct()
    toned = tones is not None or null_tones
    d_m = dev(maps) if maps is not None else None
    d_t = torch.from_numpy(np.ascontiguousarray(tones)).cuda() if tones is not None else None
    extra = ()
    if toned:
        extra = (d_m.data_ptr() if d_m is not None else None, d_t.data_ptr() if d_t is not None else None)
    elif maps is not None:
        extra = (d_m.data_ptr(),)
    if warps is not None:
        d_w = dev(warps)
        call = L.nhw_warp_toned_to_tensor_device if toned else L.nhw_warp_mapped_to_tensor_device if maps is not None else (
            L.nhw_warp_to_tensor_device if channels == 3 else L.nhw_warp_grey_to_tensor_device)
        rc = call(d_tab.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_w.data_ptr(), *extra, addr.data_ptr(), None)
    else:
        d_f = torch.from_numpy(np.asarray(flags, np.uint8)).cuda() if flags is not None else None
        call = L.nhw_resample_toned_to_tensor_device if toned else L.nhw_resample_mapped_to_tensor_device if maps is not None else (
            L.nhw_resample_to_tensor_device if channels == 3 else L.nhw_resample_grey_to_tensor_device)
        rc = call(d_tab.data_ptr(), n, out_w, out_h, filter, ctypes.byref(c), d_f.data_ptr() if d_f is not None else None, *extra, addr.data_ptr(), None)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == CANARY).all() and (host[GUARD + n * per * es:] == CANARY).all())
    return rc, [host[GUARD + i * per * es: GUARD + (i + 1) * per * es] for i in range(n)], intact


# ---------------------------------------------------------------- the two rules that make a row from a histogram, in numpy int64
def equalize_row(h):
    """PIL's ImageOps.equalize / torchvision's _scale_channel on a histogram of 256 counts (each below 2^32: the sums stay below 2^40)"""
    h = np.asarray(h).astype(np.int64)
    nz = np.flatnonzero(h)
    total, last = int(h.sum()), int(h[nz[-1]]) if len(nz) else 0
    step = (total - last) // 255
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    before = np.concatenate([[0], np.cumsum(h)[:-1]])
    row = np.minimum(np.floor_divide(before + step // 2, step), 255)
    row[0] = 0
    return row.astype(np.uint8)


def autocontrast_row(h):
    """clamp(floor(255 (x - lo) / (hi - lo))) between the lowest and the highest non-empty bin; the identity where lo >= hi or nothing is counted"""
    nz = np.flatnonzero(np.asarray(h))
    if len(nz) == 0 or nz[0] >= nz[-1]:
        return np.arange(256, dtype=np.uint8)
    lo, hi = int(nz[0]), int(nz[-1])
    return np.clip(np.floor_divide(255 * (np.arange(256, dtype=np.int64) - lo), hi - lo), 0, 255).astype(np.uint8)


def _hist(pairs):
    h = np.zeros(256, np.uint64)
    for x, v in pairs:
        h[x] = v
    return h


def _spread():
    """a total of 2^32 - 1: bin 255 holds 1000 and the bins below share the rest, so that at x = 255 the running sum 2^32 - 1001 plus step / 2
    (8 421 502) is above 2^32"""
    rest = (1 << 32) - 1 - 1000
    h = np.full(256, rest // 255, np.uint64)
    h[:rest % 255] += 1
    h[255] = 1000
    return h


# the crafted histograms, uint64 [256] each, every count below 2^32
HISTS = {
    "empty": _hist([]),
    "one bin": _hist([(77, 12345)]),
    "one bin at 0": _hist([(0, 5)]),
    "two adjacent bins": _hist([(100, 300), (101, 700)]),
    "two bins at 0 and 255": _hist([(0, 40000), (255, 60000)]),
    "flat": np.full(256, 100, np.uint64),
    "step exactly 1": _hist([(x, 1) for x in range(255)] + [(255, 7)]),
    "total - last = 254": _hist([(x, 1) for x in range(254)] + [(255, 9)]),
    "total - last = 255 in one bin": _hist([(3, 255), (200, 1)]),
    "one bin of 65535^2": _hist([(200, 65535 * 65535)]),
    "65535^2 in two bins": _hist([(10, 65535 * 65535 - 4000000000), (250, 4000000000)]),
    "2^32 - 1 spread": _spread(),
    "every bin 2^32 - 1": np.full(256, (1 << 32) - 1, np.uint64),
    "a narrow band": _hist([(x, 1000 + 37 * x) for x in range(90, 141)]),
}
assert int(_spread().sum()) == (1 << 32) - 1 and int(_spread()[:255].sum()) + int(_spread()[:255].sum()) // 255 // 2 >= 1 << 32
assert (int(HISTS["step exactly 1"].sum()) - 7) // 255 == 1 and (int(HISTS["total - last = 254"].sum()) - 9) // 255 == 0


def random_hists(n, seed):
    """n seeded histograms of mixed kinds: dense, sparse, heavy-tailed"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        top = int(rng.choice([2, 50, 5000, 1 << 20, (1 << 32) - 1]))
        h = rng.integers(0, top + 1, 256, dtype=np.uint64)
        if i % 3 == 1:
            h[rng.random(256) < 0.9] = 0
        if i % 5 == 2:
            h[:int(rng.integers(0, 200))] = 0
        out.append(h)
    return out


def hists_text(hists):
    """histograms as tests/tone/check.cpp reads them: 256 counts a line"""
    return "".join(" ".join(str(int(v)) for v in h) + "\n" for h in hists)


def hist_words(hists):
    """[n][C][256] histograms as the uint32 words the device entry reads, in an int32 array"""
    return np.ascontiguousarray(np.asarray(hists, np.uint64).astype(np.uint32)).view(np.int32)
