"""What a mapped call must produce, shared by test_colour_rule.py and test_colour_map.py.  Nothing expected here comes
from the code under test: the table of maps is written out here, the rule is numpy int64 with numpy's floor division, the bytes it is applied
to are those of the existing UNMAPPED call in the format U8 / HWC / BGR / file rows (pinned by test_crops.py, test_area_resize.py,
test_cubic_resize.py, test_warp.py and test_grey_resample.py), and an element is tensor_cases.expected_tensor's or
grey_cases.expected_grey_tensor's exact value rule."""
import ctypes

import numpy as np

from tests.support import CANARY

GUARD = 4096
NHW_E_ARG = -4
ONE, GAIN, OFFSET = 1 << 16, 1 << 20, 1 << 28
SYMBOLS = ("nhw_resample_mapped_to_tensor_device", "nhw_warp_mapped_to_tensor_device", "nhw_dec_crops_mapped_to_device", "nhw_dec_warps_mapped_to_device")
COLOUR = np.dtype([("m", "<i4", (3, 3)), ("o", "<i4", (3,)), ("reserved", "<u4", (4,))])      # the tests' own mirror of nhw_colour_map


def _map(m, o):
    return tuple(int(v) for v in np.asarray(m).reshape(9)) + tuple(int(v) for v in o)


def _corner(a, b, c):
    """every matrix entry at +-2^20 by its column's sign, every offset at +-2^28 with the sign of the majority: (+, +, +) and (-, -, -) reach
    the bound 3 x 255 x 2^20 + 2^28 at either sign"""
    s = 1 if a + b + c > 0 else -1
    return _map([[a * GAIN, b * GAIN, c * GAIN]] * 3, [s * OFFSET] * 3)


# twelve integers a map, in the struct's order B, G, R: m[0][0] .. m[2][2], o[0] .. o[2]
MAPS = {
    "identity": _map(np.eye(3, dtype=np.int64) * ONE, (0, 0, 0)),
    "inversion": _map(-np.eye(3, dtype=np.int64) * ONE, (255 * ONE,) * 3),
    "half": _map(np.eye(3, dtype=np.int64) * (ONE // 2), (0, 0, 0)),                    # every odd byte on a tie: 1 -> 1, 3 -> 2: halves go up
    "minus half": _map(-np.eye(3, dtype=np.int64) * (ONE // 2), (200 * ONE,) * 3),      # ... and at the other sign: 200 - 1/2 -> 200
    "minus half below zero": _map(-np.eye(3, dtype=np.int64) * (ONE // 2), (3 * ONE, 0, -ONE // 2)),   # ties among negative sums: all clamped, none past 0
    "luma mix": _map([[7471, 38470, 19595]] * 3, (0, 0, 0)),                            # 0.114, 0.587, 0.299 on B, G, R: the sum is 65536
    "rotation": _map([[0, ONE, 0], [0, 0, ONE], [ONE, 0, 0]], (0, 0, 0)),               # B <- G, G <- R, R <- B
    "contrast": _map(np.eye(3, dtype=np.int64) * (3 * ONE // 2), (-64 * ONE,) * 3),     # 1.5 x - 64: clamps at both ends
    **{f"corner {'+' if a > 0 else '-'}{'+' if b > 0 else '-'}{'+' if c > 0 else '-'}": _corner(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)},
}
assert len(MAPS) == 16 and len(set(MAPS.values())) == 16


def maps_text():
    """the table as tests/colour/check.cpp reads it: twelve integers a line"""
    return "".join(" ".join(str(v) for v in m) + "\n" for m in MAPS.values())


def apply_map(px, twelve):
    """the rule in numpy int64: px uint8 [..., 3] (B, G, R) -> uint8 [..., 3]; floor_divide floors at either sign"""
    m, o = np.array(twelve[:9], np.int64).reshape(3, 3), np.array(twelve[9:], np.int64)
    t = px.astype(np.int64) @ m.T + o
    return np.clip(np.floor_divide(t + 32768, 65536), 0, 255).astype(np.uint8)


def apply_grey(px, twelve):
    """the one-channel form: px uint8 [...] -> uint8 [...], from m[0][0] and o[0] alone"""
    t = px.astype(np.int64) * int(twelve[0]) + int(twelve[9])
    return np.clip(np.floor_divide(t + 32768, 65536), 0, 255).astype(np.uint8)


def map_table(twelves, reserved=None):
    """the nhw_colour_map table of a list of twelve-integer maps; reserved: {entry: (word, value)}"""
    t = np.zeros(len(twelves), COLOUR)
    for i, m in enumerate(twelves):
        t[i]["m"], t[i]["o"] = np.array(m[:9]).reshape(3, 3), m[9:]
    for i, (k, v) in (reserved or {}).items():
        t[i]["reserved"][k] = v
    return t


def drawn(n, first=0):
    """n maps of the table, walking it from `first`, so that a batch of a few entries still meets extremes, ties and negatives"""
    names = list(MAPS)
    return [MAPS[names[(first + 5 * i) % len(names)]] for i in range(n)]


def colour_views(specs, seed):
    """three-byte pictures as uint8 CUDA views [H, W, 3] into one byte buffer, spec (W, H, pitch extra, byte misalignment of addr) -> (buffer,
    views); the last picture of the specs holds every byte value in every channel (a ramp) where it has 256 pixels"""
    import torch
    rng = np.random.default_rng(seed)
    at, offs = 256, []
    for w, h, extra, mis in specs:
        at = (at + 255) // 256 * 256 + mis
        offs.append(at)
        at += (3 * w + extra) * h + 64
    host = rng.integers(0, 256, at + 256, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    views = [buf.as_strided((h, w, 3), (3 * w + extra, 3, 1), o) for (w, h, extra, _), o in zip(specs, offs)]
    w, h = specs[-1][:2]
    if w * h >= 256:
        ramp = (np.arange(w * h) % 256).astype(np.uint8).reshape(h, w)
        views[-1].copy_(torch.from_numpy(np.stack([ramp, ramp[::-1, ::-1], (ramp * 7 + 3).astype(np.uint8)], axis=2)).cuda())
    return buf, views


def picture_table(views, na):
    """the nhw_picture table of views [H, W, 3] or [H, W], on the host"""
    t = np.zeros(len(views), na.PICTURE_DTYPE)
    for i, v in enumerate(views):
        h, w = v.shape[:2]
        t[i] = (v.data_ptr(), v.stride(0) if h > 1 else w * (3 if v.dim() == 3 else 1), w, h, 0, 0)
    return t


def launch(table, out_w, out_h, fmt, channels, filter=None, flags=None, warps=None, maps=None, other_addr=None, null_maps=False):
    """One launch over a host picture table into a canary-filled batch between two guards: the resamplers (filter: its number) or the warp
    (warps: the nhw_warp table); with `maps` (a COLOUR table) or null_maps the MAPPED entry, else the unmapped one of `channels` bytes a pixel.
    other_addr: {entry: function of its slot's address} -> (rc, the slots as byte arrays, guards intact)"""
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
    mapped = maps is not None or null_maps
    d_m = dev(maps) if maps is not None else None
    m_arg = (d_m.data_ptr() if d_m is not None else None,) if mapped else ()
    if warps is not None:
        d_w = dev(warps)
        call = L.nhw_warp_mapped_to_tensor_device if mapped else (L.nhw_warp_to_tensor_device if channels == 3 else L.nhw_warp_grey_to_tensor_device)
        rc = call(d_tab.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_w.data_ptr(), *m_arg, addr.data_ptr(), None)
    else:
        d_f = torch.from_numpy(np.asarray(flags, np.uint8)).cuda() if flags is not None else None
        call = L.nhw_resample_mapped_to_tensor_device if mapped else (L.nhw_resample_to_tensor_device if channels == 3 else L.nhw_resample_grey_to_tensor_device)
        rc = call(d_tab.data_ptr(), n, out_w, out_h, filter, ctypes.byref(c), d_f.data_ptr() if d_f is not None else None, *m_arg, addr.data_ptr(), None)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == CANARY).all() and (host[GUARD + n * per * es:] == CANARY).all())
    return rc, [host[GUARD + i * per * es: GUARD + (i + 1) * per * es] for i in range(n)], intact


def slot_bits(slot, fmt, out_h, out_w):
    """a slot's bytes as the tensor's bit patterns, in the format's own shape"""
    return slot.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[fmt.dtype.itemsize]).reshape(fmt.shape(out_h, out_w))


def untouched(slot):
    return bool((slot == CANARY).all())
