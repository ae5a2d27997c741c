"""What the grey windows, crops, resamplers and warps must produce, shared by test_grey_api.py, test_grey_window_copy.py,
test_grey_resample.py and test_grey_pictures.py.  Nothing expected here comes from the code under test:
  - the grey picture of a container at scale s is grey_cases.expected_grey (the oracle's luma through the oracle's colour matrix at neutral
    chroma) of each tile file, laid on the tile grid and cut to the scaled size;
  - a resampled or warped result is what the COLOUR kernel of the same call (resize_to_tensor_device / warp_to_tensor_device, uint8 HWC BGR,
    pinned against their numpy rules by their own tests) makes of the grey picture replicated into three channels: its three channels must
    agree, and channel 0 is the expected byte;
  - a tensor element is tensor_cases.exact_elements' value rule under scale[0] and bias[0] (grey_cases.expected_grey_tensor)."""
import ctypes

import numpy as np

from tests.grey_cases import expected_grey, expected_grey_tensor
from tests.picture_cases import parse_container
from tests.support import CANARY

GUARD = 4096
NHW_E_ARG, NHW_E_FORMAT = -4, -6
SYMBOLS = ("nhw_untile_windows_grey_device", "nhw_resample_grey_to_tensor_device", "nhw_warp_grey_to_tensor_device", "nhw_dec_windows_grey",
           "nhw_dec_windows_grey_to_device", "nhw_dec_crops_grey_to_device", "nhw_dec_warps_grey_to_device")
FILTERS = ("two_tap", "area", "cubic")


def byte_format():
    """the colour reference's format: the byte path's own"""
    import nhwcodec_amd as na
    return na.TensorFormat("uint8", "HWC", "BGR", "file")


def grey_picture(oracle, container, scale):
    """the grey picture of a .nhwp container at `scale`, uint8 [ceil(H / scale), ceil(W / scale)]"""
    w, h, files = parse_container(container)
    nx, ny, T = -(-w // 512), -(-h // 512), 512 // scale
    rows = [np.concatenate([expected_grey(oracle, files[ty * nx + tx], scale) for tx in range(nx)], axis=1) for ty in range(ny)]
    full = np.concatenate(rows, axis=0)
    assert full.shape == (ny * T, nx * T)
    return np.ascontiguousarray(full[:-(-h // scale), :-(-w // scale)])


def grey_views(specs, seed):
    """one-channel pictures as uint8 CUDA views [H, W] into one byte buffer: spec (W, H, pitch extra, byte misalignment of addr) -> (buffer,
    views, their numpy copies)"""
    import torch
    rng = np.random.default_rng(seed)
    at, offs = 256, []
    for w, h, extra, mis in specs:
        at = (at + 255) // 256 * 256 + mis
        offs.append(at)
        at += (w + extra) * h + 64
    buf = torch.from_numpy(rng.integers(0, 256, at + 256, dtype=np.uint8)).cuda()
    views = [buf.as_strided((h, w), (w + extra, 1), o) for (w, h, extra, _), o in zip(specs, offs)]
    return buf, views, [v.cpu().numpy() for v in views]


def three(grey):
    """a grey picture (numpy [H, W]) replicated into three channels, as a packed CUDA tensor [H, W, 3]"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))).cuda()


def _one_channel(t, what):
    """the colour reference's result [n, out_h, out_w, 3] -> channel 0, after the three have been seen to agree"""
    r = t.cpu().numpy()
    assert (r[..., 0] == r[..., 1]).all() and (r[..., 1] == r[..., 2]).all(), f"{what}: the colour reference's channels differ on a grey picture"
    return np.ascontiguousarray(r[..., 0])


def reference_resize(greys, size, flips, filter):
    """the expected bytes of a grey resize, uint8 [n, out_h, out_w]: the colour kernel on the replicated pictures"""
    import nhwcodec_amd as na
    return _one_channel(na.resize_to_tensor_device([three(g) for g in greys], size, byte_format(), flips=flips, filter=filter), f"resize {filter}")


def reference_warp(greys, matrices, size, fill, border):
    """... and of a grey warp: the border colour is the byte in all three places"""
    import nhwcodec_amd as na
    return _one_channel(na.warp_to_tensor_device([three(g) for g in greys], matrices, size, byte_format(), fill=(fill, fill, fill), border=border), f"warp {border}")


def bits_of(t):
    """a tensor's bit patterns on the host"""
    import torch
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().view(np.uint16 if t.element_size() == 2 else np.uint32)


def assert_tensors(got_bits, want_bytes, fmt, what):
    """got_bits [n, ...] against the value rule on the expected bytes [n, out_h, out_w]"""
    assert len(got_bits) == len(want_bytes), what
    for i, (g, b) in enumerate(zip(got_bits, want_bytes)):
        want = expected_grey_tensor(b, fmt)
        assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.dtype, want.shape)
        bad = g != want
        assert not bad.any(), f"{what}, entry {i}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


def picture_table(views):
    """the nhw_picture table of one-byte views, on the host"""
    import nhwcodec_amd as na
    t = np.zeros(len(views), na.PICTURE_DTYPE)
    for i, v in enumerate(views):
        h, w = v.shape
        t[i] = (v.data_ptr(), v.stride(0) if h > 1 else w, w, h, 0, 0)
    return t


def launch_grey(table, out_w, out_h, fmt, filter=None, flags=None, warps=None, other_addr=None):
    """one launch of nhw_resample_grey_to_tensor_device (filter: its number) or nhw_warp_grey_to_tensor_device (warps: the nhw_warp table) over a
    host table into a canary-filled batch between two guards; other_addr: {entry: function of its slot's address} for the entries that get
    another address -> (rc, the slots as byte arrays, guards intact)"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    n, per, es = len(table), out_w * out_h, fmt.dtype.itemsize
    buf = torch.full((2 * GUARD + n * per * es,), CANARY, dtype=torch.uint8, device="cuda")
    slots = [buf.data_ptr() + GUARD + i * per * es for i in range(n)]
    addr = torch.tensor([(other_addr or {}).get(i, int)(s) for i, s in enumerate(slots)], dtype=torch.int64, device="cuda")
    d_tab = torch.from_numpy(np.ascontiguousarray(table).view(np.int64).copy()).cuda()
    c = fmt.c_struct()
    if warps is not None:
        d_w = torch.from_numpy(np.ascontiguousarray(warps).view(np.int64).copy()).cuda()
        rc = L.nhw_warp_grey_to_tensor_device(d_tab.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_w.data_ptr(), addr.data_ptr(), None)
    else:
        d_f = torch.from_numpy(np.asarray(flags, np.uint8)).cuda() if flags is not None else None
        rc = L.nhw_resample_grey_to_tensor_device(d_tab.data_ptr(), n, out_w, out_h, filter, ctypes.byref(c), d_f.data_ptr() if d_f is not None else None, addr.data_ptr(), None)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == CANARY).all() and (host[GUARD + n * per * es:] == CANARY).all())
    return rc, [host[GUARD + i * per * es: GUARD + (i + 1) * per * es] for i in range(n)], intact


def slot_bits(slot, fmt, out_h, out_w):
    """a slot's bytes as the tensor's bit patterns"""
    return slot.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[fmt.dtype.itemsize]).reshape(fmt.shape(out_h, out_w))

