"""What a decode must produce, as bytes and as tensors, shared by test_scaled_decode.py, test_tensor_decode.py, test_tensor_encode.py, test_crops.py,
test_decode_values.py and test_decode_surgery.py: section 14's half- and quarter-scale pictures built from the oracle decoder's intermediate
planes, section 16's tensors made on the CPU from the specification, and the decode calls into guarded buffers that are held against them.
Each module's own docstring says why these are the expected values."""
import ctypes
import hashlib
import itertools

import numpy as np

from tests.support import CANARY, device_arena

SENTINEL = 0xA5
TAIL = 4096                                     # sentinel bytes kept behind every output

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CONSTANTS = {                                   # name -> TensorFormat keywords
    "imagenet": dict(mean=IMAGENET_MEAN, std=IMAGENET_STD),
    "unit": dict(scale=1 / 255, bias=0),
    "negative": dict(scale=(-1 / 255, -0.5, -2.0), bias=(1.0, 127.5, 3.25)),
    "identity": dict(scale=1, bias=0),
}
DTYPES = ("uint8", "float16", "bfloat16", "float32")
ALL_FORMATS = list(itertools.product(DTYPES, ("HWC", "CHW"), ("BGR", "RGB"), ("file", "reversed")))      # 32


# ---------------------------------------------------------------- the scaled pictures: probes -> planes -> nhwo_dec_color
def _probe16(oracle, nhw, pid, stride):
    return np.frombuffer(oracle.decode_probe(nhw, pid), np.int16).reshape(-1, stride)


def expected_planes(oracle, nhw, scale):
    """(Y, U, V) uint8 [T, T] of section 14's definition, and the file's quality"""
    clip = lambda a: np.clip(a, 0, 255).astype(np.uint8)
    q = oracle.decode(nhw)[1]
    if scale == 2:
        y = clip(_probe16(oracle, nhw, 6, 512)[:256, :256])
        u, v = (clip(_probe16(oracle, nhw, 46 + c, 256)[:256, :256]) for c in (0, 1))
    else:
        y = clip(_probe16(oracle, nhw, 4, 512)[:128, :128].T)
        u, v = (clip(_probe16(oracle, nhw, 42 + c, 256)[:128, :128]) for c in (0, 1))
    return np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v), q


def oracle_colour(oracle, y, u, v, q):
    """the file's own quality branch of nhwo_dec_color on small planes: the function walks 262144 pixels, so the planes sit at the front of
    zero-padded arrays and the first T * T pixels come back"""
    t = y.shape[0]
    fn = oracle.lib.nhwo_dec_color
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    fn.restype = None
    pad = [np.zeros(4 * 65536, np.uint8) for _ in range(3)]
    for p, a in zip(pad, (y, u, v)):
        p[:t * t] = a.reshape(-1)
    out = np.empty(12 * 65536, np.uint8)
    fn(pad[0].ctypes.data, pad[1].ctypes.data, pad[2].ctypes.data, q, out.ctypes.data)
    return out[:3 * t * t].reshape(t, t, 3).copy()


_EXPECTED = {}


def expected(oracle, nhw, scale):
    """the expected scaled picture of a file, uint8 [T, T, 3]; computed once a (file, scale) and never written to"""
    key = (hashlib.sha1(nhw).digest(), scale)
    if key not in _EXPECTED:
        y, u, v, q = expected_planes(oracle, nhw, scale)
        px = oracle_colour(oracle, y, u, v, q)
        px.setflags(write=False)
        _EXPECTED[key] = px
    return _EXPECTED[key]


_BYTES = {}


def expected_bytes(oracle, nhw, scale):
    """the byte path's picture of a file, uint8 [S, S, 3]: the oracle decoder's at scale 1, section 14's at 2 and 4; computed once, never written to"""
    if scale != 1:
        return expected(oracle, nhw, scale)
    if nhw not in _BYTES:
        px = np.array(oracle.decode(nhw)[0], np.uint8).reshape(512, 512, 3)
        px.setflags(write=False)
        _BYTES[nhw] = px
    return _BYTES[nhw]


def decode_scaled(dec, files, scale):
    """one decode_scaled_device call into a canary-backed buffer -> (pixels, status, quality) on the host; the canary is checked"""
    import torch
    n, t = len(files), 512 // scale
    room = n * 3 * t * t
    buf = torch.full((room + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    px, st, qq = dec.decode_scaled_device(*device_arena(files), scale, out=buf)
    torch.cuda.synchronize()
    assert tuple(px.shape) == (n, t, t, 3) and px.data_ptr() == buf.data_ptr()
    assert bool((buf[room:] == CANARY).all()), "bytes behind n * 3 T T were written"
    return px.cpu().numpy(), st.cpu().numpy(), qq.cpu().numpy()


# ---------------------------------------------------------------- the tensors
def tensor_format(dtype, layout, channels, rows, constants=None):
    """the TensorFormat of a parameter tuple; the float types walk through CONSTANTS so that every set meets every dtype"""
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, channels, rows)
    if constants is None:
        constants = list(CONSTANTS)[ALL_FORMATS.index((dtype, layout, channels, rows)) % len(CONSTANTS)]
    return na.TensorFormat(dtype, layout, channels, rows, **CONSTANTS[constants])


def check_constants(fmt):
    """the condition under which the float64 form below IS the single-precision fma"""
    for s, b in zip(fmt.scale, fmt.bias):
        assert np.float32(s) == s and np.float32(b) == b and np.isfinite(s) and np.isfinite(b) and s != 0
        assert b == 0 or abs(int(np.frexp(s)[1]) - int(np.frexp(b)[1])) <= 20, (s, b)


def expected_tensor(px, fmt):
    """the specification on the CPU: px uint8 [H, W, 3] as the byte path writes it -> the bit patterns of the tensor, [H, W, 3] or [3, H, W]"""
    import torch
    check_constants(fmt)
    b = px[..., ::-1] if fmt.channels == "RGB" else px
    if fmt.dtype_name == "uint8":
        bits = b.copy()
    else:
        sc, bi = np.array(fmt.scale, np.float32), np.array(fmt.bias, np.float32)
        x = (b.astype(np.float64) * sc.astype(np.float64) + bi.astype(np.float64)).astype(np.float32)
        if fmt.dtype_name == "float32":
            bits = x.view(np.uint32)
        elif fmt.dtype_name == "float16":
            bits = x.astype(np.float16).view(np.uint16)
        else:
            bits = torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    if fmt.rows == "reversed":
        bits = bits[::-1]
    if fmt.layout == "CHW":
        bits = bits.transpose(2, 0, 1)
    return np.ascontiguousarray(bits)


def tensor_bits(t):
    """a tensor's bit patterns on the host, as unsigned integers"""
    import torch
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def decode_tensor(dec, files, fmt, scale):
    """one decode_tensor_device call into a sentinel-filled buffer -> (the tensor's bit patterns, status, quality) on the host; what lies behind
    n * 3 * S * S elements is checked"""
    import torch
    n, s = len(files), 512 // scale
    room = n * 3 * s * s * fmt.dtype.itemsize
    buf = torch.full((room + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[:room].view(fmt.dtype)
    t, st, qq = dec.decode_tensor_device(*device_arena(files), fmt, scale=scale, out=out)
    torch.cuda.synchronize()
    assert t.dtype == fmt.dtype and tuple(t.shape) == (n,) + fmt.shape(s, s) and t.data_ptr() == buf.data_ptr()
    assert bool((buf[room:] == SENTINEL).all()), "elements behind n * 3 * S * S were written"
    return tensor_bits(t), st.cpu().numpy(), qq.cpu().numpy()


def assert_tensor(oracle, got, files, status, fmt, scale, what=""):
    for i, f in enumerate(files):
        if status[i]:
            assert (got[i].view(np.uint8) == SENTINEL).all(), f"{what}: refused file {i}: its slot was written"
            continue
        want = expected_tensor(expected_bytes(oracle, f, scale), fmt)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape
        bad = got[i] != want
        assert not bad.any(), f"{what} {fmt} scale {scale} file {i}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"
