"""What a grey decode must produce, shared by test_grey_rule.py and test_grey_decode.py.  Nothing here comes from the code
under test: the grey table of a quality is the ORACLE's colour matrix at neutral chroma (nhwo_dec_color with U = V = 128, whose three channels
must agree), the luma byte is the oracle decoder's luma plane (scale 1) or section 14's luma as tests/tensor_cases.py builds it (scales 2 and 4),
and a tensor element is tensor_cases.exact_elements' exact-arithmetic value rule under scale[0] and bias[0]."""
import hashlib

import numpy as np

from tests.support import device_arena, golden, golden_names
from tests.tensor_cases import CONSTANTS, DTYPES, SENTINEL, TAIL, exact_elements, expected_planes, oracle_colour, tensor_bits

NHW_E_ARG, NHW_E_FORMAT = -4, -6
SCALES = (1, 2, 4)
# the first entry of tensor_cases.CONSTANTS, its first channel: a grey format takes one number
_FIRST = CONSTANTS[next(iter(CONSTANTS))]
GREY_CONSTANTS = dict(mean=_FIRST["mean"][0], std=_FIRST["std"][0])
GREY_FORMATS = [(d, l, r) for d in DTYPES for l in ("HWC", "CHW") for r in ("file", "reversed")]      # 16
BANDS = ("q10_0.nhw", "q18_0.nhw", "q23_0.nhw")      # a file of quality <= 16, one of 17 .. 19, one of >= 22: the integer, the float and the identity branch

_TABLES, _LUMA, _GREY = {}, {}, {}


def oracle_table(oracle, q):
    """G_q, uint8 [256], read-only: nhwo_dec_color on the 256 luma bytes at U = V = 128; its three channels are asserted equal"""
    if q not in _TABLES:
        y = np.arange(256, dtype=np.uint8).reshape(16, 16)
        c = np.full((16, 16), 128, np.uint8)
        px = oracle_colour(oracle, y, c, c, q).reshape(256, 3)
        assert (px[:, 0] == px[:, 1]).all() and (px[:, 1] == px[:, 2]).all(), f"quality {q}: the oracle's channels differ at neutral chroma"
        t = px[:, 0].copy()
        t.setflags(write=False)
        _TABLES[q] = t
    return _TABLES[q]


def expected_luma(oracle, nhw, scale):
    """(Y uint8 [S, S], quality): scale 1 the oracle decoder's luma plane in front of the colour matrix, scales 2 and 4 section 14's luma"""
    key = (hashlib.sha1(nhw).digest(), scale)
    if key not in _LUMA:
        if scale == 1:
            planes, q = oracle.decode(nhw, planes=True)
            y = np.ascontiguousarray(planes[0])
        else:
            y, _, _, q = expected_planes(oracle, nhw, scale)
        y.setflags(write=False)
        _LUMA[key] = (y, q)
    return _LUMA[key]


def expected_grey(oracle, nhw, scale):
    """the grey bytes of a file, uint8 [S, S], rows in file order; computed once a (file, scale), never written to"""
    key = (hashlib.sha1(nhw).digest(), scale)
    if key not in _GREY:
        y, q = expected_luma(oracle, nhw, scale)
        g = oracle_table(oracle, q)[y]
        g.setflags(write=False)
        _GREY[key] = g
    return _GREY[key]


def grey_format(dtype, layout, rows):
    import nhwcodec_amd as na
    if dtype == "uint8":
        return na.TensorFormat(dtype, layout, "GREY", rows)
    return na.TensorFormat(dtype, layout, "GREY", rows, **GREY_CONSTANTS)


def expected_grey_tensor(grey, fmt):
    """grey uint8 [S, S] -> the bit patterns of the tensor under fmt, [1, S, S] or [S, S, 1]"""
    bits = grey.copy() if fmt.dtype_name == "uint8" else exact_elements(fmt.scale[0], fmt.bias[0], fmt.dtype_name)[grey]
    if fmt.rows == "reversed":
        bits = bits[::-1]
    return np.ascontiguousarray(bits).reshape(fmt.shape(*grey.shape))


def decode_grey(dec, files, scale, fmt=None):
    """one decode_grey_device call into a sentinel-filled buffer -> (the output's bit patterns, status, quality) on the host; what lies behind the
    n * S * S elements is checked"""
    import torch
    n, s = len(files), 512 // scale
    dtype = torch.uint8 if fmt is None else fmt.dtype
    room = n * s * s * dtype.itemsize
    buf = torch.full((room + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    t, st, qq = dec.decode_grey_device(*device_arena(files), scale=scale, fmt=fmt, out=buf[:room].view(dtype))
    torch.cuda.synchronize()
    assert t.dtype == dtype and tuple(t.shape) == ((n, s, s) if fmt is None else (n,) + fmt.shape(s, s)) and t.data_ptr() == buf.data_ptr()
    assert bool((buf[room:] == SENTINEL).all()), "elements behind n * S * S were written"
    return tensor_bits(t), st.cpu().numpy(), qq.cpu().numpy()


def assert_grey(oracle, got, files, status, scale, fmt=None, what=""):
    """every good file's output is the expected grey (under fmt), every refused file's slot still the sentinel"""
    for i, f in enumerate(files):
        if status[i]:
            assert (got[i].view(np.uint8) == SENTINEL).all(), f"{what}: refused file {i}: its slot was written"
            continue
        grey = expected_grey(oracle, f, scale)
        want = grey if fmt is None else expected_grey_tensor(grey, fmt)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape, (got[i].dtype, got[i].shape, want.dtype, want.shape)
        bad = got[i] != want
        assert not bad.any(), f"{what} {fmt} scale {scale} file {i}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


def goldens():
    """every committed decoder file: (names, files)"""
    names = golden_names()
    return names, [golden(n) for n in names]


# the kinds of refused format of the tensor decode, on a grey format: (field, index or None, value).  Entries 1 and 2 of scale and bias are
# checked as ever, though a grey decode does not use them
def c_grey_format(**kw):
    import nhwcodec_amd as na
    c = na.TensorFormat("float32", "CHW", "GREY", "reversed").c_struct()
    for k, v in kw.items():
        if k in ("scale", "bias", "scale1", "bias2"):
            getattr(c, k.rstrip("12"))[int(k[-1]) if k[-1] in "12" else 0] = v
        else:
            setattr(c, k, v)
    return c


REFUSED_GREY_FORMATS = [dict(scale=float("inf")), dict(scale=float("nan")), dict(bias=float("-inf")), dict(bias=float("nan")),
                        dict(scale1=float("nan")), dict(bias2=float("inf")),
                        dict(dtype=4), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(channels=3), dict(channels=-1), dict(rows=2), dict(rows=-1),
                        dict(reserved=1), dict(dtype=0, scale=2.0), dict(dtype=0, bias=1.0), dict(dtype=0, scale1=2.0)]
COLOUR_CHANNELS = [dict(channels=0), dict(channels=1)]      # NHW_T_BGR, NHW_T_RGB: the grey call refuses both
