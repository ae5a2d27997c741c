"""What the grey encode tests share: the grey inputs, the oracle's file of a grey picture -- always the colour encode of the
picture with every byte in B, G and R, never the code under test --, and the encode value rule of a one-channel tensor on the host."""
import fractions
import functools

import numpy as np

from tests.tensor_cases import round_to_binary

NHW_E_ARG, NHW_E_QUALITY = -4, -1
GREY_BYTES = 512 * 512
SEEDS = (4000, 4001, 4002, 4003, 4004)


@functools.lru_cache(maxsize=None)
def _synth_grey(seed):
    from oracle.oraclepy import Oracle
    g = np.ascontiguousarray(Oracle().synth(seed)[:, :, 1])
    g.setflags(write=False)
    return g


def synth_grey(seed):
    """the green channel of the oracle's synthetic picture `seed`, uint8 [512, 512], read-only"""
    return _synth_grey(seed)


def all_greys():
    """every grey in every row: uint8 [512, 512], columns 0 .. 255 twice"""
    return np.tile(np.arange(256, dtype=np.uint8), (512, 2))


def replicated(g):
    """the colour picture of a grey one: every byte in B, G and R"""
    return np.ascontiguousarray(np.repeat(g[..., None], 3, 2))


_FILES = {}


def oracle_file(oracle, g, q, compat=False):
    """the oracle's .nhw of the replicated picture, computed once per (picture, quality, mode)"""
    key = (g.tobytes(), q, compat)
    if key not in _FILES:
        oracle.set_oob_mode(compat)
        try:
            _FILES[key] = oracle.encode(replicated(g), q)
        finally:
            oracle.set_oob_mode(False)
    return _FILES[key]


def files_of(out, sizes, status):
    """(out, sizes, status) of a device encode -> (list of files, status list); a status other than 0 is kept as it is"""
    import torch
    torch.cuda.synchronize()
    sz, st = sizes.cpu().numpy(), status.cpu().numpy()
    return [out[i, :int(sz[i])].cpu().numpy().tobytes() if st[i] == 0 else None for i in range(len(sz))], st.tolist()


def _exact_byte(x, scale, bias):
    q = fractions.Fraction(float(x)) * fractions.Fraction(float(scale)) + fractions.Fraction(float(bias))
    if q != 0:
        r = round_to_binary(abs(q), "float32")
        q = r if q > 0 else -r
    return min(255, max(0, round(q)))            # round(Fraction): half-even


def rule_bytes(x, scale, bias):
    """the encode value rule (include/nhw_hip.h) on float64 x, the elements widened exactly, with ONE float32 scale and
    bias: byte = clamp(rint(float32(x * scale + bias)), 0, 255), ties to even, NaN -> 0.  float64 where the sum is farther than 2^-12 from
    every k + 0.5 (its error and the float32 rounding are far below that for |t| < 512; beyond, the clamp decides), exact rationals elsewhere."""
    sc, bi = float(np.float32(scale)), float(np.float32(bias))
    with np.errstate(all="ignore"):
        t = x * sc + bi
        out = np.clip(np.rint(np.where(np.isnan(t), 0.0, t)), 0, 255).astype(np.uint8)
        zone = np.isfinite(t) & (t > -1) & (t < 257) & (np.abs(t - (np.floor(t) + 0.5)) <= 2.0 ** -12)
    memo = {}
    for i in map(tuple, np.argwhere(zone)):
        v = float(x[i])
        if v not in memo:
            memo[v] = _exact_byte(v, sc, bi)
        out[i] = memo[v]
    return out


NP_BITS = {"uint8": np.uint8, "float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}


def widen(bits, dtype):
    """bit patterns -> the values, exactly, as float64"""
    if dtype == "uint8":
        return bits.astype(np.float64)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float32).astype(np.float64)


def to_bits(values32, dtype):
    """float32 values rounded to the element type (uint8: truncated integers) -> its bit patterns"""
    import torch
    if dtype == "uint8":
        return values32.astype(np.uint8)
    if dtype == "float32":
        return np.ascontiguousarray(values32, np.float32).view(np.uint32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return values32.astype(np.float16).view(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(values32, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def to_device(bits, dtype):
    """bit patterns -> a CUDA tensor of the element type with those bits"""
    import torch
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}[bits.dtype]
    return torch.from_numpy(np.array(bits, order="C").view(signed)).cuda().view(getattr(torch, dtype))


def pad_tiles(g):
    """a grey picture [H, W] -> its 512 x 512 tiles by edge replication, row-major, uint8 [T, 512, 512]"""
    h, w = g.shape
    ny, nx = -(-h // 512), -(-w // 512)
    p = np.pad(g, ((0, 512 * ny - h), (0, 512 * nx - w)), mode="edge")
    return np.ascontiguousarray(p.reshape(ny, 512, nx, 512).transpose(0, 2, 1, 3).reshape(ny * nx, 512, 512))
