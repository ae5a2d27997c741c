"""What the blur rule must produce, for test_blur_rule.py.  Nothing expected here comes from the code under test: the
rule is restated in numpy int64 from its words (blur_model), and the records are built here field by field (record)."""
import numpy as np

ONE, MIX_ONE, MAX_RADIUS, MAX_MIX = 32768, 65536, 15, 16 * 65536
REFLECT, REPLICATE = 0, 1
BLUR = np.dtype([("wx", "<u2", (32,)), ("wy", "<u2", (32,)), ("mix", "<i4"), ("rx", "u1"), ("ry", "u1"), ("border", "u1"), ("reserved8", "u1"),
                 ("reserved", "<u4", (2,))])                          # the tests' own mirror of nhw_blur
assert BLUR.itemsize == 144


def record(wx, wy, mix=MIX_ONE, border=REFLECT, rx=None, ry=None):
    """one nhw_blur, field by field: taps as given (integers), the radii from their count unless named"""
    r = np.zeros((), BLUR)
    r["wx"][:len(wx)], r["wy"][:len(wy)] = wx, wy
    r["mix"], r["border"] = mix, border
    r["rx"], r["ry"] = (len(wx) // 2 if rx is None else rx), (len(wy) // 2 if ry is None else ry)
    return r[()]


def ix(i, n, border):
    """the border's index, on integer arrays"""
    i = np.asarray(i, np.int64)
    if border == REFLECT:
        return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    return np.clip(i, 0, n - 1)


def blur_model(px, wx, wy, mix=MIX_ONE, border=REFLECT):
    """the four steps in numpy int64: px uint8 [H, W] or [H, W, C] -> uint8 of that shape.  Every sum is taken in 64 bits; the divisions are
    floor divisions"""
    p = px.astype(np.int64).reshape(px.shape[0], px.shape[1], -1)
    H, W, _ = p.shape
    wx, wy = np.asarray(wx, np.int64), np.asarray(wy, np.int64)
    rx, ry = len(wx) // 2, len(wy) // 2
    cols = ix(np.arange(W)[:, None] + np.arange(2 * rx + 1)[None, :] - rx, W, border)             # [W, taps]
    h = np.floor_divide((p[:, cols, :] * wx[None, None, :, None]).sum(axis=2) + 64, 128)           # [H, W, C], 0 .. 65280
    assert h.min() >= 0 and h.max() <= 65280
    rows = ix(np.arange(H)[:, None] + np.arange(2 * ry + 1)[None, :] - ry, H, border)             # [H, taps]
    s = (h[rows] * wy[None, :, None, None]).sum(axis=1)
    assert s.max() + (1 << 22) < 1 << 31
    b = np.floor_divide(s + (1 << 22), 1 << 23)
    z = np.clip(p + np.floor_divide(int(mix) * (b - p) + 32768, 65536), 0, 255)
    return z.astype(np.uint8).reshape(px.shape)


def model_of(px, rec):
    """blur_model under a record"""
    rx, ry = int(rec["rx"]), int(rec["ry"])
    return blur_model(px, rec["wx"][:2 * rx + 1], rec["wy"][:2 * ry + 1], int(rec["mix"]), int(rec["border"]))


def one_tap(radius, at):
    """2 radius + 1 taps, all of the weight in tap `at`"""
    t = [0] * (2 * radius + 1)
    t[at] = ONE
    return t


def int_taps(weights):
    """the tests' own taps of float weights: rint(32768 w / sum), the deficit to the centre"""
    w = np.asarray(weights, np.float64)
    t = np.rint(ONE * w / w.sum()).astype(np.int64)
    t[len(t) // 2] += ONE - t.sum()
    assert t.min() >= 0
    return [int(v) for v in t]


def gaussian(sigma, radius):
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    return np.exp(-0.5 * (x / sigma) ** 2)


# ---------------------------------------------------------------- the text file of tests/blur/check.cpp
def check_cases():
    """(W, H, C, record, picture uint8 [H, W, C]) of the stand-alone program: the extreme sums, a tap of 32768 at every position, the extreme mixes
    against differences of +-255, both borders, radii up to the side under reflect"""
    rng = np.random.default_rng(2601)
    cases = []
    full = lambda w, h, c, v: np.full((h, w, c), v, np.uint8)
    board = lambda w, h, c: np.broadcast_to((((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)[:, :, None], (h, w, c)).copy()
    rand = lambda w, h, c: rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    box15, g15 = int_taps([1.0] * 31), int_taps(gaussian(5.0, 15))
    for c in (1, 3):
        for border in (REFLECT, REPLICATE):
            cases.append((33, 17, c, record(box15, box15, MIX_ONE, border), full(33, 17, c, 255)))          # all bytes 255 at radius 15
            cases.append((16, 16, c, record(g15, g15, MIX_ONE, border), rand(16, 16, c)))                 # the reflection reaches the far edge
            cases.append((17, 33, c, record(int_taps(gaussian(1.0, 3)), g15, 32768, border), rand(17, 33, c)))
    for at in range(31):                                                                                     # one tap of 32768 at every position
        for border in (REFLECT, REPLICATE):
            cases.append((19, 18, 1, record(one_tap(15, at), [ONE], MIX_ONE, border), rand(19, 18, 1)))
            cases.append((18, 19, 1, record([ONE], one_tap(15, at), MIX_ONE, border), rand(18, 19, 1)))
            cases.append((16, 16, 1, record(one_tap(15, at), one_tap(15, 30 - at), MIX_ONE, border), full(16, 16, 1, 255)))
    for mix in (MAX_MIX, -MAX_MIX, MIX_ONE, -MIX_ONE, 32768, -32768, 1, -1, 0):                           # b - p = +-255 on a checkerboard moved by one
        cases.append((9, 7, 3, record(one_tap(1, 0), [ONE], mix, REPLICATE), board(9, 7, 3)))
        cases.append((9, 7, 1, record([ONE], one_tap(1, 2), mix, REFLECT), board(9, 7, 1)))
    cases.append((1, 1, 3, record(box15, g15, MIX_ONE, REPLICATE), rand(1, 1, 3)))
    cases.append((2, 2, 3, record(int_taps([1, 2, 1]), int_taps([1, 2, 1]), MIX_ONE, REFLECT), rand(2, 2, 3)))
    cases.append((5, 4, 1, record([ONE], [ONE], -MAX_MIX, REFLECT), rand(5, 4, 1)))                        # the identity under every mix
    return cases


def check_text(cases):
    """the cases as tests/blur/check.cpp reads them, the model's bytes behind each picture"""
    lines = []
    for w, h, c, r, px in cases:
        rx, ry = int(r["rx"]), int(r["ry"])
        lines.append(f"{w} {h} {c} {int(r['border'])} {rx} {ry} {int(r['mix'])}")
        lines.append(" ".join(str(int(v)) for v in r["wx"][:2 * rx + 1]))
        lines.append(" ".join(str(int(v)) for v in r["wy"][:2 * ry + 1]))
        lines.append(" ".join(str(int(v)) for v in px.reshape(-1)))
        lines.append(" ".join(str(int(v)) for v in model_of(px, r).reshape(-1)))
    return "\n".join(lines) + "\n"
