"""The grey window copy, k_untile_window_grey behind nhw_untile_windows_grey_device, on random tile bytes with no
decode: slots of T x T bytes, segments of 1 .. T bytes where the colour copy has 3 .. 3 T.  The result must be numpy's slice of the tiles laid
on their grid, and no byte outside the windows may be written."""
import ctypes

import numpy as np
import pytest

from tests.picture_cases import Region
from tests.support import CANARY

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 15, 16, 17, 33)
PHASES = (0, 1, 15)                                                  # destination address mod 16


class Use(ctypes.Structure):                                      # the test's own mirror of nhw_window_use
    _fields_ = [(n, ctypes.c_uint32) for n in ("region", "slot", "tx", "ty")]


def _rects(W, H, T, cross):
    """(x, y, w, h) for every width: inside one tile, on the rows 31 / 32 where two bands of a tile meet, over several bands, on the picture's
    last rows and columns, and -- in a picture of 2 x 2 tiles -- across the tile cross"""
    out = []
    for w in WIDTHS:
        out += [(3, 5, w, 3), (7, 31, w, 2), (0, 30, w, 35), (W - w, H - 2, w, 2), (W - w, 0, w, 1), (0, H - 1, w, 1)]
        if cross:
            out += [(T - (w + 1) // 2, T - 2, w, 4), (T - 1, T - 1, w, 2)]
    return out


@pytest.mark.parametrize("scale", (4, 1))
def test_grey_window_copy_writes_the_slices_and_nothing_else(scale):
    import nhwcodec_amd as na
    import torch
    T = 512 // scale
    pictures = [(T + 40, T + 37), (50, T + 5)]                       # W, H: 2 x 2 tiles and 1 x 2 tiles
    grids = [(-(-w // T), -(-h // T)) for w, h in pictures]
    assert grids == [(2, 2), (1, 2)]
    first = [0, 4]
    rng = np.random.default_rng(230 + scale)
    tiles_h = rng.integers(0, 256, (6, T, T), dtype=np.uint8)
    whole = [np.concatenate([np.concatenate(list(tiles_h[f + r * nx:f + (r + 1) * nx]), axis=1) for r in range(ny)], axis=0)[:h, :w]
             for (w, h), (nx, ny), f in zip(pictures, grids, first)]
    tiles = torch.from_numpy(tiles_h).cuda()
    rects = [(p, *r) for p, ((W, H), (nx, ny)) in enumerate(zip(pictures, grids)) for r in _rects(W, H, T, nx == 2 and ny == 2)]
    # destinations: the three phases in turn; the pitch is the width (the phase then turns row by row) or the next odd number above it
    at, place = 256, []
    for i, (_, _, _, w, h) in enumerate(rects):
        pitch = w if i % 2 == 0 else w + 1 + w % 2
        at = (at + 15) // 16 * 16 + PHASES[(i // 2) % 3]
        place.append((at, pitch))
        at += pitch * (h - 1) + w + 48
    assert {(a % 16, p == r[3]) for (a, p), r in zip(place, rects)} == {(ph, eq) for ph in PHASES for eq in (False, True)}
    assert all(p == r[3] or (p > r[3] and p % 2 == 1) for (_, p), r in zip(place, rects))
    buf = torch.full((at + 256,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    views = [buf.as_strided((h, w), (pitch, 1), a) for (a, pitch), (_, _, _, w, h) in zip(place, rects)]
    table = (Region * (len(rects) + 1))()
    uses = []
    for i, ((p, x, y, w, h), (a, pitch)) in enumerate(zip(rects, place)):
        W, H = pictures[p]
        nx = grids[p][0]
        table[i] = Region(buf.data_ptr() + a, pitch, x, y, w, h, W, H, 0xDEAD, 0)          # (first_tile is not read)
        uses += [Use(i, first[p] + ty * nx + tx, tx, ty) for ty in range(y // T, (y + h - 1) // T + 1) for tx in range(x // T, (x + w - 1) // T + 1)]
    good, n_regs = len(uses), len(rects)
    assert good > n_regs                                             # some windows take several tiles
    table[n_regs] = Region(buf.data_ptr() + 16, 8, 0, 0, 8, 8, *pictures[0], 0, 0)         # behind the table's end: a good window no use may reach
    uses += [Use(n_regs, 0, 0, 0), Use(0xFFFFFFFF, 0, 0, 0),                                # a region index out of the table
             Use(0, 6, 0, 0), Use(0, 0xFFFFFFFF, 0, 0),                                     # a slot outside both chunks
             Use(0, 1, 1, 0), Use(0, 2, 0, 1), Use(0, 0, 0xFFFFFFFF, 0)]                    # rect 0 lies inside tile (0, 0): no other tile is of its selection
    assert rects[0][1] + rects[0][3] <= T and rects[0][2] + rects[0][4] <= T
    order = rng.permutation(len(uses))
    uses = [uses[i] for i in order]
    d_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).cuda()
    d_uses = torch.from_numpy(np.frombuffer(bytes((Use * len(uses))(*uses)), np.uint8).copy()).cuda()
    lib = na._library()
    for t0, m in ((4, 2), (0, 4)):                                   # the second chunk first; each launch sees the uses of both
        assert lib.nhw_untile_windows_grey_device(tiles.data_ptr() + t0 * T * T, d_table.data_ptr(), n_regs, d_uses.data_ptr(), len(uses), t0, m, scale, None) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    clean = np.ones(host.size, bool)
    for (p, x, y, w, h), (a, pitch) in zip(rects, place):
        got = np.lib.stride_tricks.as_strided(host[a:], (h, w), (pitch, 1))
        assert np.array_equal(got, whole[p][y:y + h, x:x + w]), (scale, p, x, y, w, h, a % 16, pitch)
        for r in range(h):
            clean[a + r * pitch:a + r * pitch + w] = False
    assert int((~clean).sum()) == sum(r[3] * r[4] for r in rects)
    assert (host[clean] == CANARY).all(), "a byte outside the windows was written"
    assert len(views) == len(rects)
    # what the host can check is refused, and nothing is stored
    args = [tiles.data_ptr(), d_table.data_ptr(), n_regs, d_uses.data_ptr(), len(uses), 0, 4, scale, None]
    for pos, bad in ((0, None), (0, tiles.data_ptr() + 4), (1, None), (2, 0), (3, None), (4, 0), (5, -1), (6, 0), (7, 3), (7, 0), (7, 8)):
        a = list(args)
        a[pos] = bad
        assert lib.nhw_untile_windows_grey_device(*a) == na.NHW_E_ARG, (pos, bad)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy()[clean] == CANARY).all()
