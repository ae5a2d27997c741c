"""The picture layer in the tests' own words, shared by test_pictures.py, test_picture_fit.py, test_picture_limits.py, test_regions.py,
test_windows.py and test_crops.py: the .nhwp container, the padding rule, the tiles a rectangle selects, the rectangles the tests ask for and
the device buffers they are written into.  Nothing here calls the product: these are what the product is held against."""
import ctypes
import struct

import numpy as np

from tests.support import CANARY

SIZES = [(1, 700), (500, 375), (1023, 1025)]                      # W, H of the windows' and the crops' pictures: 2 + 1 + 6 tiles
# pictures as (W, H, pitch extra, byte misalignment of addr)
SPECS = ([(1, 1, 0, 0), (1, 700, 0, 1), (700, 1, 5, 3), (511, 513, 0, 2), (513, 511, 16, 1), (512, 512, 0, 0), (1023, 1025, 7, 0),
          (1920, 1080, 0, 1)]
         + [(149 + 11 * r, 3 + r, 9 if r % 2 else 0, r % 4) for r in range(16)])          # 3W mod 16 takes every residue


class Region(ctypes.Structure):                                   # the tests' own mirror of nhw_region
    _fields_ = [("addr", ctypes.c_uint64), ("pitch", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in
                ("x", "y", "width", "height", "pic_width", "pic_height", "first_tile", "reserved")]


class Rect(ctypes.Structure):                                     # ... and of nhw_rect
    _fields_ = [(n, ctypes.c_uint32) for n in ("container", "x", "y", "width", "height")]


class World:
    """what a module's `world` fixture hangs its pictures, containers and decoder on"""


# ---------------------------------------------------------------- the container and the padding rule
def parse_container(c):
    """the test's own reading of a .nhwp container -> (W, H, [tile files])"""
    assert c[:8] == b"NHWP\x01\x00\x00\x00"
    w, h = struct.unpack_from("<II", c, 8)
    t = (-(-w // 512)) * (-(-h // 512))
    lens = struct.unpack_from(f"<{t}I", c, 16)
    files, at = [], 16 + 4 * t
    for n in lens:
        files.append(bytes(c[at:at + n]))
        at += n
    assert at == len(c)
    return w, h, files


def make_container(w, h, files, version=1, reserved=b"\0\0\0", magic=b"NHWP", lens=None):
    lens = [len(f) for f in files] if lens is None else lens
    return magic + bytes([version]) + reserved + struct.pack("<II", w, h) + struct.pack(f"<{len(lens)}I", *lens) + b"".join(files)


def pad_reference(pic):
    """the padding rule in numpy: edge replication to whole tiles, then tile_images' cut -> [ny * nx, 512, 512, 3]"""
    h, w = pic.shape[:2]
    ny, nx = -(-h // 512), -(-w // 512)
    big = np.pad(pic, ((0, 512 * ny - h), (0, 512 * nx - w), (0, 0)), mode="edge")
    return np.ascontiguousarray(big.reshape(ny, 512, nx, 512, 3).transpose(0, 2, 1, 3, 4)).reshape(ny * nx, 512, 512, 3)


def padding_mask(pic_shape):
    """True on the padded bytes of a picture's tiles [T, 512, 512, 3]"""
    h, w = pic_shape[:2]
    ny, nx = -(-h // 512), -(-w // 512)
    m = np.ones((512 * ny, 512 * nx, 3), bool)
    m[:h, :w] = False
    return np.ascontiguousarray(m.reshape(ny, 512, nx, 512, 3).transpose(0, 2, 1, 3, 4)).reshape(ny * nx, 512, 512, 3)


def np_picture_sse(tiles, pic):
    """the SSE of a picture's decoded tiles [T, 512, 512, 3], joined and cropped, against the picture"""
    h, w = pic.shape[:2]
    ny, nx = -(-h // 512), -(-w // 512)
    full = tiles.reshape(ny, nx, 512, 512, 3).transpose(0, 2, 1, 3, 4).reshape(512 * ny, 512 * nx, 3)[:h, :w]
    d = full.astype(np.int64) - pic.astype(np.int64)
    return int((d * d).sum())


# ---------------------------------------------------------------- the tiles of a rectangle
def selected(w, scale, x, y, rw, rh, coords=True):
    """the tiles a window of a picture of full width w selects at `scale`, row-major, as (number, tx, ty) -- or, without `coords`, the
    numbers alone: the rule of section 15 in the test's own words; a region (section 13) is the window at scale 1"""
    nx, T = -(-w // 512), 512 // scale
    tiles = [(ty * nx + tx, tx, ty) for ty in range(y // T, (y + rh - 1) // T + 1) for tx in range(x // T, (x + rw - 1) // T + 1)]
    return tiles if coords else [k for k, _, _ in tiles]


def expected_stats(containers, rects, scale, unique):
    """(the tiles the rects select, the bytes of exactly those tile files), the container read by the test's own parser: every tile once
    with `unique` (the windows), else as often as a rect selects it (the regions)"""
    parsed, uses = {}, []
    for ci, x, y, w, h in rects:
        if ci not in parsed:
            parsed[ci] = parse_container(containers[ci])
        uses += [(ci, k) for k in selected(parsed[ci][0], scale, x, y, w, h, coords=False)]
    if unique:
        uses = set(uses)
    return len(uses), sum(len(parsed[ci][2][k]) for ci, k in uses)


def fixed_rects(W, H, T, residues):
    """in a W x H (scaled) picture of tile side T: the whole picture; each corner pixel; a rect inside one tile; one full row; one full
    column; x = T - 1, w = 2; 2 x 2 on a four-tile corner; exactly one tile -- those of them the picture is large enough for; and with
    `residues`, on a picture at least 32 wide, sixteen rects whose x and w take every residue mod 16, so that 3x mod 16 and 3w mod 16 do"""
    r = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),
         (min(3, W - 1), min(5, H - 1), min(W - min(3, W - 1), 200), min(H - min(5, H - 1), 100)), (0, H // 2, W, 1), (W // 2, 0, 1, H)]
    if W > T:
        r.append((T - 1, min(9, H - 1), 2, min(7, H - min(9, H - 1))))
    if W > T and H > T:
        r.append((T - 1, T - 1, 2, 2))
    if W >= T and H >= T:
        r.append((0, 0, T, T))
    if W >= 2 * T and H >= 2 * T:
        r.append((T, T, T, T))
    if residues and W >= 32:
        r += [(i, (7 * i) % H, 1 + i, min(3, H - (7 * i) % H)) for i in range(16)]
    return r


def random_rects(W, H, n, rng, wide, low):
    """n rects of mixed shapes: mostly wide and low (at most `wide` x `low`), every tenth narrow and tall, so that the call's pixels stay small"""
    out = []
    for i in range(n):
        if i % 10 == 9:
            w, h = int(rng.integers(1, min(W, 48) + 1)), int(rng.integers(1, min(H, 1100) + 1))
        else:
            w, h = int(rng.integers(1, min(W, wide) + 1)), int(rng.integers(1, min(H, low) + 1))
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


# ---------------------------------------------------------------- device buffers
def picture_views(specs, seed=0):
    """pictures as uint8 CUDA views [H, W, 3] into one byte buffer: spec (W, H, pitch extra, byte misalignment of addr)"""
    import torch
    rng = np.random.default_rng(seed)
    at, offs = 256, []
    for w, h, extra, mis in specs:
        at = (at + 255) // 256 * 256 + mis
        offs.append(at)
        at += (3 * w + extra) * h + 64
    buf = torch.from_numpy(rng.integers(0, 256, at + 256, dtype=np.uint8)).cuda()
    return buf, [buf.as_strided((h, w, 3), (3 * w + extra, 3, 1), o) for (w, h, extra, _), o in zip(specs, offs)]


def dest_views(shapes):
    """destinations as uint8 CUDA views [h, w, 3] into one canary-filled byte buffer: misalignments 0 .. 15 in turn, pitch gaps of
    1, 5, 16, 7, 3 or 0 bytes, 64 bytes of slack behind a rectangle -- except that every seventh one is packed (pitch 3 w) and its successor
    starts on the very next byte, so that the two share a dword"""
    import torch
    gaps = (0, 1, 5, 16, 7, 3)
    at, offs, extras, packed = 256, [], [], False
    for i, (w, h) in enumerate(shapes):
        extra = 0 if i % 7 == 0 else gaps[i % len(gaps)]
        if not packed:
            at = (at + 15) // 16 * 16 + i % 16
        offs.append(at)
        extras.append(extra)
        at += (3 * w + extra) * (h - 1) + 3 * w
        packed = i % 7 == 0
        if not packed:
            at += 64
    buf = torch.full((at + 256,), CANARY, dtype=torch.uint8, device="cuda")
    return buf, [buf.as_strided((h, w, 3), (3 * w + e, 3, 1), o) for (w, h), e, o in zip(shapes, extras, offs)]


def views_mask(buf, views):
    """True on the bytes of buf that belong to one of its views"""
    import torch
    m = torch.zeros_like(buf, dtype=torch.bool)
    for v in views:
        m.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
    return m


def check_host_result(rects, status, out, out_off, full_of):
    """OK rects hold their slice, every other byte of the buffer is still the canary"""
    clean = np.ones(out.size, bool)
    for i, (ci, x, y, w, h) in enumerate(rects):
        if status[i] == 0:
            a = int(out_off[i])
            assert np.array_equal(out[a:a + 3 * w * h].reshape(h, w, 3), full_of(ci)[y:y + h, x:x + w]), rects[i]
            clean[a:a + 3 * w * h] = False
    assert (out[clean] == CANARY).all()
