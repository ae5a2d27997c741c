"""The picture layer at its limits (DESIGN.md sections 11 to 14): k_tile_pad, k_untile_crop<512|256|128>, k_sse_crop and k_untile_region of
nhw_picture.hip with tables long enough for two and three rounds of their 64-way search, with tile ranges nobody owns, with sides of 65535
and with row offsets past 2^32, and the host calls with more than 64 pictures.

The search is transcribed into Python (model_search); the test without a GPU checks the transcription against bisect and derives from it the
probe tiles the GPU tests launch, so that the probes are known to take every number of rounds a table allows and to sit on the boundaries of
the narrowing (the lane samples, the partial last lane, entries 62 .. 65).  Every GPU comparison is exact equality with numpy -- the padding
rule pad_reference, the crop of the supplied tiles, the SSE of the crop -- or with a path of the project that is pinned elsewhere.

Reached by the probes (asserted in the first test): the picture tables of 65 / 4096 / 4097 / 65535 entries take {1, 2} / {2} / {2, 3} / {3}
rounds (k_tile_pad; k_sse_crop at 4097 and 65535), the 4097 destination pictures of k_untile_crop<512|256|128> {2, 3}, the region tables of
4097 / 65535 entries {2, 3} / {3} (k_untile_region)."""
import bisect

import numpy as np
import pytest

from tests.picture_cases import SPECS, dest_views, np_picture_sse, pad_reference, padding_mask, parse_container, picture_views, selected
from tests.support import CANARY

FILL = 7
PERIOD = 11                                                          # global tile t is given the bytes of random tile t % PERIOD
NS = (1, 2, 64, 65, 4096, 4097, 65535)
MOST_ROUNDS = (0, 1, 1, 2, 2, 3, 3)
ROUNDS_REACHED = {1: {0}, 2: {1}, 64: {1}, 65: {1, 2}, 4096: {2}, 4097: {2, 3}, 65535: {3}}


# ---------------------------------------------------------------- the search, its model and the probes
def model_search(first, ts):
    """find_picture / find_region of nhw_picture.hip for every t of ts at once -> (the entry found, the rounds of loads it took).  Line
    by line the kernel's loop: a lane's sample counts if idx < hi and first_tile[idx] <= t, c is the ballot's popcount."""
    first = np.asarray(first, np.int64)
    ts = np.asarray(ts, np.int64)
    n = len(first)
    lo, hi, rounds = np.zeros(len(ts), np.int64), np.full(len(ts), n, np.int64), np.zeros(len(ts), np.int64)
    while True:
        live = hi - lo > 1
        if not live.any():
            return lo, rounds
        step = (hi - lo + 63) // 64
        c = np.zeros_like(lo)
        for lane in range(64):
            idx = lo + lane * step
            c += (idx < hi) & (first[np.minimum(idx, n - 1)] <= ts)
        new_lo = lo + np.maximum(c - 1, 0) * step
        new_hi = np.minimum(new_lo + step, hi)
        lo, hi, rounds = np.where(live, new_lo, lo), np.where(live, new_hi, hi), rounds + live


def probe_tiles(first, counts, seed=7):
    """the global tiles a GPU test launches for a table: the first and last tile of entries 0, 1, 62, 63, 64, 65, n - 2, n - 1; the first
    tile of round 1's samples lo + lane * step for lanes 0, 1, 63; of the last lane with idx < hi; the last tile of the entry before that
    lane's; 8 seeded random tiles"""
    n = len(first)
    last = lambda k: int(first[k] + counts[k] - 1)                   # noqa: E731
    tiles = set()
    for k in (0, 1, 62, 63, 64, 65, n - 2, n - 1):
        if 0 <= k < n:
            tiles |= {int(first[k]), last(k)}
    step = (n + 63) // 64                                            # round 1: lo = 0, hi = n
    for lane in (0, 1, 63, (n - 1) // step):
        if lane * step < n:
            tiles.add(int(first[lane * step]))
    if (n - 1) // step > 0:
        tiles.add(last((n - 1) // step * step - 1))
    total = int(first[-1] + counts[-1])
    tiles |= {int(t) for t in np.random.default_rng(seed).integers(0, total, 8)}
    return sorted(tiles)


def _tiles(w, h, side=512):
    return (-(-w // side)) * (-(-h // side))


def _first(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


def _pool_specs():
    """32 small source pictures (W, H, pitch extra, misalignment): sides 1 .. 40, every eighth 520 wide (2 tiles)"""
    rng = np.random.default_rng(41)
    return [(520 if i % 8 == 0 else int(rng.integers(1, 41)), int(rng.integers(1, 41)), (0, 5, 16, 7, 9, 3)[i % 6], (5 * i) % 16) for i in range(32)]


POOL = _pool_specs()


def pool_table(n):
    """a table of n pictures, entry k being pool picture 7 k % 32 -> (pool index, tile count, first tile) per entry"""
    p = (7 * np.arange(n)) % 32
    counts = np.array([_tiles(w, h) for w, h, *_ in POOL], np.int64)[p]
    return p, counts, _first(counts)


def crop_shapes(side, n=4097):
    """(W, H) of n destination pictures for tiles of `side`: sides 1 .. 24, every sixteenth side + 8 wide (2 tiles)"""
    rng = np.random.default_rng(43 + side)
    return [(side + 8 if k % 16 == 0 else int(rng.integers(1, 25)), int(rng.integers(1, 25))) for k in range(n)]


def region_rects(n):
    """n regions (x, y, w, h) of a 1024 x 1024 picture: at most 8 x 8 at seeded places, every 50th 2 x 2 on the four-tile corner, the next
    one 2 x 3 across the column border"""
    rng = np.random.default_rng(47 + n)
    w, h = rng.integers(1, 9, n), rng.integers(1, 9, n)
    x, y = rng.integers(0, 1025 - w), rng.integers(0, 1025 - h)
    k = np.arange(n)
    corner, pair = k % 50 == 0, k % 50 == 1
    x[corner | pair], w[corner | pair] = 511, 2
    y[corner], h[corner] = 511, 2
    y[pair], h[pair] = y[pair] % 500, 3
    return [tuple(int(v) for v in r) for r in zip(x, y, w, h)]


def _region_counts(rects):
    return np.array([len(selected(1024, 1, *r)) for r in rects], np.int64)


def _check_model(first, counts, reached):
    """the model finds bisect's entry for every tile of the table (and three behind it); the probes take every round count the table allows"""
    total = int(first[-1] + counts[-1])
    ts = np.arange(total + 3)
    k, rounds = model_search(first, ts)
    fl = [int(f) for f in first]
    assert k.tolist() == [bisect.bisect_right(fl, t) - 1 for t in ts.tolist()]
    probes = probe_tiles(first, counts)
    assert 0 <= probes[0] and probes[-1] < total
    assert set(model_search(first, probes)[1].tolist()) == set(rounds[:total].tolist()) == reached
    return int(rounds.max())


def test_search_model_equals_bisect_and_the_probes_take_every_round_count():
    for n, most in zip(NS, MOST_ROUNDS):
        _, counts, first = pool_table(n)
        assert (n < 9 or (first != np.arange(n)).any()) and _check_model(first, counts, ROUNDS_REACHED[n]) == most
    for side in (512, 256, 128):                                     # the destination tables of the untile test
        counts = np.array([_tiles(w, h, side) for w, h in crop_shapes(side)], np.int64)
        assert counts.max() == 2 and _check_model(_first(counts), counts, {2, 3}) == 3
    for n in (4097, 65535):                                          # the region tables
        counts = _region_counts(region_rects(n))
        assert {1, 2, 4} <= set(counts.tolist()) and _check_model(_first(counts), counts, ROUNDS_REACHED[n]) == 3
    # the partial last lane is among the probes: at n = 4097 lane 63 holds entries 4095 and 4096 only
    _, counts, first = pool_table(4097)
    assert {int(first[4095]), int(first[4095] - 1), int(first[4096])} <= set(probe_tiles(first, counts))
    # a table that starts above tile 0, and entries that share a first tile (an empty one before its successor): the last one wins
    assert model_search([3, 9, 21], [0, 2, 3, 8, 9, 22])[0].tolist() == [0, 0, 0, 0, 1, 2]
    assert model_search([0, 1, 1, 2], [0, 1, 2, 3])[0].tolist() == [0, 2, 3, 3]


# ---------------------------------------------------------------- on the MI355X: helpers
def _upload(table):
    import torch
    return torch.from_numpy(table.view(np.uint8).copy()).cuda()


def _picture_table(views, first):
    """nhw_picture entries for torch views [H, W, 3] with the given first tiles"""
    import nhwcodec_amd as na
    table = np.zeros(len(views), na.PICTURE_DTYPE)
    for i, (v, f) in enumerate(zip(views, first)):
        table[i] = (v.data_ptr(), v.stride(0), v.shape[1], v.shape[0], f, 0)
    return table


def _random_tiles(side, seed):
    """PERIOD random tiles of `side`, the first two repeated behind them, so that any 3 consecutive global tiles t (bytes of tile t % PERIOD)
    lie back to back -> (host [PERIOD + 2, side, side, 3], the same on the device)"""
    import torch
    rand = np.random.default_rng(seed).integers(0, 256, (PERIOD + 2, side, side, 3), dtype=np.uint8)
    rand[PERIOD:] = rand[:2]
    return rand, torch.from_numpy(rand).cuda()


def _host_rows(exp, view, base):
    """the rows of a torch view [H, W, 3] of the device buffer `base` as a writable numpy view [H, 3 W] of the host copy `exp`"""
    h, w = view.shape[:2]
    off = view.data_ptr() - base.data_ptr()
    return np.lib.stride_tricks.as_strided(exp[off:], (h, 3 * w), (view.stride(0), 1))


def _same_bytes(buf, exp, what):
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])} ({int(got[bad[0]])}, not {int(exp[bad[0]])})"


def _join(tiles, ny, nx):
    """tiles [ny nx, S, S, 3], row-major -> [ny S, nx S, 3]"""
    s = tiles.shape[1]
    return tiles.reshape(ny, nx, s, s, 3).transpose(0, 2, 1, 3, 4).reshape(ny * s, nx * s, 3)


def _join_crop(tiles, w, h, side=512):
    return _join(tiles, -(-h // side), -(-w // side))[:h, :w]


def _untile(lib, side, tiles_ptr, table_ptr, n, tile0, m):
    if side == 512:
        return lib.nhw_untile_pictures_device(tiles_ptr, table_ptr, n, tile0, m, None)
    return lib.nhw_untile_pictures_scaled_device(tiles_ptr, table_ptr, n, tile0, m, 512 // side, None)


class Pool:
    pass


@pytest.fixture(scope="module")
def pool():
    """the 32 source pictures on the device, their numpy copies, their padded tiles by pad_reference (host and device) and padding masks"""
    import torch
    p = Pool()
    p.buf, p.views = picture_views(POOL, seed=21)
    p.pics = [v.cpu().numpy() for v in p.views]
    ref = [pad_reference(a) for a in p.pics]
    p.first = _first([len(r) for r in ref])
    p.ref = np.concatenate(ref)
    p.ref_dev = torch.from_numpy(p.ref).cuda()
    p.padding = np.concatenate([padding_mask(a.shape) for a in p.pics])
    assert len({a.tobytes() for a in p.pics}) == 32
    return p


def _pool_table(pool, n):
    import nhwcodec_amd as na
    idx, counts, first = pool_table(n)
    table = np.zeros(n, na.PICTURE_DTYPE)
    table["addr"] = np.array([v.data_ptr() for v in pool.views], np.uint64)[idx]
    table["pitch"] = np.array([v.stride(0) for v in pool.views], np.uint64)[idx]
    table["width"] = np.array([w for w, *_ in POOL], np.uint32)[idx]
    table["height"] = np.array([h for _, h, *_ in POOL], np.uint32)[idx]
    table["first_tile"] = first
    return table, idx, counts, first


# ---------------------------------------------------------------- k_tile_pad on big tables
@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 4096, 4097, 65535])
def test_tile_pad_finds_its_picture_in_a_big_table(pool, n):
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    table, idx, counts, first = _pool_table(pool, n)
    d_table = _upload(table)
    fl, total = first.tolist(), int(first[-1] + counts[-1])
    out = torch.empty((3, 512, 512, 3), dtype=torch.uint8, device="cuda")

    def check(t, m):
        for j in range(3):
            if j >= m or t + j >= total:                             # beyond the launch, or beyond the table: untouched
                assert bool((out[j] == FILL).all()), (n, t, m, j)
                continue
            k = bisect.bisect_right(fl, t + j) - 1
            assert torch.equal(out[j], pool.ref_dev[int(pool.first[idx[k]]) + t + j - fl[k]]), (n, t, m, j, k)

    for t in probe_tiles(first, counts):
        for m in (1, 3):
            out.fill_(FILL)
            assert lib.nhw_tile_pictures_device(d_table.data_ptr(), n, t, m, out.data_ptr(), None) == 0
            check(t, m)
    if n == 4097:                                                    # one launch captured on a side stream
        t = int(first[4095]) - 1                                     # the entry before the partial last lane's, and the two of that lane
        torch.cuda.synchronize()
        g, side_stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(g, stream=side_stream):
            assert lib.nhw_tile_pictures_device(d_table.data_ptr(), n, t, 3, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        out.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(t, 3)


# ---------------------------------------------------------------- k_untile_crop<512 | 256 | 128> on a big table
@pytest.mark.gpu
@pytest.mark.parametrize("side", [512, 256, 128])
def test_untile_crop_finds_its_picture_in_a_big_table(side):
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    shapes = crop_shapes(side)
    n = len(shapes)
    counts = np.array([_tiles(w, h, side) for w, h in shapes], np.int64)
    first = _first(counts)
    fl, total = first.tolist(), int(first[-1] + counts[-1])
    buf, views = dest_views(shapes)
    d_table = _upload(_picture_table(views, first))
    rand, d_rand = _random_tiles(side, 3)
    exp = np.full(buf.numel(), CANARY, np.uint8)
    touched = set()
    for t in probe_tiles(first, counts):
        for m in (1, 3):
            assert _untile(lib, side, d_rand.data_ptr() + (t % PERIOD) * 3 * side * side, d_table.data_ptr(), n, t, m) == 0
            for u in range(t, min(t + m, total)):
                k = bisect.bisect_right(fl, u) - 1
                w, h = shapes[k]
                ty, tx = divmod(u - fl[k], -(-w // side))
                rows, cols = min(side, h - side * ty), min(side, w - side * tx)
                _host_rows(exp, views[k], buf)[side * ty:side * ty + rows, 3 * side * tx:3 * (side * tx + cols)] = \
                    rand[(t % PERIOD) + u - t][:rows, :cols].reshape(rows, 3 * cols)
                touched.add(k)
    torch.cuda.synchronize()
    assert len(touched) > 20 and {0, 1, 62, 63, 64, 65, n - 2, n - 1} <= touched
    _same_bytes(buf, exp, f"tiles of {side}")


# ---------------------------------------------------------------- k_sse_crop on a big table
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4097, 65535])
def test_sse_crop_adds_to_its_own_picture_in_a_big_table(pool, n):
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    table, idx, counts, first = _pool_table(pool, n)
    d_table = _upload(table)
    fl, total = first.tolist(), int(first[-1] + counts[-1])
    rand, d_rand = _random_tiles(512, 4)
    acc = torch.zeros(n, dtype=torch.int64, device="cuda")
    want, known = np.zeros(n, np.int64), {}
    for t in probe_tiles(first, counts):
        for m in (1, 3):
            assert lib.nhw_sse_pictures_device(d_rand.data_ptr() + (t % PERIOD) * na.IMG_BYTES, d_table.data_ptr(), n, t, m, acc.data_ptr(), None) == 0
            for u in range(t, min(t + m, total)):
                k = bisect.bisect_right(fl, u) - 1
                key = (int(pool.first[idx[k]]) + u - fl[k], (t % PERIOD) + u - t)
                if key not in known:
                    d = rand[key[1]].astype(np.int64) - pool.ref[key[0]].astype(np.int64)
                    d[pool.padding[key[0]]] = 0
                    known[key] = int((d * d).sum())
                want[k] += known[key]
    torch.cuda.synchronize()
    assert 20 < np.count_nonzero(want) < 200
    got = acc.cpu().numpy()
    assert np.array_equal(got, want), [(int(k), int(got[k]), int(want[k])) for k in np.flatnonzero(got != want)[:8]]


# ---------------------------------------------------------------- k_untile_region with three search rounds
def _region_table(rects, views, first):
    import nhwcodec_amd as na
    table = np.zeros(len(rects), na.REGION_DTYPE)
    table["addr"] = np.array([v.data_ptr() for v in views], np.uint64)
    table["pitch"] = np.array([v.stride(0) for v in views], np.uint64)
    for j, name in enumerate(("x", "y", "width", "height")):
        table[name] = np.array([r[j] for r in rects], np.uint32)
    table["pic_width"] = table["pic_height"] = 1024
    table["first_tile"] = first
    return table


def _launch_regions(lib, d_table, n, rects, fl, total, views, buf, exp, d_pic_tiles, picture, t, m):
    """one launch over the running tiles [t, t + m): the selected tiles gathered from the picture's, and what it must write put into exp"""
    import torch
    sel = []
    for u in range(t, t + m):
        k = bisect.bisect_right(fl, u) - 1
        if u >= total or u < fl[0]:
            sel.append(3 - u % 2)                                    # nobody's tile: any bytes
            continue
        x, y, w, h = rects[k]
        tile = selected(1024, 1, x, y, w, h, coords=False)[u - fl[k]]
        sel.append(tile)
        ty, tx = divmod(tile, 2)
        r0, r1, c0, c1 = max(512 * ty, y), min(512 * ty + 512, y + h), max(512 * tx, x), min(512 * tx + 512, x + w)
        _host_rows(exp, views[k], buf)[r0 - y:r1 - y, 3 * (c0 - x):3 * (c1 - x)] = picture[r0:r1, c0:c1].reshape(r1 - r0, 3 * (c1 - c0))
    tiles = d_pic_tiles[torch.tensor(sel, device="cuda")].contiguous()
    assert lib.nhw_untile_regions_device(tiles.data_ptr(), d_table.data_ptr(), n, t, m, None) == 0
    return tiles


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4097, 65535])
def test_untile_region_finds_its_region_in_a_big_table(n):
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    rects = region_rects(n)
    counts = _region_counts(rects)
    first = _first(counts)
    fl, total = first.tolist(), int(first[-1] + counts[-1])
    buf, views = dest_views([(w, h) for _, _, w, h in rects])
    d_table = _upload(_region_table(rects, views, first))
    pic_tiles = np.random.default_rng(5).integers(0, 256, (4, 512, 512, 3), dtype=np.uint8)
    d_pic_tiles = torch.from_numpy(pic_tiles).cuda()
    picture = _join(pic_tiles, 2, 2)
    exp = np.full(buf.numel(), CANARY, np.uint8)
    keep, whole = [], set()
    for t in probe_tiles(first, counts):
        k = bisect.bisect_right(fl, t) - 1
        whole.add(k)
        for t0, m in ((t, 1), (t, 3), (fl[k], int(counts[k]))):      # the last: all tiles of the probe's region together
            keep.append(_launch_regions(lib, d_table, n, rects, fl, total, views, buf, exp, d_pic_tiles, picture, t0, m))
    torch.cuda.synchronize()
    assert {int(counts[k]) for k in whole} == {1, 2, 4}
    for k in whole:                                                  # (exp was put together tile by tile)
        x, y, w, h = rects[k]
        assert np.array_equal(_host_rows(exp, views[k], buf), picture[y:y + h, x:x + w].reshape(h, 3 * w))
    _same_bytes(buf, exp, f"{n} regions")


# ---------------------------------------------------------------- the host calls with more than 64 pictures
BYTE_LADDER = [20, 12, 4]
SSE_LADDER = [4, 12, 20]


class Crowd:
    pass


@pytest.fixture(scope="module")
def crowd():
    """73 pictures -- 70 of 1 .. 30 pixels a side (one tile each) and three of 520 x 9 (two) --, crops of generated images; their
    containers at the three rungs and the SSE of each one's decode"""
    import nhwcodec_amd as na
    c = Crowd()
    c.enc, c.dec = na.Encoder(0, max_batch=76), na.Decoder(0, max_batch=76)
    scene = na.untile_images(c.enc.synth_device(4, 2100).cpu().numpy(), 2, 2)
    rng = np.random.default_rng(61)
    c.pics = []
    for i in range(73):
        w, h = (520, 9) if i in (9, 40, 72) else (int(rng.integers(1, 31)), int(rng.integers(1, 31)))
        y, x = int(rng.integers(0, 1025 - h)), int(rng.integers(0, 1025 - w))
        c.pics.append(np.ascontiguousarray(scene[y:y + h, x:x + w]))
    assert sum(_tiles(p.shape[1], p.shape[0]) for p in c.pics) == 76
    c.cont = {q: c.enc.encode_pictures(c.pics, q) for q in BYTE_LADDER}
    c.sse = {}
    for q in BYTE_LADDER:
        c.sse[q] = []
        for pic, px in zip(c.pics, c.dec.decode_pictures(c.cont[q])):
            d = px.astype(np.int64) - pic.astype(np.int64)
            c.sse[q].append(int((d * d).sum()))
    yield c
    c.enc.close()
    c.dec.close()


@pytest.mark.gpu
def test_encode_and_decode_73_pictures(crowd):
    import nhwcodec_amd as na
    pics, conts = crowd.pics, crowd.cont[20]
    want = crowd.enc.encode(np.concatenate([pad_reference(p) for p in pics]), 20)   # the padded tiles as one ordinary batch
    files = []
    for pic, c in zip(pics, conts):
        w, h, f = parse_container(c)
        assert (w, h) == (pic.shape[1], pic.shape[0]) and len(f) == _tiles(w, h)
        files += f
    assert files == want
    bounds = np.concatenate([[0], np.cumsum([_tiles(p.shape[1], p.shape[0]) for p in pics])])
    for scale in (1, 2, 4):
        side = 512 // scale
        tiles = crowd.dec.decode(files)[0] if scale == 1 else crowd.dec.decode_scaled(files, scale)[0]
        got = crowd.dec.decode_pictures(conts) if scale == 1 else crowd.dec.decode_pictures_scaled(conts, scale)
        assert len(got) == len(pics)
        for i, (pic, g) in enumerate(zip(pics, got)):
            w, h = na.scaled_size(pic.shape[1], pic.shape[0], scale)
            assert g.shape == (h, w, 3) and np.array_equal(g, _join_crop(tiles[bounds[i]:bounds[i + 1]], w, h, side)), (scale, i)


def _spread(n, feasible):
    """answer i % 4 for picture i (0 .. 2: that rung, 3: NHW_E_BUDGET) where the first pass allows it, else rung 0"""
    return [i % 4 if feasible(i, i % 4) else 0 for i in range(n)]


@pytest.mark.gpu
def test_byte_fit_of_73_pictures_equals_73_calls(crowd):
    import nhwcodec_amd as na
    pics, enc = crowd.pics, crowd.enc
    size = [[len(crowd.cont[q][i]) for q in BYTE_LADDER] for i in range(len(pics))]
    answer = _spread(len(pics), lambda i, a: a in (0, 3) or size[i][a] < min(size[i][:a]))
    budget = [min(size[i]) - 1 if a == 3 else size[i][a] for i, a in enumerate(answer)]
    assert set(answer) == {0, 1, 2, 3}                               # every rung and NHW_E_BUDGET is some picture's answer
    want = [(crowd.cont[BYTE_LADDER[min(a, 2)]][i], BYTE_LADDER[min(a, 2)], na.NHW_E_BUDGET if a == 3 else 0) for i, a in enumerate(answer)]
    got = enc.encode_pictures_fit(pics, budget, BYTE_LADDER)
    assert got[1] == [w[1] for w in want] and got[2] == [w[2] for w in want]
    assert got[0] == [w[0] for w in want]
    for i, pic in enumerate(pics):                                   # a table of one entry never enters the search loop
        c, q, s = enc.encode_pictures_fit([pic], budget[i], BYTE_LADDER)
        assert (c[0], q[0], s[0]) == (got[0][i], got[1][i], got[2][i]), i


@pytest.mark.gpu
def test_psnr_fit_of_73_pictures_equals_73_calls(crowd):
    import nhwcodec_amd as na
    pics, enc, dec = crowd.pics, crowd.enc, crowd.dec
    sse = [[crowd.sse[q][i] for q in SSE_LADDER] for i in range(len(pics))]
    peak = [65025.0 * 3 * p.shape[0] * p.shape[1] for p in pics]
    psnr = lambda i, s: 10 * np.log10(peak[i] / s)                  # noqa: E731

    def target(i, a):
        """dB for which picture i's first passing rung is a (3: none), or None if the first pass's errors allow no such target"""
        s, w, h = sse[i], pics[i].shape[1], pics[i].shape[0]
        before = min(s[:a], default=None)                           # every earlier rung must fail: max_sse < before
        if before == 0:
            return None
        if a == 3:
            db = psnr(i, before) + 0.5
        elif s[a] == 0:
            db = 99.0 if before is None else psnr(i, before) + 0.5
        else:
            db = psnr(i, s[a]) - 0.01 if before is None else (psnr(i, s[a]) + psnr(i, before)) / 2
        m = na.picture_psnr_to_max_sse(float(db), w, h)
        return float(db) if (a == 3 or s[a] <= m) and (before is None or m < before) else None

    answer = _spread(len(pics), lambda i, a: target(i, a) is not None)
    dbs = [target(i, a) for i, a in enumerate(answer)]
    assert None not in dbs and set(answer) == {0, 1, 2, 3}
    want = [(crowd.cont[SSE_LADDER[min(a, 2)]][i], SSE_LADDER[min(a, 2)], na.NHW_E_BUDGET if a == 3 else 0, sse[i][min(a, 2)])
            for i, a in enumerate(answer)]
    got = enc.encode_pictures_fit_psnr(pics, dec, dbs, SSE_LADDER)
    assert got[1] == [w[1] for w in want] and got[2] == [w[2] for w in want] and got[3] == [w[3] for w in want]
    assert got[0] == [w[0] for w in want]
    for i, pic in enumerate(pics):
        c, q, s, e = enc.encode_pictures_fit_psnr([pic], dec, dbs[i], SSE_LADDER)
        assert (c[0], q[0], s[0], e[0]) == (got[0][i], got[1][i], got[2][i], got[3][i]), i


# ---------------------------------------------------------------- tiles nobody owns
RANGE_SPECS = [SPECS[6], SPECS[7], SPECS[2]]                         # 1023 x 1025, 1920 x 1080, 700 x 1: test_tile_pad's range case


@pytest.mark.gpu
def test_tile_pad_and_sse_crop_leave_the_tiles_nobody_owns():
    """the table starts at tile 3 and the launch covers [0, tiles + 5): 3 tiles before the table and 2 behind it"""
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    _, views = picture_views(RANGE_SPECS, seed=8)
    pics = [v.cpu().numpy() for v in views]
    ref = [pad_reference(p) for p in pics]
    counts = [len(r) for r in ref]
    tiles = sum(counts)
    assert tiles == 20
    d_table = _upload(_picture_table(views, 3 + _first(counts)))
    out = torch.full((tiles + 5, 512, 512, 3), FILL, dtype=torch.uint8, device="cuda")
    assert lib.nhw_tile_pictures_device(d_table.data_ptr(), 3, 0, tiles + 5, out.data_ptr(), None) == 0
    got = out.cpu().numpy()
    assert (got[:3] == FILL).all() and (got[3 + tiles:] == FILL).all(), "a tile no picture holds was written"
    assert np.array_equal(got[3:3 + tiles], np.concatenate(ref))
    # the error: what the call over the owned range alone adds, which is numpy's
    rand = np.random.default_rng(9).integers(0, 256, (tiles + 5, 512, 512, 3), dtype=np.uint8)
    d_rand = torch.from_numpy(rand).cuda()
    acc = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), d_table.data_ptr(), 3, 0, tiles + 5, acc[0].data_ptr(), None) == 0
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr() + 3 * na.IMG_BYTES, d_table.data_ptr(), 3, 3, tiles, acc[1].data_ptr(), None) == 0
    bounds = 3 + np.concatenate([[0], np.cumsum(counts)])
    want = [np_picture_sse(rand[bounds[k]:bounds[k + 1]], p) for k, p in enumerate(pics)]
    assert acc.cpu().tolist() == [want, want]


@pytest.mark.gpu
@pytest.mark.parametrize("side", [512, 256, 128])
def test_untile_crop_leaves_the_tiles_nobody_owns(side):
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    buf, views = picture_views(RANGE_SPECS, seed=10)
    buf.fill_(CANARY)
    counts = [_tiles(w, h, side) for w, h, *_ in RANGE_SPECS]
    tiles = sum(counts)
    d_table = _upload(_picture_table(views, 3 + _first(counts)))
    rand = np.random.default_rng(11).integers(0, 256, (tiles + 5, side, side, 3), dtype=np.uint8)
    d_rand = torch.from_numpy(rand).cuda()
    assert _untile(lib, side, d_rand.data_ptr(), d_table.data_ptr(), 3, 0, tiles + 5) == 0
    exp = np.full(buf.numel(), CANARY, np.uint8)
    at = 3
    for v, c, (w, h, *_) in zip(views, counts, RANGE_SPECS):
        _host_rows(exp, v, buf)[:] = _join_crop(rand[at:at + c], w, h, side).reshape(h, 3 * w)
        at += c
    _same_bytes(buf, exp, f"tiles of {side}")


@pytest.mark.gpu
def test_untile_region_leaves_the_tiles_nobody_owns():
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    rects = [(511, 511, 2, 2), (5, 7, 8, 8), (511, 100, 2, 3), (1000, 1016, 24, 8)]
    counts = _region_counts(rects)
    assert counts.tolist() == [4, 1, 2, 1]
    first = 3 + _first(counts)
    fl, total = first.tolist(), int(first[-1] + counts[-1])
    buf, views = dest_views([(w, h) for _, _, w, h in rects])
    d_table = _upload(_region_table(rects, views, first))
    pic_tiles = np.random.default_rng(12).integers(0, 256, (4, 512, 512, 3), dtype=np.uint8)
    d_pic_tiles = torch.from_numpy(pic_tiles).cuda()
    picture = _join(pic_tiles, 2, 2)
    exp = np.full(buf.numel(), CANARY, np.uint8)
    keep = _launch_regions(lib, d_table, 4, rects, fl, total, views, buf, exp, d_pic_tiles, picture, 0, total + 2)
    torch.cuda.synchronize()
    for (x, y, w, h), v in zip(rects, views):
        assert np.array_equal(_host_rows(exp, v, buf), picture[y:y + h, x:x + w].reshape(h, 3 * w))
    _same_bytes(buf, exp, "regions from tile 3 on")
    del keep


EMPTY_SPECS = [(30, 20, 5, 1), (17, 9, 0, 2), (17, 9, 0, 2), (520, 4, 3, 3)]      # the second stands for the empty entry


@pytest.mark.gpu
@pytest.mark.parametrize("zero", ["width", "height"])
def test_an_empty_picture_entry_is_passed_over(zero):
    """entry 1 has a zero side and its successor's first tile: the successor is served, the empty entry writes and adds nothing"""
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    first = [0, 1, 1, 2]
    _, src = picture_views(EMPTY_SPECS, seed=13)
    table = _picture_table(src, first)
    table[zero][1] = 0
    d_table = _upload(table)
    real = [0, 2, 3]
    ref = np.concatenate([pad_reference(src[k].cpu().numpy()) for k in real])
    out = torch.full((4, 512, 512, 3), FILL, dtype=torch.uint8, device="cuda")
    assert lib.nhw_tile_pictures_device(d_table.data_ptr(), 4, 0, 4, out.data_ptr(), None) == 0
    assert np.array_equal(out.cpu().numpy(), ref)
    # the error
    rand = np.random.default_rng(14).integers(0, 256, (4, 512, 512, 3), dtype=np.uint8)
    d_rand = torch.from_numpy(rand).cuda()
    acc = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), d_table.data_ptr(), 4, 0, 4, acc.data_ptr(), None) == 0
    want = [np_picture_sse(rand[0:1], src[0].cpu().numpy()), 0, np_picture_sse(rand[1:2], src[2].cpu().numpy()),
            np_picture_sse(rand[2:4], src[3].cpu().numpy())]
    assert acc.cpu().tolist() == want and min(want[0], want[2], want[3]) > 0
    # the inverse, the empty entry's address inside the canary
    buf, dst = picture_views(EMPTY_SPECS, seed=15)
    buf.fill_(CANARY)
    table = _picture_table(dst, first)
    table[zero][1] = 0
    d_table = _upload(table)
    assert lib.nhw_untile_pictures_device(d_rand.data_ptr(), d_table.data_ptr(), 4, 0, 4, None) == 0
    exp = np.full(buf.numel(), CANARY, np.uint8)
    for k, (a, b) in zip(real, ((0, 1), (1, 2), (2, 4))):
        w, h = EMPTY_SPECS[k][:2]
        _host_rows(exp, dst[k], buf)[:] = _join_crop(rand[a:b], w, h).reshape(h, 3 * w)
    _same_bytes(buf, exp, f"an entry of {zero} 0")


@pytest.mark.gpu
def test_an_empty_region_entry_is_passed_over():
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    rects = [(5, 7, 8, 8), (100, 100, 6, 3), (100, 100, 6, 3), (511, 100, 2, 3)]
    first = [0, 1, 1, 2]
    buf, views = dest_views([(w, h) for _, _, w, h in rects])
    table = _region_table(rects, views, first)
    table["width"][1] = 0
    d_table = _upload(table)
    pic_tiles = np.random.default_rng(16).integers(0, 256, (4, 512, 512, 3), dtype=np.uint8)
    picture = _join(pic_tiles, 2, 2)
    d_tiles = torch.from_numpy(pic_tiles[[0, 0, 0, 1]]).cuda()       # the running selection: tile 0, tile 0, tiles 0 and 1
    assert lib.nhw_untile_regions_device(d_tiles.data_ptr(), d_table.data_ptr(), 4, 0, 4, None) == 0
    exp = np.full(buf.numel(), CANARY, np.uint8)
    for k in (0, 2, 3):
        x, y, w, h = rects[k]
        _host_rows(exp, views[k], buf)[:] = picture[y:y + h, x:x + w].reshape(h, 3 * w)
    _same_bytes(buf, exp, "a region of width 0")


# ---------------------------------------------------------------- sides of 65535
@pytest.mark.gpu
@pytest.mark.parametrize("spec", [(65535, 1, 0, 0), (1, 65535, 0, 0), (65535, 3, 5, 3)], ids=["65535x1", "1x65535", "65535x3"])
def test_sides_of_65535(spec):
    """128 tiles a picture: tx = 127 on the edge path (3 W = 196605 ends 3 bytes before the tile column does), ty = 127 with 511 replicated
    rows.  The error's tiles are random in 200 .. 255 against a picture random in 0 .. 31, which keeps even the 196605-byte pictures' sums
    above 2^32 (uniform bytes on both sides would give about 2^31)."""
    import nhwcodec_amd as na
    import torch
    w, h = spec[:2]
    rng = np.random.default_rng(17)
    _, (src,) = picture_views([spec], seed=18)
    pic = src.cpu().numpy()
    tiles = na.tile_pictures_device([src])
    want = torch.from_numpy(pad_reference(pic)).cuda()
    assert tiles.shape == want.shape == (128, 512, 512, 3)
    assert torch.equal(tiles, want), [t for t in range(128) if not torch.equal(tiles[t], want[t])]
    del want
    # back into a canary copy of the layout
    buf, (dst,) = picture_views([spec], seed=19)
    buf.fill_(CANARY)
    na.untile_pictures_device(tiles, [dst])
    exp = np.full(buf.numel(), CANARY, np.uint8)
    _host_rows(exp, dst, buf)[:] = pic.reshape(h, 3 * w)
    _same_bytes(buf, exp, "untile")
    del tiles
    # the error
    low = rng.integers(0, 32, pic.shape, dtype=np.uint8)
    src.copy_(torch.from_numpy(low).cuda())
    rand = rng.integers(200, 256, (128, 512, 512, 3), dtype=np.uint8)
    sse = np_picture_sse(rand, low)
    assert sse > 2**32
    assert na.sse_pictures_device(torch.from_numpy(rand).cuda(), [src]).cpu().tolist() == [sse]
    del rand
    # the tiles of a scaled decode into the scaled picture
    for scale in (2, 4):
        side = 512 // scale
        ws, hs = na.scaled_size(w, h, scale)
        assert _tiles(ws, hs, side) == 128
        buf, (dst,) = picture_views([(ws, hs, spec[2], spec[3])], seed=20)
        buf.fill_(CANARY)
        rand = rng.integers(0, 256, (128, side, side, 3), dtype=np.uint8)
        na.untile_scaled_pictures_device(torch.from_numpy(rand).cuda(), [dst], scale)
        exp = np.full(buf.numel(), CANARY, np.uint8)
        _host_rows(exp, dst, buf)[:] = _join_crop(rand, ws, hs, side).reshape(hs, 3 * ws)
        _same_bytes(buf, exp, f"scale {scale}")


# ---------------------------------------------------------------- row offsets past 2^32
@pytest.mark.gpu
def test_row_offsets_past_4_gib():
    """a 5 x 33 picture (two bands) of pitch 2^27 + 5 in an uninitialised buffer of 4.43 GB, the smallest in which a row can start more
    than 2^32 bytes behind the first: row 32 does, by 160 bytes.  A row offset computed in 32 bits lands on another row inside the buffer,
    so it shows as a wrong value, not as a fault."""
    import nhwcodec_amd as na
    import torch
    lib = na._library()
    pitch, w, h = 2**27 + 5, 5, 33
    assert 32 * pitch == 4294967456 > 2**32
    try:
        big = torch.empty(33 * pitch + 64, dtype=torch.uint8, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no 4.43 GB of device memory free for the buffer")
    pic_at, reg_at = 17, 64 + 3                                      # misalignments 1 and 3; 16 bytes of guard before the first row
    view = big.as_strided((h, w, 3), (pitch, 3, 1), pic_at)
    guard = big.as_strided((h, 3 * w + 32), (pitch, 1), pic_at - 16)
    rng = np.random.default_rng(22)
    pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    view.copy_(torch.from_numpy(pic).cuda())
    assert np.array_equal(view.cpu().numpy(), pic)
    d_table = _upload(_picture_table([view], [0]))
    # pad
    out = torch.full((1, 512, 512, 3), FILL, dtype=torch.uint8, device="cuda")
    assert lib.nhw_tile_pictures_device(d_table.data_ptr(), 1, 0, 1, out.data_ptr(), None) == 0
    assert np.array_equal(out.cpu().numpy(), pad_reference(pic))
    # the error
    rand = rng.integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
    d_rand = torch.from_numpy(rand).cuda()
    acc = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), d_table.data_ptr(), 1, 0, 1, acc.data_ptr(), None) == 0
    assert acc.cpu().tolist() == [np_picture_sse(rand, pic)]
    # untile: the picture's rows, and the 16 bytes on either side of each as they were
    around = rng.integers(0, 256, (h, 3 * w + 32), dtype=np.uint8)
    around[:, 16:16 + 3 * w] = CANARY
    guard.copy_(torch.from_numpy(around).cuda())
    assert lib.nhw_untile_pictures_device(d_rand.data_ptr(), d_table.data_ptr(), 1, 0, 1, None) == 0
    around[:, 16:16 + 3 * w] = rand[0, :h, :w].reshape(h, 3 * w)
    assert np.array_equal(guard.cpu().numpy(), around)
    # regions whose destinations have that pitch: rows 30 .. 32 of the tile, and all 33, whose last row lies past 2^32
    for x, y, rw, rh in ((1, 30, 3, 3), (1, 0, 3, 33)):
        dest = big.as_strided((rh, 3 * rw + 32), (pitch, 1), reg_at - 16)
        around = rng.integers(0, 256, (rh, 3 * rw + 32), dtype=np.uint8)
        around[:, 16:16 + 3 * rw] = CANARY
        dest.copy_(torch.from_numpy(around).cuda())
        table = np.zeros(1, na.REGION_DTYPE)
        table[0] = (big.data_ptr() + reg_at, pitch, x, y, rw, rh, w, h, 0, 0)
        d_regs = _upload(table)
        assert lib.nhw_untile_regions_device(d_rand.data_ptr(), d_regs.data_ptr(), 1, 0, 1, None) == 0
        around[:, 16:16 + 3 * rw] = rand[0, y:y + rh, x:x + rw].reshape(rh, 3 * rw)
        assert np.array_equal(dest.cpu().numpy(), around), (x, y, rw, rh)
