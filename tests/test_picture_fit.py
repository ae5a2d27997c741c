"""Pictures of any size to a byte budget or a PSNR target: the picture-cropped error k_sse_crop
(nhw_sse_pictures_device, sse_pictures_device), the walks nhw_enc_fit_pictures / nhw_enc_fit_sse_pictures and their Python wrappers
Encoder.encode_pictures_fit / encode_pictures_fit_psnr, and picture_psnr_to_max_sse.  A picture's result must be the container of the first
ladder rung that passes its test, byte-identical to encode_pictures at that quality; brute force over every quality is the yardstick."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests.picture_cases import np_picture_sse, pad_reference, padding_mask, parse_container, picture_views
from tests.support import ROOT, load_lib

UINT64_MAX = 2**64 - 1
NEW_SYMBOLS = ("nhw_sse_pictures_device", "nhw_enc_fit_pictures", "nhw_enc_fit_sse_pictures")
DEFAULT_BYTES = list(range(23, 0, -1))
DEFAULT_SSE = list(range(1, 24))
LADDERS = {"default": None, "short": [20, 15, 10, 5], "one": [17], "non_monotone": [5, 22, 9, 17, 1]}


# ---------------------------------------------------------------- without a GPU
def test_picture_fit_symbols_and_prototypes():
    import nhwcodec_amd as na
    lib = load_lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    hdr = " ".join(open(os.path.join(ROOT, "include", "nhw_hip.h")).read().split())
    assert ("int nhw_sse_pictures_device(const void *d_tiles, const nhw_picture *d_pics, int n_pics, int tile0, int m, uint64_t *d_sse, "
            "void *stream);") in hdr
    assert ("int nhw_enc_fit_pictures(nhw_enc *e, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, const uint32_t *height, "
            "int n, const uint64_t *max_bytes, const int *ladder, int ladder_len, uint8_t *out_arena, size_t arena_cap, uint64_t *out_off, "
            "int32_t *status, int32_t *quality);") in hdr
    assert ("int nhw_enc_fit_sse_pictures(nhw_enc *e, nhw_dec *d, const uint8_t *bgr, const uint64_t *in_off, const uint32_t *width, "
            "const uint32_t *height, int n, const uint64_t *max_sse, const int *ladder, int ladder_len, uint8_t *out_arena, size_t arena_cap, "
            "uint64_t *out_off, int32_t *status, int32_t *quality, uint64_t *sse);") in hdr
    for name in ("sse_pictures_device", "picture_psnr_to_max_sse"):
        assert callable(getattr(na, name))
    for name in ("encode_pictures_fit", "encode_pictures_fit_psnr"):
        assert callable(getattr(na.Encoder, name))


@pytest.mark.parametrize("w,h", [(1, 1), (500, 375), (513, 700), (1100, 530), (1920, 1080), (65535, 65535), (65535, 1)])
def test_picture_psnr_to_max_sse_formula(w, h):
    import nhwcodec_amd as na
    dbs = [0.5, 10.0, 28.25, 30.0, 38.0, 48.13, 100.0]
    got = [na.picture_psnr_to_max_sse(db, w, h) for db in dbs]
    assert got == [math.floor(65025.0 * 3 * w * h * 10 ** (-db / 10)) for db in dbs]
    assert all(isinstance(g, int) for g in got)
    assert all(a >= b for a, b in zip(got, got[1:]))
    arr = na.picture_psnr_to_max_sse(np.array(dbs), w, h)
    assert arr.dtype == np.int64 and arr.tolist() == got


def test_picture_psnr_to_max_sse_agrees_at_512():
    import nhwcodec_amd as na
    for db in [0.1, 1.0, 20.0, 30.0, 33.3, 36.23, 40.0, 60.0, 99.9]:
        assert na.picture_psnr_to_max_sse(db, 512, 512) == na.psnr_to_max_sse(db)
    assert 65025 * 3 * 65535 * 65535 < 2**53


@pytest.mark.parametrize("db,w,h", [(0, 10, 10), (-1.0, 10, 10), (float("nan"), 10, 10), (float("inf"), 10, 10), ("x", 10, 10), ([], 10, 10),
                                    (30.0, 0, 10), (30.0, 10, 0), (30.0, 65536, 1), (30.0, 1, 65536), (30.0, 1.5, 10)])
def test_picture_psnr_to_max_sse_refusals(db, w, h):
    import nhwcodec_amd as na
    with pytest.raises(na.NhwError):
        na.picture_psnr_to_max_sse(db, w, h)


# ---------------------------------------------------------------- on the MI355X: the error kernel
SSE_SPECS = ([(1, 1, 0, 0), (1, 700, 0, 1), (700, 1, 5, 3), (511, 513, 0, 2), (513, 511, 16, 1), (512, 512, 0, 0), (1023, 1025, 7, 0),
              (1100, 530, 0, 1), (1100, 530, 3, 2)]
             + [(149 + 11 * r, 3 + r, 9 if r % 2 else 0, r % 4) for r in range(16)])          # 3W mod 16 takes every residue, every alignment


@pytest.mark.gpu
def test_sse_pictures_device_matches_numpy():
    import nhwcodec_amd as na
    import torch
    assert sorted({(3 * w) % 16 for w, *_ in SSE_SPECS}) == list(range(16))
    buf, views = picture_views(SSE_SPECS, seed=5)
    pics = [v.cpu().numpy() for v in views]
    counts = [na.picture_tiles(p.shape[1], p.shape[0]) for p in pics]
    bounds = np.concatenate([[0], np.cumsum(counts)])
    # tiles that differ from the padded input only in the padding: SSE 0
    rng = np.random.default_rng(6)
    padded = na.tile_pictures_device(views).cpu().numpy()
    noisy = padded.copy()
    for k, p in enumerate(pics):
        m = padding_mask(p.shape)
        part = noisy[bounds[k]:bounds[k + 1]]
        part[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)
    assert (noisy != padded).any()
    got = na.sse_pictures_device(torch.from_numpy(noisy).cuda(), views)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.cpu().tolist() == [0] * len(views)
    # random tiles: the numpy SSE over each crop
    rand = rng.integers(0, 256, padded.shape, dtype=np.uint8)
    want = [np_picture_sse(rand[bounds[k]:bounds[k + 1]], p) for k, p in enumerate(pics)]
    assert max(want) > 2**32                                          # beyond 32 bits: the 64-bit sums are needed
    d_rand = torch.from_numpy(rand).cuda()
    got = na.sse_pictures_device(d_rand, views)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == want
    # chunks: [0, k) and [k, m) add up to one call over [0, m), k inside a picture
    table, tiles, dev = na._picture_table(views, "test")
    lib = na._library()
    n = len(views)
    for k in (1, 5, int(bounds[8]) + 1, tiles - 1):
        acc = torch.zeros(n, dtype=torch.int64, device=dev)
        assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), n, 0, k, acc.data_ptr(), None) == 0
        assert lib.nhw_sse_pictures_device(d_rand.data_ptr() + k * na.IMG_BYTES, table.data_ptr(), n, k, tiles - k, acc.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert acc.cpu().tolist() == want, k
    # one graph-captured call
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), n, 0, tiles, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream) == 0
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == want
    # what the host can check is refused
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), n, 0, tiles, out.data_ptr() + 4, None) == na.NHW_E_ARG
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), n, 0, tiles, None, None) == na.NHW_E_ARG
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr() + 8, table.data_ptr(), n, 0, tiles, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), 0, 0, tiles, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), n, -1, tiles, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_sse_pictures_device(d_rand.data_ptr(), table.data_ptr(), n, 0, 0, out.data_ptr(), None) == na.NHW_E_ARG
    with pytest.raises(na.NhwError):
        na.sse_pictures_device(d_rand[:-1], views)
    del buf


# ---------------------------------------------------------------- on the MI355X: the walks against a brute force
def _fit_pictures(oracle):
    """1 x 1, 500 x 375, 513 x 700 (4 tiles), 1100 x 530 (6 tiles) crops of the generator's images, and a 1024 x 512 picture whose left
    tile is make(50431), which overflows the code book from q17 up"""
    import nhwcodec_amd as na
    from gpu_fuzz_classes import make
    big = na.untile_images(np.stack([oracle.synth(700 + t) for t in range(6)]), 2, 3)
    return [big[100:101, 200:201].copy(), big[37:412, 5:505].copy(), big[200:900, 600:1113].copy(), big[300:830, 200:1300].copy(),
            np.ascontiguousarray(np.concatenate([make(50431), oracle.synth(777)], axis=1))]


def _raw_encode_pictures(enc, pics, q):
    """nhw_enc_pictures with the per-picture status (encode_pictures raises on a failed picture) -> (containers, status)"""
    n, blob, in_off, width, height, _, arena = enc._host_pictures(pics, "test")
    offs = np.empty(n + 1, np.uint64)
    status = np.empty(n, np.int32)
    assert enc.lib.nhw_enc_pictures(enc.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n, q, arena.ctypes.data,
                                    arena.size, offs.ctypes.data, status.ctypes.data) == 0
    return [arena[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)], status.tolist()


def _sse_fit_raw(enc, dec, pics, max_sse, ladder):
    """nhw_enc_fit_sse_pictures with exact SSE targets -> (containers, qualities, status, sse)"""
    n, blob, in_off, width, height, _, arena = enc._host_pictures(pics, "test")
    target = np.array(max_sse, np.uint64)
    offs = np.empty(n + 1, np.uint64)
    status = np.empty(n, np.int32)
    quality = np.empty(n, np.int32)
    sse = np.empty(n, np.uint64)
    lad, lad_n = enc._ladder(ladder)
    enc._chk(enc.lib.nhw_enc_fit_sse_pictures(enc.h, dec.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n,
                                              target.ctypes.data, lad, lad_n, arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data,
                                              quality.ctypes.data, sse.ctypes.data))
    return [arena[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)], quality.tolist(), status.tolist(), [int(x) for x in sse]


@pytest.fixture(scope="module")
def brute(oracle):
    """every quality's containers and statuses (nhw_enc_pictures), and the SSE of every successful one's decode over the picture"""
    import nhwcodec_amd as na
    pics = _fit_pictures(oracle)
    enc = na.Encoder(0, max_batch=64)
    dec = na.Decoder(0, max_batch=64)
    cont, stat, sse = {}, {}, {}
    for q in range(1, 24):
        cont[q], stat[q] = _raw_encode_pictures(enc, pics, q)
        ok = [i for i in range(len(pics)) if stat[q][i] == 0]
        sse[q] = [UINT64_MAX] * len(pics)
        for i, px in zip(ok, dec.decode_pictures([cont[q][i] for i in ok])):
            d = px.astype(np.int64) - pics[i].astype(np.int64)
            sse[q][i] = int((d * d).sum())
    assert all(stat[q][4] == na.NHW_E_CODEBOOK for q in range(17, 24)) and all(stat[q][4] == 0 for q in range(1, 17))
    assert all(s == 0 for q in range(1, 24) for s in stat[q][:4])
    yield pics, enc, dec, cont, stat, sse
    enc.close()
    dec.close()


def _expect(brute, ladder, passes):
    """the first rung of `ladder` at which picture i passes (passes(q, i)), else the last rung with its failure -> (container, q, status) lists"""
    import nhwcodec_amd as na
    pics, _, _, cont, stat, _ = brute
    out = []
    for i in range(len(pics)):
        for q in ladder:
            if stat[q][i] == 0 and passes(q, i):
                out.append((cont[q][i], q, 0))
                break
        else:
            q = ladder[-1]
            out.append((b"", q, na.NHW_E_CODEBOOK) if stat[q][i] else (cont[q][i], q, na.NHW_E_BUDGET))
    return out


def _byte_budgets(brute, ladder, shift):
    """per picture one of: exactly the container size at a rung, that size - 1, one below every rung's size, a generous budget"""
    pics, _, _, cont, stat, _ = brute
    out = []
    for i in range(len(pics)):
        sizes = [len(cont[q][i]) for q in ladder if stat[q][i] == 0] or [10]
        mid = sizes[len(sizes) // 2]
        out.append([mid, mid - 1, min(sizes) - 1, 1 << 40][(i + shift) % 4])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ladder_name", sorted(LADDERS))
def test_byte_fit_equals_the_brute_force(brute, ladder_name):
    pics, enc, _, cont, _, _ = brute
    ladder = LADDERS[ladder_name]
    lad = ladder or DEFAULT_BYTES
    for shift in range(4):
        budgets = _byte_budgets(brute, lad, shift)
        want = _expect(brute, lad, lambda q, i: len(cont[q][i]) <= budgets[i])
        got = enc.encode_pictures_fit(pics, budgets, ladder)
        assert got[1] == [w[1] for w in want] and got[2] == [w[2] for w in want], (shift, budgets)
        assert got[0] == [w[0] for w in want], shift
        for c, (w, h) in zip(got[0], [(p.shape[1], p.shape[0]) for p in pics]):
            assert not c or parse_container(c)[:2] == (w, h)
    # one budget for all, the container size as the user stores it (16 + 4 T + the tile lengths)
    got = enc.encode_pictures_fit(pics, 1 << 40, ladder)
    assert got[1] == [next(q for q in lad if brute[4][q][i] == 0) if any(brute[4][q][i] == 0 for q in lad) else lad[-1] for i in range(len(pics))]


def _sse_targets(brute, ladder, shift):
    """per picture one of: exactly the SSE at a rung, that SSE - 1, one below every rung's SSE, a generous target"""
    pics, _, _, _, stat, sse = brute
    out = []
    for i in range(len(pics)):
        vals = [sse[q][i] for q in ladder if stat[q][i] == 0] or [10]
        mid = vals[len(vals) // 2]
        out.append(max(0, [mid, mid - 1, min(vals) - 1, 1 << 60][(i + shift) % 4]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ladder_name", sorted(LADDERS))
def test_psnr_fit_equals_the_brute_force(brute, ladder_name):
    import nhwcodec_amd as na
    pics, enc, dec, _, _, sse = brute
    ladder = LADDERS[ladder_name]
    lad = ladder or DEFAULT_SSE
    for shift in range(4):
        targets = _sse_targets(brute, lad, shift)
        want = _expect(brute, lad, lambda q, i: sse[q][i] <= targets[i])
        got = _sse_fit_raw(enc, dec, pics, targets, ladder)
        assert got[1] == [w[1] for w in want] and got[2] == [w[2] for w in want], (shift, targets)
        assert got[0] == [w[0] for w in want], shift
        assert got[3] == [sse[w[1]][i] if w[2] != na.NHW_E_CODEBOOK else UINT64_MAX for i, w in enumerate(want)]
        assert na.NHW_E_FORMAT not in got[2]
        ok = [i for i in range(len(pics)) if got[2][i] != na.NHW_E_CODEBOOK]
        for i, px in zip(ok, dec.decode_pictures([got[0][i] for i in ok])):      # the returned SSE is the one a user measures
            d = px.astype(np.int64) - pics[i].astype(np.int64)
            assert int((d * d).sum()) == got[3][i]
    # the Python wrapper with dB targets, one number and one per picture
    for db in (30.0, [25.0, 31.5, 36.0, 28.0, 40.0]):
        dbs = [db] * len(pics) if isinstance(db, float) else db
        targets = [na.picture_psnr_to_max_sse(x, p.shape[1], p.shape[0]) for x, p in zip(dbs, pics)]
        assert enc.encode_pictures_fit_psnr(pics, dec, db, ladder) == _sse_fit_raw(enc, dec, pics, targets, ladder)


@pytest.mark.gpu
def test_codebook_picture_passes_over_its_overflowing_rungs(brute):
    import nhwcodec_amd as na
    pics, enc, dec, cont, _, sse = brute
    c, q, s = enc.encode_pictures_fit(pics[4:], 1 << 40)                  # bytes: 23, 22, ... overflow down to q17
    assert (q, s) == ([16], [0]) and c == [cont[16][4]]
    c, q, s = enc.encode_pictures_fit(pics[4:], 1 << 40, [23, 20, 17])
    assert (c, q, s) == ([b""], [17], [na.NHW_E_CODEBOOK])
    c, q, s, e = _sse_fit_raw(enc, dec, pics[4:], [0], [15, 16, 17, 18])    # SSE: nothing reaches 0, the last rung overflows
    assert (c, q, s, e) == ([b""], [18], [na.NHW_E_CODEBOOK], [UINT64_MAX])
    c, q, s, e = _sse_fit_raw(enc, dec, pics[4:], [sse[16][4]], [20, 17, 16, 1])
    assert (c, q, s, e) == ([cont[16][4]], [16], [0], [sse[16][4]])


@pytest.mark.gpu
def test_chunked_walks_equal_one_chunk(brute):
    """handles of max_batch 4: the 6-tile and 4-tile pictures straddle chunk boundaries"""
    import nhwcodec_amd as na
    pics, enc, dec, _, _, sse = brute
    e4, d4 = na.Encoder(0, max_batch=4), na.Decoder(0, max_batch=4)
    lad = [20, 15, 10, 5, 1]
    budgets = _byte_budgets(brute, lad, 1)
    assert e4.encode_pictures_fit(pics, budgets, lad) == enc.encode_pictures_fit(pics, budgets, lad)
    lad = [3, 8, 13, 18, 23]
    targets = _sse_targets(brute, lad, 2)
    assert _sse_fit_raw(e4, d4, pics, targets, lad) == _sse_fit_raw(enc, dec, pics, targets, lad)
    e4.close(); d4.close()


@pytest.mark.gpu
def test_chosen_containers_hold_the_oracles_tiles(brute, oracle):
    pics, enc, dec, cont, _, sse = brute
    sel = [pics[1], pics[3]]
    c, q, s = enc.encode_pictures_fit(sel, [len(cont[14][1]), len(cont[14][3])], [22, 18, 14, 10, 6])
    c2, q2, s2, _ = _sse_fit_raw(enc, dec, sel, [sse[14][1], sse[14][3]], [6, 10, 14, 18, 22])
    for conts, quals, stats in ((c, q, s), (c2, q2, s2)):
        assert stats == [0, 0]
        for pic, cont, qq in zip(sel, conts, quals):
            w, h, files = parse_container(cont)
            assert (w, h) == (pic.shape[1], pic.shape[0])
            for t, (f, tile) in enumerate(zip(files, pad_reference(pic))):
                assert f == oracle.encode(tile, qq), (pic.shape, qq, t)


@pytest.mark.gpu
def test_fit_stats_count_the_open_tiles(brute):
    import nhwcodec_amd as na
    pics, enc, dec, cont, stat, sse = brute
    tiles = [na.picture_tiles(p.shape[1], p.shape[0]) for p in pics]
    cases = [(False, [20, 15, 10, 5], _byte_budgets(brute, [20, 15, 10, 5], 0)), (False, None, _byte_budgets(brute, DEFAULT_BYTES, 2)),
             (True, [5, 10, 15, 20], _sse_targets(brute, [5, 10, 15, 20], 3)), (True, [9, 22, 3], [1 << 60] * len(pics))]
    for by_sse, ladder, lim in cases:
        lad = ladder or DEFAULT_BYTES
        if by_sse:
            _sse_fit_raw(enc, dec, pics, lim, ladder)
        else:
            enc.encode_pictures_fit(pics, lim, ladder)
        st = enc.fit_stats()
        open_, counts = list(range(len(pics))), []
        for q in lad:
            if not open_:
                break
            counts.append(sum(tiles[i] for i in open_))
            open_ = [i for i in open_ if not (stat[q][i] == 0 and (sse[q][i] if by_sse else len(cont[q][i])) <= lim[i])]
        assert st.rungs == len(counts) and list(st.images[:st.rungs]) == counts and list(st.quality[:st.rungs]) == lad[:st.rungs]
        assert st.total_ms > 0
    assert st.rungs == 1


@pytest.mark.gpu
def test_refusals_come_before_any_launch(brute):
    import nhwcodec_amd as na
    pics = brute[0][:2]
    e = na.Encoder(0, max_batch=8)
    d, d1 = na.Decoder(0, max_batch=8), na.Decoder(0, max_batch=1)
    L = e.lib
    n, blob, in_off, width, height, tiles, arena = e._host_pictures(pics, "test")
    assert tiles == 2
    lim = np.full(n, 1 << 40, np.uint64)
    offs = np.empty(n + 1, np.uint64)
    st = np.empty(n, np.int32)
    qu = np.empty(n, np.int32)
    ss = np.empty(n, np.uint64)
    bad_w = width.copy(); bad_w[1] = 0
    big_w = width.copy(); big_w[0] = 65536
    P = lambda a: a.ctypes.data                                          # noqa: E731

    def fit(enc=e.h, bgr=P(blob), w=P(width), nn=n, lad=None, lad_n=0, out=P(arena), o=P(offs), limit=P(lim), q=P(qu)):
        return L.nhw_enc_fit_pictures(enc, bgr, P(in_off), w, P(height), nn, limit, lad, lad_n, out, arena.size, o, P(st), q)

    def fit_sse(dec=d.h, enc=e.h, bgr=P(blob), w=P(width), nn=n, lad=None, lad_n=0, s=P(ss)):
        return L.nhw_enc_fit_sse_pictures(enc, dec, bgr, P(in_off), w, P(height), nn, P(lim), lad, lad_n, P(arena), arena.size, P(offs), P(st),
                                          P(qu), s)

    dup = (ctypes.c_int * 2)(20, 20)
    out_of_range = (ctypes.c_int * 2)(20, 24)
    ok_lad = (ctypes.c_int * 2)(20, 10)
    arg = [fit(enc=None), fit(bgr=None), fit(w=None), fit(nn=0), fit(out=None), fit(o=None), fit(limit=None), fit(q=None), fit(w=P(bad_w)),
           fit(w=P(big_w)), fit(lad=ok_lad, lad_n=0), fit(lad=None, lad_n=2), fit(lad=ok_lad, lad_n=24),
           fit_sse(dec=None), fit_sse(s=None), fit_sse(dec=d1.h), fit_sse(nn=0), fit_sse(w=P(bad_w)), fit_sse(lad=ok_lad, lad_n=-1)]
    assert arg == [na.NHW_E_ARG] * len(arg)
    assert [fit(lad=dup, lad_n=2), fit(lad=out_of_range, lad_n=2), fit_sse(lad=dup, lad_n=2)] == [na.NHW_E_QUALITY] * 3
    L.nhw_debug_stop_after.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.nhw_debug_stop_after(e.h, 3)
    assert fit() == na.NHW_E_ARG and fit_sse() == na.NHW_E_ARG
    L.nhw_debug_stop_after(e.h, 0)
    d.lib.nhw_dec_debug_stop_after(d.h, 2)
    assert fit_sse() == na.NHW_E_ARG
    d.lib.nhw_dec_debug_stop_after(d.h, 0)
    assert L.nhw_enc_last_fit_stats(e.h, ctypes.byref(na.FitStats())) == na.NHW_E_ARG        # nothing has run
    # a short arena: NHW_E_SPACE
    assert L.nhw_enc_fit_pictures(e.h, P(blob), P(in_off), P(width), P(height), n, P(lim), None, 0, P(arena), 100, P(offs), P(st), P(qu)) == na.NHW_E_SPACE
    # the decoder needs min(max_batch, tiles): one of 2 suffices for one single-tile picture, and a decoder of max_batch 1 for 2 tiles does not
    assert fit_sse(dec=d1.h, nn=1) == 0 and st[0] == 0
    with pytest.raises(na.NhwError):
        e.encode_pictures_fit_psnr(pics, d1, 30.0)
    with pytest.raises(na.NhwError):
        e.encode_pictures_fit(pics, [-1, 5])
    with pytest.raises(na.NhwError):
        e.encode_pictures_fit(pics, [5])
    with pytest.raises(na.NhwError):
        e.encode_pictures_fit_psnr(pics, d, [30.0])
    with pytest.raises(na.NhwError):
        e.encode_pictures_fit_psnr(pics, d, float("nan"))
    e.close(); d.close(); d1.close()

