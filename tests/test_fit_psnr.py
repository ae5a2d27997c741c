"""Encode to a PSNR target (nhw_sse_batch_device, nhw_enc_fit_sse_batch_device / nhw_enc_fit_sse_batch, sse_device, Encoder.encode_fit_psnr*,
nhw-enc --min-psnr): for every image the file of the first ladder rung whose encode succeeds and whose device decode is within the image's
SSE target, identical to the fixed-quality encode at that quality."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests.support import CLI, ROOT, built_cli, load_lib, run, same_files

PEAK = 65025 * 786432
UINT64_MAX = 2**64 - 1
LADDERS = {"default": None, "q17_23": list(range(17, 24)), "descending": [23, 20, 17], "q20": [20]}


@pytest.fixture(scope="module")
def cli():
    return built_cli("nhw-enc")


def _np_sse(a, b):
    """exact per-picture SSE in int64 of two uint8 arrays [n, 512, 512, 3] (or one picture each)"""
    d = a.astype(np.int32) - b.astype(np.int32)
    return (d * d).reshape(-1 if a.ndim == 4 else 1, 786432).sum(axis=1, dtype=np.int64)


# ---------------------------------------------------------------- without a GPU
def test_library_exports_the_psnr_entry_points():
    lib = load_lib()
    for name in ("nhw_sse_batch_device", "nhw_enc_fit_sse_batch_device", "nhw_enc_fit_sse_batch"):
        assert hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "nhw_hip.h")).read()
    assert "NHW_E_BUDGET = -7" in hdr and "byte or distortion budget" in hdr


def test_psnr_to_max_sse_formula_and_refusals():
    import nhwcodec_amd as na
    dbs = [0.5, 1.0, 10.0, 20.0, 28.25, 30.0, 33.3, 40.0, 48.13, 60.0, 100.0]
    got = [na.psnr_to_max_sse(db) for db in dbs]
    assert got == [math.floor(65025.0 * 786432.0 * 10 ** (-db / 10)) for db in dbs]
    assert all(isinstance(g, int) for g in got)
    assert all(a > b for a, b in zip(got, got[1:]))                       # monotone: a higher target, a smaller SSE bound
    assert na.psnr_to_max_sse(30.0) == 51137740
    arr = na.psnr_to_max_sse(np.array(dbs))
    assert arr.dtype == np.int64 and arr.tolist() == got
    fine = na.psnr_to_max_sse(np.linspace(20.0, 50.0, 2001))
    assert (np.diff(fine) <= 0).all()
    for bad in (0, 0.0, -1.0, float("inf"), float("-inf"), float("nan"), [30.0, 0.0], [30.0, float("nan")], "x", []):
        with pytest.raises(na.NhwError):
            na.psnr_to_max_sse(bad)


@pytest.mark.parametrize("args,msg", [
    (["--min-psnr", "0", "a.bmp", "b.nhw"], "--min-psnr wants a positive number"),
    (["--min-psnr", "-3", "a.bmp", "b.nhw"], "--min-psnr wants a positive number"),
    (["--min-psnr", "x", "a.bmp", "b.nhw"], "--min-psnr wants a positive number"),
    (["--min-psnr", "30dB", "a.bmp", "b.nhw"], "--min-psnr wants a positive number"),
    (["--min-psnr", "inf", "a.bmp", "b.nhw"], "--min-psnr wants a positive number"),
    (["--min-psnr", "30", "--max-bytes", "5000", "a.bmp", "b.nhw"], "mutually exclusive"),
    (["--max-bytes", "5000", "--min-psnr", "30", "a.bmp", "b.nhw"], "mutually exclusive"),
    (["--min-psnr", "30", "--synthetic", "4", "--outdir", "d"], "not with --synthetic or --tar"),
    (["--min-psnr", "30", "--tar", "a.tar", "b.tar"], "not with --synthetic or --tar"),
    (["-q10", "--min-quality", "12", "--min-psnr", "30", "a.bmp", "b.nhw"], "--min-quality 12 is above the top quality q10"),
    (["--min-psnr", "30", "--min-quality", "0", "a.bmp", "b.nhw"], "--min-quality wants a quality 1..23"),
    (["--min-quality", "3", "a.bmp", "b.nhw"], "--min-quality needs --max-bytes or --min-psnr"),
])
def test_cli_psnr_arguments_fail_before_any_gpu_work(cli, tmp_path, args, msg):
    """(a.bmp does not exist: a run that got as far as reading it would say "Could not open file" and exit 255)"""
    rc, out, err = run(CLI, *[str(tmp_path / a) if a.endswith((".bmp", ".nhw", ".tar")) else a for a in args])
    assert rc == 1 and msg in err and "Could not open" not in out
    assert "PSNR (MI355X build): " in run(CLI, "-h")[1]


# ---------------------------------------------------------------- on the MI355X
def _expected(files, status, sse, ladder, targets):
    """the contract in Python over fixed-quality results files[q][i] / status[q][i] / sse[q][i] (None where the encode failed):
    (file, size, status, quality, sse) per image"""
    ladder = ladder or list(range(1, 24))
    want = []
    for i, t in enumerate(targets):
        for q in ladder:
            if status[q][i] == 0 and sse[q][i] <= t:
                want.append((files[q][i], len(files[q][i]), 0, q, sse[q][i]))
                break
        else:
            q = ladder[-1]
            st = status[q][i]
            want.append((files[q][i], len(files[q][i]), -7 if st == 0 else st, q, sse[q][i] if st == 0 else UINT64_MAX))
    return want


@pytest.fixture(scope="module")
def psnr_set(oracle):
    """test_fit.py's 48 images (oracle synth seeds, noise / flat / gradient / blocks, make(50431) which overflows from q17 up, make(1000..1016)),
    their fixed-quality files at every quality, the device decoder's pictures of them and the numpy SSE against the input"""
    import nhwcodec_amd as na
    from gpu_fuzz_classes import encode_with_status, make
    from oracle.harness import class_image
    imgs = [oracle.synth(s) for s in range(20)] + [class_image("noise", s) for s in range(4)] + [class_image("flat"), class_image("gradient")]
    imgs += [class_image("blocks", s) for s in range(4)] + [make(50431)] + [make(s) for s in range(1000, 1017)]
    imgs = np.stack(imgs)
    enc = na.Encoder(0, max_batch=64)
    dec = na.Decoder(0, max_batch=64)
    files, status, sse = {}, {}, {}
    for q in range(1, 24):
        files[q], status[q] = encode_with_status(enc, imgs, q)
        ok = [i for i in range(len(imgs)) if status[q][i] == 0]
        px, dq = dec.decode([files[q][i] for i in ok])
        assert dq == [q] * len(ok)
        s = _np_sse(imgs[ok], px)
        sse[q] = [None] * len(imgs)
        for k, i in enumerate(ok):
            sse[q][i] = int(s[k])
    assert status[17][30] == na.NHW_E_CODEBOOK and status[16][30] == 0
    yield enc, dec, imgs, files, status, sse
    dec.close()
    enc.close()


def _targets(imgs, status, sse, exact_minus_one):
    """per image: met at the first rung (a huge target), met by no rung (0 where no rung decodes exactly), the exact SSE at a middle rung
    (q18, or q16 for the image that overflows from q17) -- minus 1 with `exact_minus_one` -- and a seeded spread between the extremes"""
    rng = np.random.default_rng(5)
    t = []
    for i in range(len(imgs)):
        ok = [sse[q][i] for q in range(1, 24) if status[q][i] == 0]
        k = i % 4
        if k == 0:
            t.append(1 << 40)
        elif k == 1:
            t.append(max(min(ok) - 1, 0))
        elif k == 2:
            x = sse[18][i] if status[18][i] == 0 else sse[16][i]
            t.append(x - 1 if exact_minus_one else x)
        else:
            t.append(int(rng.integers(min(ok), max(ok) + 1)))
    return t


def _device_fit(enc, dec, imgs, targets, ladder):
    import torch
    bgr = torch.from_numpy(imgs).cuda()
    o, sizes, st, qual, sse = enc.encode_fit_psnr_device(bgr, dec, max_sse=torch.tensor(targets, dtype=torch.int64, device="cuda"), ladder=ladder)
    torch.cuda.synchronize()
    o, sizes, st, qual, sse = o.cpu().numpy(), sizes.cpu().numpy(), st.cpu().numpy(), qual.cpu().numpy(), sse.cpu().numpy().view(np.uint64)
    return [(o[i, :sizes[i]].tobytes(), int(sizes[i]), int(st[i]), int(qual[i]), int(sse[i])) for i in range(len(imgs))]


def _host_fit(enc, dec, imgs, targets, ladder):
    """nhw_enc_fit_sse_batch with SSE targets (encode_fit_psnr takes dB: the C entry point is called directly to give exact targets)"""
    n = len(imgs)
    imgs = np.ascontiguousarray(imgs)
    tgt = np.asarray(targets, np.uint64)
    arena = np.empty(n * (512 << 10), np.uint8)
    offs = np.empty(n + 1, np.uint64)
    status = np.empty(n, np.int32)
    quality = np.empty(n, np.int32)
    sse = np.empty(n, np.uint64)
    lad, lad_n = enc._ladder(ladder)
    enc._chk(enc.lib.nhw_enc_fit_sse_batch(enc.h, dec.h, imgs.ctypes.data, n, tgt.ctypes.data, lad, lad_n, arena.ctypes.data, arena.size,
                                           offs.ctypes.data, status.ctypes.data, quality.ctypes.data, sse.ctypes.data))
    return [(arena[int(offs[i]):int(offs[i + 1])].tobytes(), int(offs[i + 1] - offs[i]), int(status[i]), int(quality[i]), int(sse[i])) for i in range(n)]


@pytest.mark.gpu
def test_sse_against_numpy():
    import torch
    import nhwcodec_amd as na
    rng = np.random.default_rng(3)
    for n in (1, 7, 129):
        a = rng.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)
        b = rng.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)
        b[0] = a[0]                                                      # identical
        if n > 1:
            b[1] = a[1]; b[1].reshape(-1)[0] ^= 0x5A                     # one byte at the first position
        if n > 2:
            b[2] = a[2]; b[2].reshape(-1)[-1] = 255 - a[2].reshape(-1)[-1]   # one byte at the last position
        if n > 3:
            a[3] = 0; b[3] = 255                                         # the largest SSE, beyond 32 bits
        if n > 4:
            b[4] = np.clip(a[4].astype(np.int32) + rng.integers(-3, 4, a[4].shape), 0, 255)   # a near copy
        got = na.sse_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
        torch.cuda.synchronize()
        want = _np_sse(a, b)
        assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == want.tolist()
        assert want[0] == 0
        if n > 3:
            assert want[3] == 51137740800
    lib = na._library()
    x = torch.zeros(2 * 786432 + 64, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.int64, device="cuda")
    assert lib.nhw_sse_batch_device(x.data_ptr() + 8, x.data_ptr() + 16, 1, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_sse_batch_device(x.data_ptr(), x.data_ptr() + 4, 1, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_sse_batch_device(x.data_ptr(), x.data_ptr(), 0, out.data_ptr(), None) == na.NHW_E_ARG
    assert lib.nhw_sse_batch_device(x.data_ptr(), None, 1, out.data_ptr(), None) == na.NHW_E_ARG
    with pytest.raises(na.NhwError, match="rc=-4"):
        na.sse_device(x[8:8 + 786432], x[786432 + 16:2 * 786432 + 16])


@pytest.mark.gpu
def test_sse_captured_in_a_graph():
    import torch
    import nhwcodec_amd as na
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.integers(0, 256, (5, 512, 512, 3), dtype=np.uint8)).cuda()
    b = torch.from_numpy(rng.integers(0, 256, (5, 512, 512, 3), dtype=np.uint8)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = na.sse_device(a, b)
    b.copy_(a)
    b[2].view(-1)[100] ^= 1
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0, 0, int(_np_sse(a[2].cpu().numpy(), b[2].cpu().numpy())[0]), 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("ladder", list(LADDERS))
def test_fit_psnr_equals_the_brute_force(psnr_set, ladder):
    """device and host paths: file, size, status, quality and SSE are those the contract picks out of fixed-quality encodes and decodes;
    a target equal to the exact SSE at a rung fits there, that value minus 1 does not"""
    enc, dec, imgs, files, status, sse = psnr_set
    lad = LADDERS[ladder]
    wants = {}
    for minus_one in (False, True):
        targets = _targets(imgs, status, sse, minus_one)
        want = wants[minus_one] = _expected(files, status, sse, lad, targets)
        assert _device_fit(enc, dec, imgs, targets, lad) == want
        assert _host_fit(enc, dec, imgs, targets, lad) == want
        if ladder == "default":
            assert any(w[2] == -7 for w in want) and any(w[2] == 0 and w[3] == 1 for w in want) and any(w[2] == 0 and 1 < w[3] < 23 for w in want)
        if ladder == "q20":
            assert any(w[2] == -7 for w in want)
    if ladder == "default":
        targets = _targets(imgs, status, sse, False)
        exact = [i for i in range(2, len(imgs), 4) if wants[False][i][2] == 0 and wants[False][i][4] == targets[i]]
        assert len(exact) >= 5                                      # the equality case: the target is the SSE the image gets ...
        for i in exact:                                             # ... and one less moves the image on to a later rung, or to none
            assert wants[True][i][3] > wants[False][i][3] or wants[True][i][2] != 0
    assert not any(status[q][i] == 0 and sse[q][i] is None for q in range(1, 24) for i in range(len(imgs)))


@pytest.mark.gpu
def test_fit_psnr_python_targets_in_db(psnr_set):
    """min_psnr as one float and per image, on both paths, equals max_sse = psnr_to_max_sse(min_psnr)"""
    import torch
    import nhwcodec_amd as na
    enc, dec, imgs, files, status, sse = psnr_set
    dbs = np.linspace(24.0, 40.0, len(imgs))
    targets = na.psnr_to_max_sse(dbs).tolist()
    want = _expected(files, status, sse, None, targets)
    bgr = torch.from_numpy(imgs).cuda()
    o, sizes, st, q, s = enc.encode_fit_psnr_device(bgr, dec, min_psnr=dbs)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [w[2] for w in want] and q.cpu().tolist() == [w[3] for w in want]
    hf, hq, hs, hsse = enc.encode_fit_psnr(imgs, dec, dbs)
    assert [(f, len(f), a, b, c) for f, b, a, c in zip(hf, hq, hs, hsse)] == want
    one = na.psnr_to_max_sse(31.5)
    want1 = _expected(files, status, sse, [18, 19, 20], [one] * len(imgs))
    hf, hq, hs, hsse = enc.encode_fit_psnr(imgs, dec, 31.5, [18, 19, 20])
    assert [(f, len(f), a, b, c) for f, b, a, c in zip(hf, hq, hs, hsse)] == want1


@pytest.mark.gpu
def test_fit_psnr_against_the_cpu_oracle(psnr_set, oracle):
    """the chosen file is the oracle's at the chosen quality; the oracle's decode of it meets the target with the reported SSE; every
    earlier rung's oracle decode misses the target, or its encode overflows"""
    enc, dec, imgs, files, status, sse = psnr_set
    ladder = [12, 16, 17, 18, 20, 23]
    pick = [3, 21, 27, 30]
    sub = imgs[pick]
    tgt = []
    for i in pick:
        ok = sorted(sse[q][i] for q in ladder if status[q][i] == 0)
        tgt.append(ok[len(ok) // 2])
    got = _host_fit(enc, dec, sub, tgt, ladder)
    for k in range(len(pick)):
        f, size, st, q, s = got[k]
        assert st == 0 and s <= tgt[k]
        assert f == oracle.encode(sub[k], q)
        px, dq = oracle.decode(f)
        assert dq == q and int(_np_sse(sub[k], px)[0]) == s
        for q2 in ladder[:ladder.index(q)]:
            try:
                f2 = oracle.encode(sub[k], q2)
            except RuntimeError as ex:
                assert "rc=-2" in str(ex)
                continue
            assert int(_np_sse(sub[k], oracle.decode(f2)[0])[0]) > tgt[k]


@pytest.mark.gpu
def test_fit_psnr_stats_count_the_open_images(psnr_set):
    import nhwcodec_amd as na
    enc, dec, imgs, files, status, sse = psnr_set
    for ladder, exact in ((None, False), ([17, 18, 19, 20, 21, 22, 23], True), ([23, 20, 17], False)):
        targets = _targets(imgs, status, sse, exact)
        _host_fit(enc, dec, imgs, targets, ladder)
        st = enc.fit_stats()
        lad = ladder or list(range(1, 24))
        open_ = list(range(len(imgs)))
        counts = []
        for q in lad:
            if not open_:
                break
            counts.append(len(open_))
            open_ = [i for i in open_ if not (status[q][i] == 0 and sse[q][i] <= targets[i])]
        assert st.rungs == len(counts) and list(st.images[:st.rungs]) == counts and list(st.quality[:st.rungs]) == lad[:st.rungs]
        assert st.total_ms > 0
    _host_fit(enc, dec, imgs, [1 << 40] * len(imgs), None)
    st = enc.fit_stats()
    assert st.rungs == 1 and st.images[0] == len(imgs)          # a generous target: every image closes at the first rung
    t = na.DecTiming()
    assert dec.lib.nhw_dec_last_timing(dec.h, ctypes.byref(t)) == 0 and t.total_ms > 0


@pytest.mark.gpu
def test_fit_psnr_codebook_overflow_rungs_are_passed_over(psnr_set):
    import nhwcodec_amd as na
    enc, dec, imgs, files, status, sse = psnr_set
    got = _host_fit(enc, dec, imgs[30:31], [0], [16, 17, 20])
    assert got[0][2] == na.NHW_E_CODEBOOK and got[0][1] == 0 and got[0][3] == 20 and got[0][4] == UINT64_MAX
    got = _host_fit(enc, dec, imgs[30:31], [1 << 40], [17, 20, 16])
    assert got[0] == (files[16][30], len(files[16][30]), 0, 16, sse[16][30])


@pytest.mark.gpu
def test_fit_psnr_rejects_bad_calls_before_launching(psnr_set):
    import torch
    import nhwcodec_amd as na
    enc, dec, imgs = psnr_set[:3]
    bgr = torch.from_numpy(imgs[:4]).cuda()
    small = na.Decoder(0, max_batch=2)
    with pytest.raises(na.NhwError, match="max_batch"):
        enc.encode_fit_psnr_device(bgr, small, min_psnr=30.0)
    with pytest.raises(na.NhwError, match="max_batch"):
        enc.encode_fit_psnr(imgs[:4], small, 30.0)
    tgt = torch.full((4,), 1000, dtype=torch.int64, device="cuda")
    o, sz, st, q = enc.alloc_out(4) + (torch.empty(4, dtype=torch.int32, device="cuda"),)
    s = torch.empty(4, dtype=torch.int64, device="cuda")
    lib = enc.lib
    args = (bgr.data_ptr(), 4, tgt.data_ptr(), None, 0, o.data_ptr(), sz.data_ptr(), st.data_ptr(), q.data_ptr(), s.data_ptr(), None)
    assert lib.nhw_enc_fit_sse_batch_device(enc.h, small.h, *args) == na.NHW_E_ARG         # the C side refuses it as well
    assert lib.nhw_enc_fit_sse_batch_device(enc.h, None, *args) == na.NHW_E_ARG
    small.close()
    for ladder, rc in (([20, 20], na.NHW_E_QUALITY), ([24], na.NHW_E_QUALITY), ([0, 5], na.NHW_E_QUALITY), (list(range(1, 24)) + [1], na.NHW_E_ARG)):
        with pytest.raises(na.NhwError, match=f"rc={rc}"):
            enc.encode_fit_psnr(imgs[:2], dec, 30.0, ladder)
        with pytest.raises(na.NhwError, match=f"rc={rc}"):
            enc.encode_fit_psnr_device(bgr, dec, max_sse=tgt, ladder=ladder)
    for kw in ({}, {"min_psnr": 30.0, "max_sse": 1000}):
        with pytest.raises(na.NhwError, match="exactly one of"):
            enc.encode_fit_psnr_device(bgr, dec, **kw)
    for kw in ({"min_psnr": 0.0}, {"min_psnr": float("nan")}, {"max_sse": -1}, {"min_psnr": [30.0] * 3}, {"max_sse": torch.zeros(4, dtype=torch.int32, device="cuda")}):
        with pytest.raises(na.NhwError):
            enc.encode_fit_psnr_device(bgr, dec, **kw)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        with pytest.raises(na.NhwError, match="rc=-4.*captured"):
            enc.encode_fit_psnr_device(bgr, dec, max_sse=tgt, out=(o, sz, st, q, s))
    torch.cuda.synchronize()


def _fit_psnr_on_device_reference(enc, dec, bgr, target, ladder):
    """the contract, on the device, from full-batch fixed-quality encodes, decodes and sse_device"""
    import torch
    import nhwcodec_amd as na
    n = bgr.shape[0]
    e_out = torch.zeros((n, 512 << 10), dtype=torch.uint8, device="cuda")
    e_sz = torch.zeros(n, dtype=torch.int32, device="cuda"); e_st = torch.zeros_like(e_sz); e_q = torch.zeros_like(e_sz)
    e_sse = torch.zeros(n, dtype=torch.int64, device="cuda")
    open_ = torch.ones(n, dtype=torch.bool, device="cuda")
    buf = enc.alloc_out(n)
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * (512 << 10)
    for r, q in enumerate(ladder):
        o, sz, st = enc.encode_device(bgr, q, out=buf)
        px, dst, _ = dec.decode_device(o, offs, sz)
        s = na.sse_device(bgr, px)
        good = (st == 0) & (dst == 0)
        fits = open_ & good & (s <= target)
        close = fits | open_ if r == len(ladder) - 1 else fits
        e_out[close] = o[close]
        e_sz[close] = sz[close]
        e_st[close] = torch.where(fits, st, torch.where(st == 0, torch.full_like(st, -7), st))[close]
        e_q[close] = q
        e_sse[close] = torch.where(good, s, torch.full_like(s, -1))[close]
        open_ &= ~fits
    return e_out, e_sz, e_st, e_q, e_sse


@pytest.mark.gpu
def test_fit_psnr_at_scale_on_a_device_only_handle():
    """1024 images made on the device, n == max_batch on both handles, per-image targets spread around the q18 SSE, on torch's default
    stream and on a side stream; a plain encode and a plain decode on the handles afterwards give what they gave before"""
    import torch
    import nhwcodec_amd as na
    n = 1024
    enc = na.Encoder(0, max_batch=n, device_only=True)
    dec = na.Decoder(0, max_batch=n)
    bgr = enc.synth_device(n, 777)
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * (512 << 10)
    o18, s18, st18 = [x.clone() for x in enc.encode_device(bgr, 18)]
    px18, dst18, _ = [x.clone() for x in dec.decode_device(o18, offs, s18)]
    sse18 = na.sse_device(bgr, px18)
    assert bool((st18 == 0).all()) and bool((dst18 == 0).all())
    g = torch.Generator(device="cuda").manual_seed(13)
    target = (sse18.double() * (0.6 + 0.8 * torch.rand(n, device="cuda", generator=g, dtype=torch.float64))).long()
    target[::101] = 0
    target[5::97] = sse18[5::97]                                        # exactly the q18 SSE
    ladder = list(range(14, 24))
    want = _fit_psnr_on_device_reference(enc, dec, bgr, target, ladder)
    assert (want[2] == -7).any() and (want[2] == 0).any() and (want[3] < 18).any() and (want[3] > 18).any()
    for side in (False, True):
        s = torch.cuda.Stream() if side else torch.cuda.default_stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            o, sz, st, q, sse = enc.encode_fit_psnr_device(bgr, dec, max_sse=target, ladder=ladder)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert torch.equal(sz, want[1]) and torch.equal(st, want[2]) and torch.equal(q, want[3]) and torch.equal(sse, want[4])
        assert same_files(o, want[0], sz)
    o, s, st = enc.encode_device(bgr, 18)
    px, dst, _ = dec.decode_device(o, offs, s)
    torch.cuda.synchronize()
    assert torch.equal(s, s18) and torch.equal(st, st18) and same_files(o, o18, s18)
    assert torch.equal(dst, dst18) and torch.equal(px, px18)
    dec.close()
    enc.close()


@pytest.mark.gpu
def test_cli_batch_to_a_psnr_target(cli, oracle, tmp_path):
    """nhw-enc -q20 --min-psnr DB --batch: the written files equal the oracle's at the quality they carry and meet DB; the image whose best
    PSNR is the lowest reaches DB at no quality, is not written and is reported, and the exit status is 1"""
    import nhwcodec_amd as na
    from gpu_fuzz_classes import encode_with_status
    from oracle.harness import bmp_bytes, class_image
    imgs = np.stack([oracle.synth(s) for s in (41, 42, 43, 44, 45)] + [class_image("noise", 9)])
    enc = na.Encoder(0, max_batch=8)
    dec = na.Decoder(0, max_batch=8)
    best = np.full(len(imgs), 1 << 62)
    for q in range(1, 21):
        files, status = encode_with_status(enc, imgs, q)
        ok = [i for i in range(len(imgs)) if status[i] == 0]
        px, _ = dec.decode([files[i] for i in ok])
        for k, i in enumerate(ok):
            best[i] = min(best[i], int(_np_sse(imgs[i], px[k])[0]))
    dec.close(); enc.close()
    order = np.argsort(best)
    worst = int(order[-1])
    assert best[worst] > best[order[-2]]
    psnr = lambda s: 10 * math.log10(PEAK / s)
    db = round((psnr(best[worst]) + psnr(best[order[-2]])) / 2, 3)
    bound = na.psnr_to_max_sse(db)
    assert best[order[-2]] <= bound < best[worst]
    for k, im in enumerate(imgs):
        (tmp_path / f"img{k}.bmp").write_bytes(bmp_bytes(im))
    rc, out, err = run(CLI, "-q20", "--min-psnr", str(db), "--batch", str(tmp_path))
    assert rc == 1
    assert f"img{worst}.nhw: no quality in q1..q20 reaches" in err
    assert not (tmp_path / f"img{worst}.nhw").exists()
    for k in range(len(imgs)):
        if k == worst:
            continue
        f = (tmp_path / f"img{k}.nhw").read_bytes()
        px, q = oracle.decode(f)
        assert f == oracle.encode(imgs[k], q)
        assert int(_np_sse(imgs[k], px)[0]) <= bound
