"""Encode to a byte budget (nhw_enc_fit_batch_device / nhw_enc_fit_batch, Encoder.encode_fit*, nhw-enc --max-bytes): for every image the
file of the first ladder rung whose encode succeeds within the image's budget, identical to the fixed-quality encode at that quality."""
import os

import numpy as np
import pytest

from tests.support import CLI, ROOT, built_cli, load_lib, run, same_files

LADDERS = {"default": None, "every4": [20, 16, 12, 8, 4], "q20": [20]}


@pytest.fixture(scope="module")
def cli():
    return built_cli("nhw-enc")


# ---------------------------------------------------------------- without a GPU
def test_library_exports_the_fit_entry_points():
    import nhwcodec_amd
    lib = load_lib()
    for name in ("nhw_enc_fit_batch_device", "nhw_enc_fit_batch", "nhw_enc_last_fit_stats"):
        assert hasattr(lib, name)
    assert nhwcodec_amd.NHW_E_BUDGET == -7
    assert "NHW_E_BUDGET = -7" in open(os.path.join(ROOT, "include", "nhw_hip.h")).read()


@pytest.mark.parametrize("args,msg", [
    (["--max-bytes", "0", "a.bmp", "b.nhw"], "--max-bytes wants a positive number"),
    (["--max-bytes", "x", "a.bmp", "b.nhw"], "--max-bytes wants a positive number"),
    (["--max-bytes", "-5", "a.bmp", "b.nhw"], "--max-bytes wants a positive number"),
    (["--max-bytes", "5000", "--synthetic", "4", "--outdir", "d"], "not with --synthetic or --tar"),
    (["--max-bytes", "5000", "--tar", "a.tar", "b.tar"], "not with --synthetic or --tar"),
    (["-q10", "--min-quality", "12", "--max-bytes", "5000", "a.bmp", "b.nhw"], "--min-quality 12 is above the top quality q10"),
    (["--max-bytes", "5000", "--min-quality", "0", "a.bmp", "b.nhw"], "--min-quality wants a quality 1..23"),
    (["--min-quality", "3", "a.bmp", "b.nhw"], "--min-quality needs --max-bytes"),
])
def test_cli_budget_arguments_fail_before_any_gpu_work(cli, tmp_path, args, msg):
    """(a.bmp does not exist: a run that got as far as reading it would say "Could not open file" and exit 255)"""
    rc, out, err = run(CLI, *[str(tmp_path / a) if a.endswith((".bmp", ".nhw", ".tar")) else a for a in args])
    assert rc == 1 and msg in err and "Could not open" not in out
    assert "--max-bytes" in run(CLI, "-h")[1]


# ---------------------------------------------------------------- on the MI355X
def _expected(files, status, ladder, budgets):
    """the contract in Python over fixed-quality results files[q][i] / status[q][i]: (files, sizes, status, quality) per image"""
    ladder = ladder or list(range(23, 0, -1))
    want = []
    for i, b in enumerate(budgets):
        for q in ladder:
            if status[q][i] == 0 and len(files[q][i]) <= b:
                want.append((files[q][i], len(files[q][i]), 0, q))
                break
        else:
            q = ladder[-1]
            st = status[q][i]
            want.append((files[q][i], len(files[q][i]), -7 if st == 0 else st, q))
    return want


@pytest.fixture(scope="module")
def fit_set(oracle):
    """48 images: oracle synth seeds, noise / flat / gradient / blocks, gpu_fuzz_classes images (50431 overflows the code book from q17 up),
    their fixed-quality files at every quality, and budgets spread between each image's q1 and largest size (every sixth below its q1 size)"""
    import nhwcodec_amd as na
    from gpu_fuzz_classes import encode_with_status, make
    from oracle.harness import class_image
    imgs = [oracle.synth(s) for s in range(20)] + [class_image("noise", s) for s in range(4)] + [class_image("flat"), class_image("gradient")]
    imgs += [class_image("blocks", s) for s in range(4)] + [make(50431)] + [make(s) for s in range(1000, 1017)]
    imgs = np.stack(imgs)
    enc = na.Encoder(0, max_batch=64)
    files, status = {}, {}
    for q in range(1, 24):
        files[q], status[q] = encode_with_status(enc, imgs, q)
    assert status[17][30] == na.NHW_E_CODEBOOK and status[16][30] == 0
    rng = np.random.default_rng(7)
    budgets = []
    for i in range(len(imgs)):
        lo = len(files[1][i])
        hi = max(len(files[q][i]) for q in range(1, 24) if status[q][i] == 0)
        budgets.append(lo - 1 if i % 6 == 5 else int(rng.integers(lo, hi + 1)))
    yield enc, imgs, files, status, budgets
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ladder", list(LADDERS))
def test_fit_equals_the_fixed_quality_encodes(fit_set, ladder):
    """device and host paths: files, sizes, status and quality are those the contract picks out of fixed-quality encodes"""
    import torch
    enc, imgs, files, status, budgets = fit_set
    want = _expected(files, status, LADDERS[ladder], budgets)
    bgr = torch.from_numpy(imgs).cuda()
    o, sizes, st, qual = enc.encode_fit_device(bgr, torch.tensor(budgets, dtype=torch.int32, device="cuda"), LADDERS[ladder])
    torch.cuda.synchronize()
    o, sizes, st, qual = o.cpu().numpy(), sizes.cpu().numpy(), st.cpu().numpy(), qual.cpu().numpy()
    got = [(o[i, :sizes[i]].tobytes(), int(sizes[i]), int(st[i]), int(qual[i])) for i in range(len(imgs))]
    assert got == want
    hf, hq, hs = enc.encode_fit(imgs, budgets, LADDERS[ladder])
    assert [(f, len(f), s, q) for f, s, q in zip(hf, hs, hq)] == want
    if ladder == "q20":
        assert any(w[2] == -7 for w in want)


@pytest.mark.gpu
def test_fit_against_the_cpu_oracle(fit_set, oracle):
    """the chosen file is the oracle's at the chosen quality; every higher rung's oracle file is over the budget or overflows"""
    enc, imgs, files, status, budgets = fit_set
    ladder = [23, 21, 18, 16, 12, 8, 4]
    pick = [3, 21, 27, 30]
    sub = imgs[pick]
    bud = [sorted(len(files[q][i]) for q in ladder if status[q][i] == 0)[1] for i in pick]
    got_f, got_q, got_s = enc.encode_fit(sub, bud, ladder)
    for k in range(len(pick)):
        assert got_s[k] == 0 and len(got_f[k]) <= bud[k]
        assert got_f[k] == oracle.encode(sub[k], got_q[k])
        for q in ladder[:ladder.index(got_q[k])]:
            try:
                assert len(oracle.encode(sub[k], q)) > bud[k]
            except RuntimeError as ex:
                assert "rc=-2" in str(ex)


@pytest.mark.gpu
def test_codebook_overflow_rungs_are_passed_over(fit_set):
    import nhwcodec_amd as na
    from gpu_fuzz_classes import make
    enc = fit_set[0]
    f, q, s = enc.encode_fit(make(50431)[None], 1 << 20)
    assert (q, s) == ([16], [na.NHW_OK]) and f[0] == fit_set[2][16][30]


@pytest.mark.gpu
def test_budget_below_every_rung(fit_set):
    import nhwcodec_amd as na
    enc, imgs, files, status = fit_set[:4]
    f, q, s = enc.encode_fit(imgs[:3], 1, [20, 16, 12, 8, 4])
    assert s == [na.NHW_E_BUDGET] * 3 and q == [4] * 3
    assert f == files[4][:3]
    dec = na.Decoder(0, max_batch=4)
    _, dq = dec.decode(f)
    dec.close()
    assert dq == [4] * 3


@pytest.mark.gpu
def test_fit_stats_count_the_open_images(fit_set):
    enc, imgs, files, status, budgets = fit_set
    for ladder, bud in (([20, 16, 12, 8, 4], budgets), (None, budgets), ([16, 10, 4], [1 << 20] * len(imgs))):
        enc.encode_fit(imgs, bud, ladder)
        st = enc.fit_stats()
        lad = ladder or list(range(23, 0, -1))
        open_ = list(range(len(imgs)))
        counts = []
        for q in lad:
            if not open_:
                break
            counts.append(len(open_))
            open_ = [i for i in open_ if not (status[q][i] == 0 and len(files[q][i]) <= bud[i])]
        assert st.rungs == len(counts) and list(st.images[:st.rungs]) == counts and list(st.quality[:st.rungs]) == lad[:st.rungs]
        assert st.total_ms > 0
    assert st.rungs < 3          # a generous budget: the search stops once no image is left open


@pytest.mark.gpu
def test_fit_rejects_bad_calls_before_launching(fit_set):
    import nhwcodec_amd as na
    enc, imgs = fit_set[:2]
    for ladder, rc in (([20, 20], na.NHW_E_QUALITY), ([24], na.NHW_E_QUALITY), ([0, 5], na.NHW_E_QUALITY), (list(range(23, 0, -1)) + [1], na.NHW_E_ARG)):
        with pytest.raises(na.NhwError, match=f"rc={rc}"):
            enc.encode_fit(imgs[:2], 5000, ladder)


def _fit_on_device_reference(enc, bgr, budget, ladder):
    """the contract, on the device, from full-batch fixed-quality encodes"""
    import torch
    n = bgr.shape[0]
    e_out = torch.zeros((n, 512 << 10), dtype=torch.uint8, device="cuda")
    e_sz = torch.zeros(n, dtype=torch.int32, device="cuda"); e_st = torch.zeros_like(e_sz); e_q = torch.zeros_like(e_sz)
    open_ = torch.ones(n, dtype=torch.bool, device="cuda")
    buf = enc.alloc_out(n)
    for r, q in enumerate(ladder):
        o, sz, st = enc.encode_device(bgr, q, out=buf)
        fits = open_ & (st == 0) & (sz.long() <= budget.long())
        close = fits | open_ if r == len(ladder) - 1 else fits
        e_out[close] = o[close]
        e_sz[close] = sz[close]
        e_st[close] = torch.where(fits, st, torch.where(st == 0, torch.full_like(st, -7), st))[close]
        e_q[close] = q
        open_ &= ~fits
    return e_out, e_sz, e_st, e_q


@pytest.mark.gpu
def test_fit_at_scale_on_a_device_only_handle():
    """1024 images made on the device, n == max_batch, per-image budgets around the q20 sizes (some below every rung), on torch's default
    stream and on a side stream; a plain encode on the handle afterwards is what it was before"""
    import torch
    import nhwcodec_amd as na
    n = 1024
    enc = na.Encoder(0, max_batch=n, device_only=True)
    bgr = enc.synth_device(n, 4242)
    o20, s20, st20 = [x.clone() for x in enc.encode_device(bgr, 20)]
    g = torch.Generator(device="cuda").manual_seed(11)
    budget = (s20.float() * (0.25 + 0.9 * torch.rand(n, device="cuda", generator=g))).int()
    budget[::97] = 100
    ladder = [22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 1]
    want = _fit_on_device_reference(enc, bgr, budget, ladder)
    assert (want[2] == -7).any() and (want[2] == 0).any()
    for side in (False, True):
        s = torch.cuda.Stream() if side else torch.cuda.default_stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            o, sz, st, q = enc.encode_fit_device(bgr, budget, ladder)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert torch.equal(sz, want[1]) and torch.equal(st, want[2]) and torch.equal(q, want[3])
        assert same_files(o, want[0], sz)
    o, s, st = enc.encode_device(bgr, 20)
    torch.cuda.synchronize()
    assert torch.equal(s, s20) and torch.equal(st, st20) and same_files(o, o20, s20)
    enc.close()


@pytest.mark.gpu
def test_cli_batch_to_a_byte_budget(cli, oracle, tmp_path):
    """nhw-enc -q20 --max-bytes N --batch: five files within N bytes that equal the oracle's at the quality they carry; the sixth image
    fits no quality, is not written and is reported, and the exit status is 1"""
    import nhwcodec_amd as na
    from gpu_fuzz_classes import encode_with_status
    from oracle.harness import bmp_bytes, class_image
    imgs = np.stack([oracle.synth(s) for s in (31, 32, 33, 34, 35)] + [class_image("noise", 9)])
    enc = na.Encoder(0, max_batch=8)
    least = np.full(len(imgs), 1 << 30)
    for q in range(1, 21):
        files, status = encode_with_status(enc, imgs, q)
        least = np.minimum(least, [len(f) if s == 0 else 1 << 30 for f, s in zip(files, status)])
    enc.close()
    order = np.argsort(least)
    assert order[-1] == 5 and least[order[-1]] > least[order[-2]]
    budget = int(least[order[-2]])
    for k, im in enumerate(imgs):
        (tmp_path / f"img{k}.bmp").write_bytes(bmp_bytes(im))
    rc, out, err = run(CLI, "-q20", "--max-bytes", str(budget), "--batch", str(tmp_path))
    assert rc == 1
    assert f"img5.nhw: no quality in q20..q1 fits {budget} bytes (q1: " in err
    assert not (tmp_path / "img5.nhw").exists()
    for k in range(5):
        f = (tmp_path / f"img{k}.nhw").read_bytes()
        assert len(f) <= budget
        _, q = oracle.decode(f)
        assert f == oracle.encode(imgs[k], q)
