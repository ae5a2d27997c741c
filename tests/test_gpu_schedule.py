"""The kernels that split one item across workgroups, under forced slice orders (pytest -m gpu).

In production the workgroups of one picture or file are dispatched side by side, so a kernel that reads what another workgroup of the
same launch writes can pass every other test by timing alone.  nhw_debug_slice_order / nhw_dec_debug_slice_order run each such kernel
one slice per launch, slices ascending (mode 1) or descending (mode 2): a slice that reads what a slice before it (mode 1) or behind it
(mode 2) writes then sees the written values.  Every check here is against the CPU oracle, byte for byte.  The kernels in the mode and
the ones that cannot have the hazard: DESIGN.md, "Kernels that split an item".
"""

import numpy as np
import pytest

from oracle.harness import class_image
from tests.support import golden, golden_names

# k_low_apply used to re-read the last row of the band above for its entry tail-rules flag, a row that band rewrites in the same launch.
# In mode 1 that read sees the rewritten row; it changes the flag only where the pair machine's answer for pair 254 of that row rewrites
# a map cell the flag depends on.  Synthetic seeds 0..255 at qualities 8, 9, 10, 15 and 16 never did (no seed to pin); the seeds below
# widen the batch's quality 1..16 content beyond the ones the other tests use.
EXTRA_SEEDS = [37, 101]
MODES = (1, 2)


def _batch(oracle):
    """21 pictures (a partial group of 8 behind two whole ones): synthetic seeds and the secondary classes"""
    imgs = [oracle.synth(s) for s in (0, 1, 2, 5, 8, 13)]
    imgs += [class_image(k, s) for k, s in (("noise", 0), ("blocks", 1), ("tiles", 2), ("gradient", 0), ("flat", 0), ("blocks", 4), ("noise", 3))]
    imgs += [oracle.synth(s) for s in EXTRA_SEEDS]
    while len(imgs) < 21:
        imgs.append(oracle.synth(100 + len(imgs)))
    return np.stack(imgs[:21])


@pytest.fixture(scope="module")
def imgs(oracle):
    return _batch(oracle)


@pytest.fixture(scope="module")
def want(oracle, imgs):
    """the oracle's files, per quality on demand"""
    cache = {}

    def get(q):
        if q not in cache:
            cache[q] = [oracle.encode(im, q) for im in imgs]
        return cache[q]
    return get


@pytest.fixture(scope="module")
def enc():
    import nhwcodec_amd
    e = nhwcodec_amd.Encoder(0, max_batch=32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=64)
    yield d
    d.close()


def _enc_mode(enc, mode):
    assert enc.lib.nhw_debug_slice_order(enc.h, mode) == 0


def _dec_mode(dec, mode):
    assert dec.lib.nhw_dec_debug_slice_order(dec.h, mode) == 0


def _encode(enc, imgs, q, mode):
    _enc_mode(enc, mode)
    try:
        return enc.encode(imgs, q)
    finally:
        _enc_mode(enc, 0)


def _decode(dec, files, mode):
    _dec_mode(dec, mode)
    try:
        return dec.decode(files)
    finally:
        _dec_mode(dec, 0)


def _first_diff(got, want):
    return next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


@pytest.mark.gpu
def test_mode_arguments_are_checked(enc, dec):
    assert enc.lib.nhw_debug_slice_order(enc.h, 3) != 0 and enc.lib.nhw_debug_slice_order(enc.h, -1) != 0
    assert dec.lib.nhw_dec_debug_slice_order(dec.h, 3) != 0 and dec.lib.nhw_dec_debug_slice_order(None, 1) != 0
    _enc_mode(enc, 0)
    _dec_mode(dec, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("q", range(1, 24))
def test_encoder_forced_order_matches_oracle(enc, imgs, want, q, mode):
    """every quality: pass A / pass B bands and pass C windows of the pre-filter (1..16), the chroma level-1 quarters (on the chroma stream)"""
    got = _encode(enc, imgs, q, mode)
    i = _first_diff(got, want(q))
    assert i is None, f"q{q} mode {mode}: image {i} ({len(got[i])} vs {len(want(q)[i])} bytes) differs from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_decoder_forced_order_goldens(dec, oracle, mode):
    """the committed reference-encoder files, every quality, in one batch (not a multiple of 8)"""
    names = golden_names()
    files = [golden(f) for f in names]
    assert len({int(f[1:3]) for f in names}) == 23
    px, qs = _decode(dec, files, mode)
    for i, f in enumerate(files):
        w, q = oracle.decode(f)
        assert qs[i] == q and np.array_equal(px[i], w), f"mode {mode}: {names[i]} decodes differently from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("q", [1, 8, 10, 16, 17, 20, 23])
def test_decoder_forced_order_gpu_files(enc, dec, oracle, imgs, q, mode):
    """files of the production encoder, a batch of 21"""
    files = enc.encode(imgs, q)
    px, qs = _decode(dec, files, mode)
    for i, f in enumerate(files):
        w, wq = oracle.decode(f)
        assert qs[i] == wq == q and np.array_equal(px[i], w), f"q{q} mode {mode}: file {i} decodes differently from the oracle"


@pytest.mark.gpu
def test_forced_order_leaves_no_state(enc, dec, oracle, imgs, want):
    """production, mode 2, production again on one handle each: the two production runs agree (and with the oracle)"""
    for q in (10, 20):
        a = enc.encode(imgs, q)
        b = _encode(enc, imgs, q, 2)
        c = enc.encode(imgs, q)
        assert a == c == want(q) and b == want(q), f"q{q}"
        pa, _ = dec.decode(a)
        pb, _ = _decode(dec, a, 2)
        pc, _ = dec.decode(a)
        assert np.array_equal(pa, pc) and np.array_equal(pa, pb)
        assert all(np.array_equal(pa[i], oracle.decode(f)[0]) for i, f in enumerate(a))
