"""CPU tests: the oracle restatement is pinned to the reference's outputs.

1. against the committed golden vectors (tests/golden/, generated from the canonical reference build by
   tests/golden/make_golden.py) -- complete .nhw files, sha256 of more files, per-checkpoint hashes;
2. against what the real reference (oracle/_ref: the unmodified sources, the stock binary) returned for the inputs below, checkpoint by
   checkpoint -- recorded in tests/golden/ref_record.json by tests/golden/make_ref_golden.py, so that no test needs the reference's sources.
"""
import hashlib
import os

import numpy as np
import pytest

from oracle.harness import class_image, synth_image

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _image(oracle, kind, seed):
    return oracle.synth(seed) if kind == "synth" else class_image(kind, seed)


def _h16(b):
    return hashlib.sha1(b).hexdigest()[:16]


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _trace_record(data, tr):
    """what the record holds of one traced encode: the file's sha256 and every checkpoint blob's short hash, in call order"""
    return {"nhw_sha256": _sha(data), "checkpoints": [[n, [_h16(b) for b in blobs]] for n, blobs in tr]}


def _assert_trace(rec, data, tr, what):
    got = _trace_record(data, tr)
    assert [n for n, _ in got["checkpoints"]] == [n for n, _ in rec["checkpoints"]], what
    for g, w in zip(got["checkpoints"], rec["checkpoints"]):
        assert g == w, f"{what}: checkpoint {g[0]}"
    assert got["nhw_sha256"] == rec["nhw_sha256"], what


# the inputs the reference was run on (tests/golden/make_ref_golden.py records its answers for exactly these)
TRACE_QS = [1, 3, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 23]
COLOUR_QS = [1, 4, 8, 12, 16]
STOCK_QS = [1, 6, 10, 11, 12, 13, 14, 16, 17, 18, 19, 20, 21, 22, 23]
HARD_KINDS = ["noise", "blocks", "tiles", "gradient"]
HARD_QS = (1, 5, 8, 10, 13, 16)
CODEBOOK_SEED, CODEBOOK_QS = 50431, (16, 17, 20, 23)


def colour_images(oracle):
    return [("synth_s12", oracle.synth(12)), ("noise_s2", class_image("noise", 2))]


def stock_images(oracle, q):
    # below quality 14 the third heap neighbour (what follows resIII) only shows on images loud enough for Y20's parent look-up
    imgs = [(str(s), oracle.synth(s)) for s in ((0, 1, 110, 117, 925) if q > 16 else (0, 110))]
    if q <= 16:
        imgs += [("noise3", class_image("noise", 3)), ("noise5", class_image("noise", 5)), ("blocks2", class_image("blocks", 2))]
    return imgs


def masked_sha(nhw, pad):
    """sha256 of a .nhw file with the bytes at `pad` (the stock binary's un-initialised positions) set to zero"""
    b = bytearray(nhw)
    for i in pad:
        b[i] = 0
    return _sha(bytes(b))


def _parse(key):
    kind, s, q = key.rsplit("_", 2)
    return kind, int(s[1:]), int(q[1:])


def test_generator_matches_python_definition(oracle):
    # SURVEY 8d generator: C restatement == numpy/pure-python definition
    assert np.array_equal(oracle.synth(3), synth_image(3))


def test_supported_range(oracle):
    assert [q for q in range(0, 25) if oracle.supported(q)] == list(range(1, 24))


def test_golden_files_bit_exact(oracle, manifest):
    for key, size in manifest["files"].items():
        kind, seed, q = _parse(key)
        with open(os.path.join(GOLD, "nhw", key + ".nhw"), "rb") as f:
            want = f.read()
        assert len(want) == size
        got = oracle.encode(_image(oracle, kind, seed), q)
        assert got == want, f"{key}: oracle output differs from the reference's .nhw"


def test_golden_hashes(oracle, manifest):
    for key, h in manifest["hashes"].items():
        kind, seed, q = _parse(key)
        got = oracle.encode(_image(oracle, kind, seed), q)
        assert hashlib.sha256(got).hexdigest() == h, key


def test_golden_checkpoints(oracle, manifest):
    # every intermediate plane / stream the reference hands between its translation units
    for key, cps in manifest["checkpoints"].items():
        kind, seed, q = _parse(key)
        _, tr = oracle.encode(_image(oracle, kind, seed), q, trace=True)
        got = [[n, [hashlib.sha1(b).hexdigest()[:16] for b in blobs]] for n, blobs in tr]
        assert [g[0] for g in got] == [c[0] for c in cps], key
        for g, c in zip(got, cps):
            assert g == c, f"{key}: checkpoint {g[0]} differs"


def test_stage_entry_points_consistent(oracle):
    # the stage-level entry points used by the kernel parity tests reproduce the whole-encoder trace
    img = oracle.synth(5)
    _, tr = oracle.encode(img, 20, trace=True)
    t = {}
    for n, b in tr:
        t.setdefault(n, b)
    y, u, v = oracle.color(img, 20)
    assert y.tobytes() == t["downsample_YUV420"][0] and u.tobytes() == t["downsample_YUV420"][1] and v.tobytes() == t["downsample_YUV420"][2]
    y = oracle.prefilter(y, 20)
    assert y.tobytes() == t["pre_processing"][0]
    j, p = oracle.analysis(y, 512, 512, 0)
    assert j.tobytes() == t["wavelet_analysis_512"][0] and p.tobytes() == t["wavelet_analysis_512"][1]


def test_unsupported_quality_is_loud(oracle):
    for q in (0, 24):      # -q0 is accepted by the reference CLI but has no tables downstream
        with pytest.raises(RuntimeError):
            oracle.encode(oracle.synth(0), q)


@pytest.mark.parametrize("q", TRACE_QS)
def test_against_real_reference_trace(oracle, ref_record, q):
    d_or, t_or = oracle.encode(oracle.synth(12), q, trace=True)
    _assert_trace(ref_record["trace"][f"synth_s12_q{q}"], d_or, t_or, f"q{q}")


def test_reference_decoder_accepts_oracle_output(oracle, ref_record):
    """The stock reference decoder (oracle/_ref/nhw-dec) was given the oracle's own q20 file: its BMP is on record; the oracle's decoder
    writes the same BMP from the same file, and that picture is faithful to the input."""
    rec = ref_record["ref_decodes_oracle_file"]
    img = oracle.synth(4)
    nhw = oracle.encode(img, 20)
    assert _sha(nhw) == rec["nhw_sha256"], "the oracle's file is not the one the reference decoder was given"
    px, q = oracle.decode(nhw)
    bmp = oracle.bmp_header() + px.tobytes()
    assert q == 20 and _sha(bmp) == rec["bmp_sha256"], "the reference decoder's BMP differs"
    out = np.frombuffer(bmp[54:], np.uint8).reshape(512, 512, 3).astype(int)
    mse = ((out - img.astype(int)) ** 2).mean()
    assert 10 * np.log10(255 ** 2 / mse) > 30  # a q20 decode is a faithful picture of the input


@pytest.mark.parametrize("q", COLOUR_QS)
def test_colour_below_q17_against_reference(oracle, ref_record, q):
    """Row a1 below q17 (integer BT.601 scaled by the quality table, colorspace.c:172-214): the oracle's colour stage against the
    reference's first checkpoint."""
    for name, img in colour_images(oracle):
        want = ref_record["colour"][f"{name}_q{q}"]
        assert want[0] == "downsample_YUV420"
        y, u, v = oracle.color(img, q)
        assert [_h16(y.tobytes()), _h16(u.tobytes()), _h16(v.tobytes())] == want[1], f"{name} q{q}"


@pytest.mark.parametrize("q", STOCK_QS)
def test_glibc_oneshot_mode_reproduces_the_stock_binary(oracle, ref_record, q):
    """SURVEY 8(c) vanilla-compat: in NHWO_OOB_GLIBC_ONESHOT mode the oracle equals the stock `gcc -O3` nhw-enc (no shim, one process per
    image) byte for byte, except at the header-locatable positions that binary itself leaves un-initialised.  (In the default canonical
    mode the two differ in thousands of bytes at q >= 20, and on white noise below quality 14 even in the file length.)
    The stock binary's files are on record as their length, their un-initialised positions and the sha256 of the rest."""
    oracle.set_oob_mode(True)
    try:
        for seed, img in stock_images(oracle, q):
            stock = ref_record["stock"][f"q{q}"][seed]
            got = oracle.encode(img, q)
            assert len(got) == stock["len"], (q, seed)
            assert masked_sha(got, stock["pad"]) == stock["masked_sha256"], f"q{q} seed {seed}: bytes differ outside the un-initialised positions"
    finally:
        oracle.set_oob_mode(False)


@pytest.mark.parametrize("kind", HARD_KINDS)
def test_low_quality_hard_classes_against_real_reference(oracle, ref_record, kind):
    """Quality 1..16 on the input classes that drive the rationed pre-filter, the LL2 smoothing and the coders through their rare
    branches; every checkpoint and the file."""
    img = class_image(kind, 3)
    for q in HARD_QS:
        d_or, t_or = oracle.encode(img, q, trace=True)
        _assert_trace(ref_record["trace"][f"{kind}_s3_q{q}"], d_or, t_or, f"{kind} q{q}")


def test_code_book_overflow_is_the_reference_exit(oracle, ref_record):
    """compress_pixel.c:234,270,271: the reference calls exit(-1) when the packetiser's code book does not fit.  A busy synthetic class image
    (found by tools/dev/gpu_fuzz_classes.py, seed 50431) does that from quality 17 on and encodes at 16: the oracle reports NHWO_E_CODEBOOK (-2)
    exactly where the reference exits.  On record: the reference's file's sha256 at each quality, null where it exited with -1."""
    from gpu_fuzz_classes import make
    rec = ref_record["codebook"]
    img = make(CODEBOOK_SEED)
    assert _sha(img.tobytes()) == rec["image_sha256"], "the fuzz generator no longer makes the recorded picture"
    for q in CODEBOOK_QS:
        want = rec["nhw_sha256"][str(q)]
        try:
            got = oracle.encode(img, q)
        except RuntimeError as ex:
            assert "rc=-2" in str(ex)
            got = None
        assert (got is None) == (want is None), q
        if got is not None:
            assert _sha(got) == want, q
    assert oracle.encode(img, 16) and got is None
