"""The decoder on files no encoder writes: long code books, books at the 708-byte and 354-entry caps, short side
strings, position lists at their caps, streams that end early, damaged headers.  tests/nhw_surgery.py builds the fixed list of cases from four
golden files; the oracle, built with AddressSanitizer and UBSan, says for each whether it is defined (and what its pixels are), refused, or
undefined (the oracle itself reads outside a buffer: such a case has no expectation and is left out of the GPU lists).

CPU (-m "not gpu"): the layout reader / writer round trip, the classification and its two conditions, tests/golden/dec/surgery.json reproduced.
GPU (-m gpu): every defined case bit-exact and every refused case NHW_E_FORMAT, next to golden files that must stay exact -- in mixed batches,
under forced slice orders, on a handle that has just decoded dense files, at half and quarter scale, and as a tile of a .nhwp container.
"""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from tests import nhw_surgery as S
from tests.dec_stages import dec_batch
from tests.support import CANARY, device_arena

NHW_E_FORMAT = -6
NEIGHBOURS = S.NEIGHBOURS
sha = lambda b: hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def record():
    return S.load_record()[0]


@pytest.fixture(scope="module")
def neighbours():
    return S.load_record()[1]


@pytest.fixture(scope="module")
def dec_manifest():
    with open(os.path.join(S.GOLD, "manifest.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- CPU
def test_layout_round_trip_on_every_golden(dec_manifest):
    names = sorted(n for n in os.listdir(S.GOLD) if n.endswith(".nhw"))
    assert set(names) == set(dec_manifest) and {dec_manifest[n]["quality"] for n in names} == set(range(1, 24))
    for n in names:
        data = S.golden(n)
        f = S.read(data)
        assert f.q == dec_manifest[n]["quality"] and f.tail == b""
        assert S.write(f) == data, n
        assert S.section_ends(f)["packet2"] == len(data)
        assert S.write(f, **S.write_fields(f)) == data, f"{n}: explicit lengths"


def test_prefix_code_is_complete():
    """Every 20-bit pattern is headed by one of the 290 code words (Kraft sum 1): 'no code word matches' (rank -1 in next_rank / code_at) cannot
    happen, so no file can be built for that refusal"""
    v = np.arange(1 << 20, dtype=np.int64)
    hit = np.zeros(1 << 20, bool)
    kraft = 0.0
    for first, ln, count in S.RUNS:
        p = v >> (20 - ln)
        m = (p >= first) & (p < first + count)
        assert not (hit & m).any(), "two code words head one pattern: not a prefix code"
        hit |= m
        kraft += count / (1 << ln)
    assert hit.all() and kraft == 1.0
    assert sum(c for _, _, c in S.RUNS) == 290
    assert all(S.rank_of(S.word_of(r)[0] << (20 - S.word_of(r)[1])) == (r, S.word_of(r)[1]) for r in range(290))


def test_cases_reproduce_the_record(record):
    cs = S.cases()
    assert {n for n, *_ in cs} == set(record) and len(cs) == len(record)
    for name, group, data, cap in cs:
        r = record[name]
        assert (r["group"], r.get("gpu_cap"), r["bytes"], r["nhw_sha256"]) == (group, cap, len(data), sha(data)), name
        assert len(data) < S.OUT_STRIDE
    # the caps are only claimed for files the oracle takes, and only by the cap cases of group B
    assert {n for n, r in record.items() if r.get("gpu_cap")} == {"q23_res1_bits_over_cap", "q23_res3_bits_over_cap", "q23_res5_bits_over_cap",
                                                                  "q23_res6_bits_over_cap", f"data2_{S.PK_WORDS - 7}"}
    assert all(r["class"] == "defined" and r["group"] == "B" for r in record.values() if r.get("gpu_cap"))


def test_oracle_classifies_every_case_under_the_sanitizers(record, oracle, tmp_path):
    exe = S.build_asan()
    if exe is None:
        pytest.skip("this machine's compiler cannot build oracle/_asan/nhwo_dec_asan (-fsanitize=address,undefined)")
    cs, res = S.classify_all(exe, str(tmp_path))
    undefined = [n for (n, *_), (cls, _, _) in zip(cs, res) if cls == "undefined"]
    print(f"{len(cs)} cases; undefined (left out of the GPU lists): {undefined}")
    for (name, group, data, cap), (cls, q, px) in zip(cs, res):
        assert group != "A" or cls == "defined", f"{name}: a group A case must be defined, the oracle says {cls}: {px if cls == 'undefined' else ''}"
        r = record[name]
        assert r["class"] == cls, f"{name}: recorded {r['class']}, now {cls}"
        if cls == "defined":
            assert (r["quality"], r["pixels_sha256"]) == (q, sha(px)), name
    assert 10 * len(undefined) <= len(cs), f"{len(undefined)} of {len(cs)} cases are undefined"
    # the plain build of the oracle agrees with the sanitizer build on one case of every kind
    for name in ("long_book1_2300_edge", "q20_packet1_middle_word_ones", "book2_708_and_12_dropped_tree_end_65535", "q23_res6_at_cap", "last_cell_2_word132", "q10_packet1_minus_3"):
        data = next(d for n, _, d, _ in cs if n == name)
        got, q = oracle.decode(data)
        assert (record[name]["quality"], record[name]["pixels_sha256"]) == (q, sha(got.tobytes())), name
    for name in ("q20_packet1_minus_3", "book1_rank0_254_half_stream", "book1_expands_to_709"):
        with pytest.raises(RuntimeError):
            oracle.decode(next(d for n, _, d, _ in cs if n == name))


def test_no_golden_reads_behind_its_ll_word_string():
    """the oracle reads 0 behind ll_word (as it does behind the sign and selection strings); no file an encoder wrote gets there: every golden
    of q > 15 holds exactly one byte for every verbatim token of its luma LL2 walk"""
    names = [n for n in sorted(os.listdir(S.GOLD)) if n.endswith(".nhw")]
    fs = [S.read(S.golden(n)) for n in names]
    assert sum(f.q > 15 for f in fs) >= 8
    assert all(S.ll_verbatim_tokens(f) == len(f.s["llword"]) for f in fs if f.q > 15)
    assert sum(S.ll_verbatim_tokens(f) > 100 for f in fs if f.q > 15) >= 8


def test_padded_books_and_slack_decode_as_the_file_they_were_made_from(record, oracle):
    """group A's cases that add only what expands to nothing, or what is dropped: the recorded pixels are the golden file's own"""
    same = [n for n in record if n.startswith(("long_", "slack_", "book1_ends", "book2_ends", "book1_expands_to_707", "book1_expands_to_708", "book1_708_and", "book2_708_and",
                                              "book2_expands_to_708", "book2_dropped", "q01_slack", "q01_book1_ends"))]
    assert len(same) > 45
    want = {k: sha(oracle.decode(S.golden(k))[0].tobytes()) for k in ("q20_0.nhw", "q10_0.nhw", "q23_0.nhw", "q01_0.nhw")}
    for n in same:
        base = "q01_0.nhw" if "q01" in n else "q23_0.nhw" if "q23" in n else "q10_0.nhw" if n.startswith(("long_book2", "book2_ends")) else "q20_0.nhw"
        assert record[n]["class"] == "defined" and record[n]["pixels_sha256"] == want[base], n


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=160)
    yield d
    d.close()


def _batches(record):
    """(defined, refused): lists of (name, bytes, expectation or None for a neighbour) with a golden file in front, behind and after every
    eighth case.  'refused' is what the GPU decoder must refuse: what the oracle refuses and the cap cases."""
    cs = {n: d for n, _, d, _ in S.cases()}
    out = []
    for want_refused in (False, True):
        names = [n for n, r in record.items() if r["class"] != "undefined" and (r["class"] == "refused" or bool(r.get("gpu_cap"))) == want_refused]
        names.sort(key=list(cs).index)
        items = [(NEIGHBOURS[0], S.golden(NEIGHBOURS[0]), None)]
        for k, n in enumerate(names):
            items.append((n, cs[n], record[n]))
            if k % 8 == 7:
                g = NEIGHBOURS[(k // 8 + 1) % len(NEIGHBOURS)]
                items.append((g, S.golden(g), None))
        items.append((NEIGHBOURS[1], S.golden(NEIGHBOURS[1]), None))
        out.append(items)
    return out


def _check(items, px, status, quality, dec_manifest, hdr, what):
    bad = []
    for i, (name, data, r) in enumerate(items):
        if r is None:                                              # a neighbour: the golden file's own BMP digest
            ok = status[i] == 0 and quality[i] == dec_manifest[name]["quality"] and sha(hdr + px[i].tobytes()) == dec_manifest[name]["bmp_sha256"]
        elif r["class"] == "defined" and not r.get("gpu_cap"):
            ok = status[i] == 0 and quality[i] == r["quality"] and sha(px[i].tobytes()) == r["pixels_sha256"]
        else:
            ok = status[i] == NHW_E_FORMAT
        if not ok:
            bad.append((i, name, int(status[i])))
    assert not bad, f"{what}: (slot, file, status) {bad[:12]} of {len(items)}"


def _mode(dec, mode):
    assert dec.lib.nhw_dec_debug_slice_order(dec.h, mode) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gpu_defined_cases_one_mixed_batch(dec, record, dec_manifest, mode):
    items = _batches(record)[0]
    files = [d for _, d, _ in items]
    assert 60 < len(files) <= dec.max_batch
    hdr = dec.bmp_header()
    _mode(dec, mode)
    try:
        px, st, qq = dec_batch(dec, files)
        _check(items, px, st, qq, dec_manifest, hdr, f"nhw_dec_batch, slice order {mode}")
        if mode == 0:
            px2, q2 = dec.decode(files)
            _check(items, px2, np.zeros(len(files), np.int32), q2, dec_manifest, hdr, "Decoder.decode")
    finally:
        _mode(dec, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gpu_refused_cases_one_mixed_batch(dec, record, dec_manifest, mode):
    """NHW_E_FORMAT for every file the oracle refuses and for the cap cases (never 'either'); the golden files between them exact.  The header
    promises nothing about a refused file's slot of a full-size decode, so nothing is asserted about it (the scaled calls do: see below)."""
    items = _batches(record)[1]
    files = [d for _, d, _ in items]
    assert 60 < len(files) <= dec.max_batch
    _mode(dec, mode)
    try:
        px, st, qq = dec_batch(dec, files)
        _check(items, px, st, qq, dec_manifest, dec.bmp_header(), f"nhw_dec_batch, slice order {mode}")
        if mode == 0:
            import nhwcodec_amd
            with pytest.raises(nhwcodec_amd.NhwError):
                dec.decode(files)
    finally:
        _mode(dec, 0)


@pytest.mark.gpu
def test_gpu_both_batches_on_a_handle_that_just_decoded_dense_files(record, dec_manifest):
    """64 white-noise files at q20 (nearly every cell of the value lists, every group of the detail bands in use) through a Decoder of 64 slots,
    then both batches in chunks of 64 over the same slots: a refused or short file must not pick up what the dense batch left there"""
    import torch
    import nhwcodec_amd as na
    n = 64
    enc = na.Encoder(0, n)
    g = torch.Generator(device="cuda"); g.manual_seed(20260930)
    noise = torch.randint(0, 256, (n, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=g)
    out, sizes, status = enc.encode_device(noise, 20)
    torch.cuda.synchronize()
    ok = status == 0
    assert int(ok.sum()) > n // 2
    enc.close()
    d = na.Decoder(0, n)
    try:
        offs = torch.arange(n, dtype=torch.int64, device="cuda") * na.OUT_STRIDE
        _, st, _ = d.decode_device(out, offs, torch.where(ok, sizes, torch.zeros_like(sizes)))
        torch.cuda.synchronize()
        assert int(st[ok].abs().sum()) == 0
        hdr = d.bmp_header()
        for items, what in zip(_batches(record), ("defined", "refused")):
            px, st, qq = dec_batch(d, [x for _, x, _ in items])
            _check(items, px, st, qq, dec_manifest, hdr, f"{what} cases after a dense batch")
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 4])
def test_gpu_scaled_decode_of_every_case(dec, record, neighbours, scale):
    """decode_scaled_device: status and quality as the full decode's; a defined case equals the scaled definition of DESIGN.md section 14 (the
    digest surgery.json keeps was computed by tests/tensor_cases.py's `expected`); a refused file's bytes are left untouched, as
    include/nhw_hip.h promises for the scaled calls"""
    import torch
    t = 512 // scale
    for items in _batches(record):
        files = [d for _, d, _ in items]
        buf = torch.full((len(files) * 3 * t * t + 4096,), CANARY, dtype=torch.uint8, device="cuda")
        px, st, qq = dec.decode_scaled_device(*device_arena(files), scale, out=buf)
        torch.cuda.synchronize()
        assert bool((buf[len(files) * 3 * t * t:] == CANARY).all())
        px, st, qq = px.cpu().numpy(), st.cpu().numpy(), qq.cpu().numpy()
        bad = []
        for i, (name, data, r) in enumerate(items):
            if r is None:                                          # a neighbour: its own scaled picture, untouched by the files around it
                ok = st[i] == 0 and qq[i] == int(name[1:3]) and sha(px[i].tobytes()) == neighbours[name][f"scale{scale}_sha256"]
            elif r["class"] == "defined" and not r.get("gpu_cap"):
                ok = st[i] == 0 and qq[i] == r["quality"] and sha(px[i].tobytes()) == r[f"scale{scale}_sha256"]
            else:
                ok = st[i] == NHW_E_FORMAT and bool((px[i] == CANARY).all())
            if not ok:
                bad.append((i, name, int(st[i])))
        assert not bad, f"scale {scale}: (slot, file, status) {bad[:12]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["q20_packet1_minus_8", "book1_expands_to_709", "q23_res1_bits_over_cap"])
def test_gpu_container_whose_second_tile_is_refused(dec, record, dec_manifest, case):
    """a 1024 x 512 .nhwp picture of two tiles, the second one a file the decoder refuses: nhw_dec_pictures answers NHW_E_FORMAT and leaves the
    picture's bytes untouched, the good container next to it is exact; a region inside the good tile decodes, one that
    touches the refused tile is NHW_E_FORMAT with its bytes untouched and does not disturb the other (section 13)"""
    import nhwcodec_amd as na
    good, bad_tile = S.golden("q20_0.nhw"), next(d for n, _, d, _ in S.cases() if n == case)
    pack = lambda fs: b"NHWP\x01\0\0\0" + struct.pack("<II", 512 * len(fs), 512) + struct.pack(f"<{len(fs)}I", *[len(f) for f in fs]) + b"".join(fs)
    cons = [pack([good, bad_tile]), pack([good, good])]
    want = dec.decode([good])[0][0]
    assert sha(dec.bmp_header() + want.tobytes()) == dec_manifest["q20_0.nhw"]["bmp_sha256"]
    with pytest.raises(na.NhwError):
        dec.decode_pictures(cons)
    offs = np.zeros(3, np.uint64); offs[1:] = np.cumsum([len(c) for c in cons])
    blob = np.frombuffer(b"".join(cons), np.uint8)
    size = 3 * 1024 * 512
    out_off = np.array([0, size], np.uint64)
    out = np.full(2 * size, CANARY, np.uint8); status = np.full(2, 77, np.int32)
    assert dec.lib.nhw_dec_pictures(dec.h, blob.ctypes.data, offs.ctypes.data, 2, out.ctypes.data, out_off.ctypes.data, status.ctypes.data) == 0
    assert status.tolist() == [NHW_E_FORMAT, 0]
    assert (out[:size] == CANARY).all(), "the refused picture's bytes were written"
    pic = out[size:].reshape(512, 1024, 3)
    assert np.array_equal(pic[:, :512], want) and np.array_equal(pic[:, 512:], want)
    # regions: (container, x, y, w, h)
    rects = np.zeros(3, na.RECT_DTYPE)
    rects[0] = (0, 100, 50, 300, 200); rects[1] = (0, 500, 50, 40, 30); rects[2] = (1, 500, 50, 40, 30)
    sizes = [3 * int(r["width"]) * int(r["height"]) for r in rects]
    r_off = np.zeros(3, np.uint64); r_off[1:] = np.cumsum(sizes)[:-1]
    r_out = np.full(sum(sizes), CANARY, np.uint8); r_st = np.full(3, 77, np.int32)
    assert dec.lib.nhw_dec_regions(dec.h, blob.ctypes.data, offs.ctypes.data, 2, rects.ctypes.data, 3, r_out.ctypes.data, r_off.ctypes.data, r_st.ctypes.data) == 0
    assert r_st.tolist() == [0, NHW_E_FORMAT, 0]
    assert np.array_equal(r_out[:sizes[0]].reshape(200, 300, 3), want[50:250, 100:400])
    assert (r_out[sizes[0]:sizes[0] + sizes[1]] == CANARY).all()
    assert np.array_equal(r_out[sizes[0] + sizes[1]:].reshape(30, 40, 3), pic[50:80, 500:540])
