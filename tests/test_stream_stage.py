"""The stream stage on crafted symbol streams: the Y31 symbol rewrites (k_y31, scan_rewrite_list_par) and the RLE + VLC packetiser (k_final,
pack_part_par / pack_walk_list) behind nhw_stage_stream (include/nhw_hip_debug.h), against the oracle's export of the same stage
(nhwo_stream_stage).  Both are pure functions of the symbol stream; a picture cannot be steered to the edges of their index arithmetic, a
stream can.  The cases, the two alphabets and the device's list format: tests/stream_cases.py.

What pins what:
  * the packetiser of the oracle is pinned to the unmodified wavlts2packet on every case that fits the reference's packet block
    (tests/golden/make_stream_golden.py -> stream_record.json; checked here on the CPU against the record);
  * the rewrites sit in the middle of encode_image and cannot be called alone: for them the oracle's transcription is the reference.  It is
    pinned on pictures by the pre_highres_compression checkpoint (tests/test_oracle.py);
  * the device is compared with the oracle's export (pytest -m gpu): form 0 (k_y31 + k_final from the quantisers' lists) for every case --
    status, packet words, both books, both sign-word arrays, select1/2, size_data1/2, size_book1/2, tree_end, wavelet_type, and the luma lists
    behind Y31 decoded to a dense stream (read behind form 2, k_y31 alone: k_final reuses B_NZS / B_VOFF for the chroma part's map);
    form 1 (k_final alone on lists made from the oracle's rewritten stream) against form 0.
    select1/2 BEFORE packing (the counts the second rewrite leaves) only size two scratch lists in the reference; the device keeps no such
    counts (its lists have a fixed capacity), so they are recorded, not compared.

The alphabets (as counted from nhwo_quantise_luma / nhwo_quantise_chroma): luma 75 non-zero symbols -- the 31 multiples of 8, the marks 121,
122, 125, 126, 127, 129, the 38 escape codes; chroma 73 -- the multiples of 8, 122, 124, 126, 130, the escape codes.  With the six book symbols
the rewrites add, a luma book holds at most 334 entries and a chroma book 327: the `select++` loop (more than 354) is unreachable for
admissible streams, and no case feeds other symbols to reach it.

Capacity: the rule is the device's own (pack_part_par: word0 + last >= 80000): a stream of exactly 80000 packet words is packed, one of
80001 answers NHW_E_SPACE with size 0.  The oracle supplies only the count."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

from tests import stream_cases as sc
from tests.enc_stages import ws_index
from tests.support import ROOT

Q = sc.Q
E_CODEBOOK, E_SPACE = -2, -3


def _ws_text():
    return open(os.path.join(ROOT, "nhwcodec_amd", "csrc", "nhw_ws.h")).read()


def _meta_index():
    """int index of every scalar of NhwMeta (nhw_ws.h)"""
    txt = re.sub(r"/\*.*?\*/", "", _ws_text(), flags=re.S)
    body = txt[txt.index("struct NhwMeta {"):]
    body = body[body.index("{") + 1:body.index("};")]
    at, out = 0, {}
    for typ, names in re.findall(r"(int|NhwPosLens)\s+([^;]+);", body):
        for nm in names.split(","):
            out[nm.strip()] = at
            at += 3 if typ == "NhwPosLens" else 1
    return out, at


META, META_INTS = _meta_index()
B = {k: ws_index(k) for k in ("SCAN", "NZQ", "NZS", "VOFF", "VALS", "CNZQ", "CVALS", "PACKET", "BOOK1", "BOOK2", "SEL1", "SEL2", "META")}
SCALARS = ("select1", "select2", "size_data1", "size_data2", "size_book1", "size_book2", "tree_end", "wavelet_type")


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oraclepy import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def want_batch(name):
    """the cases of a batch and the oracle's answers, made once and shared (read-only) by the tests that need them"""
    if name == "capacity":
        quiet = sc.family("budget")
        cap = sc.capacity_cases(_oracle())
        cases = [c for k, (n, l, c_, w) in enumerate(cap) for c in (quiet[k % len(quiet)], (n, l, c_))] + [quiet[0]]
    else:
        cases = sc.batch(name)
    res = [_oracle().stream_stage(l, c, 80000) for _, l, c in cases]
    for (_, l, c), r in zip(cases, res):
        for a in (l, c) + tuple(r[k] for k in sc.ARRAYS):
            a.setflags(write=False)
    return cases, res


# ------------------------------------------------------------------------------------------------ CPU
def test_alphabets_enter_the_book_and_the_select_loop_is_unreachable():
    """Every symbol a quantiser can write passes book_symbol_ok (the reference would otherwise use its COUNT as a rank), and so do the six the
    rewrites add; 334 and 327 entries at the most, against the 354 the `select++` loop needs.  Every case keeps to the alphabets."""
    o = _oracle()
    assert len(sc.LUMA_ALPHABET) == 75 and len(sc.CHROMA_ALPHABET) == 73
    assert all(o.book_symbol_ok(v) for v in sc.LUMA_ALPHABET + sc.CHROMA_ALPHABET + sc.LUMA_REWRITTEN + (sc.Z,))
    assert not any(o.book_symbol_ok(v) for v in (153, 155, 157, 159, 201))
    assert sc.MAX_LUMA_ENTRIES == 334 and sc.MAX_CHROMA_ENTRIES == 327 and max(sc.MAX_LUMA_ENTRIES, sc.MAX_CHROMA_ENTRIES) <= 354
    for name in list(sc.BATCHES) + ["capacity"]:
        for (n, l, c), r in zip(*want_batch(name)):
            sc.admissible(n, l, c)
            lone, all201 = sc.orphans(r["luma"])
            assert lone == 0 or all201 <= 2, f"{n}: {lone} orphaned 201 of {all201}: their count is their rank"


def test_oracle_stream_export_equals_the_record():
    """nhwo_stream_stage on every case against tests/golden/stream_record.json, whose entries were checked against the unmodified
    wavlts2packet when they were written (every case but the ones of more than 80000 packet words, which would overrun the reference's
    block).  The rewrites cannot be called alone in the reference: for them the oracle's transcription is the reference, pinned on pictures
    by the pre_highres_compression checkpoint."""
    with open(os.path.join(ROOT, "tests", "golden", "stream_record.json")) as f:
        rec = json.load(f)
    o = _oracle()
    cases = sc.all_cases(o)
    assert sorted(n for n, _, _ in cases) == sorted(rec["cases"]) == sorted(rec["reference"])
    bad = [n for n, l, c in cases if sc.digest(o.stream_stage(l, c, 80000)) != rec["cases"][n]]
    assert bad == []
    kinds = list(rec["reference"].values())
    assert kinds.count("equal") > 250 and set(kinds) == {"equal", "exit", "over capacity"}


def test_lists_helpers_are_inverse_to_the_decoding():
    rng = np.random.default_rng(5)
    luma = np.where(rng.random(sc.NL) < 0.2, rng.choice(sc.LUMA_ALPHABET + (132, 133), sc.NL), sc.Z).astype(np.uint8)
    luma[64 * 7 + 61] = 133; luma[64 * 9 + 59] = 132; luma[64 * 11 + 63] = 135
    L = sc.lists_from_rewritten(luma)
    assert np.array_equal(sc.dense_from_lists(L["nzs"], L["voff"], L["vals"]), luma)
    assert (L["voff"][8] >> 29, L["voff"][10] >> 29, L["voff"][12] >> 29) == (2, 0, 4)
    chroma = np.where(rng.random(sc.NC) < 0.3, rng.choice(sc.CHROMA_ALPHABET, sc.NC), sc.Z).astype(np.uint8)
    P = sc.lists_from_streams(luma, chroma)
    maps, fb = P["cnzq"][:Q // 4].view(np.uint64).reshape(16, 64, 2), P["cnzq"][Q // 4:].view(np.uint32)
    got = np.full(sc.NC, sc.Z, np.uint8)
    for F in range(16):                                          # the decoding of test_symbol_list_equals_the_byte_stream
        at = int(fb[F])
        for lane in range(64):
            for half in range(2):
                S = 64 * (lane >> 1) + 16 * (F >> 2) + 4 * (F & 3) + 2 * (lane & 1) + half
                b = np.unpackbits(maps[F, lane, half:half + 1].view(np.uint8), bitorder="little").astype(bool)
                n = int(b.sum())
                got[64 * S:64 * S + 64][b] = P["cvals"][at:at + n]
                at += n
    assert np.array_equal(got, chroma)
    fbase = P["nzq"][32768:].view(np.uint32)
    maps = P["nzq"][:32768].view(np.uint64).reshape(32, 128)
    got = np.full(sc.NL, sc.Z, np.uint8)
    at = 0
    for f in range(32):
        assert at == fbase[f]
        for strip in range(128):
            b = np.unpackbits(maps[f, strip:strip + 1].view(np.uint8), bitorder="little").astype(bool)
            g = strip * 32 + f
            got[64 * g:64 * g + 64][b] = P["vals"][at:at + int(b.sum())]
            at += int(b.sum())
    assert at == fbase[32] and np.array_equal(got, luma)


def test_code_book_cases_sit_on_the_290_entry_limit():
    """289 and 290 entries are packed; 291 are packed only by the luma part with the zero symbol at the top rank (the zone), and answer
    NHWO_E_CODEBOOK otherwise (compress_pixel.c:269-271): the oracle's status says that the builders count right.  Entries of equal weight
    keep their order; with the zone on, wavelet_type is 0."""
    cases, res = want_batch("books")
    seen = 0
    for (n, _, _), r in zip(cases, res):
        m = re.match(r"book: book (luma|chroma) k(\d+) zero (\w+)", n)
        if not m:
            continue
        part, k, zero = m.group(1), int(m.group(2)), m.group(3)
        ok = k <= 290 or (part == "luma" and zero == "top")
        assert r["status"] == (0 if ok else E_CODEBOOK), n
        if ok and part == "luma":
            assert r["wavelet_type"] == (0 if zero == "top" else 4), n
        if ok and part == "chroma":
            assert r["tree_end"] == k + (253 if k > 261 else k - 8), n      # a run entry takes two bytes
        seen += 1
    assert seen == 36


def test_stale_cases_read_the_bytes_the_luma_book_left():
    """The chroma book of a stale-bytes case depends on the luma part: with the long luma book the run of 128s that closes the chroma table
    reads on into the luma table's byte 128 (a run LENGTH there), with the short one into zeros."""
    o = _oracle()
    long_, short = sc.stale_streams(True), sc.stale_streams(False)
    differ = 0
    for (n, l, c), (_, l2, _) in zip(long_, short):
        a, b = o.stream_stage(l, c, 80000), o.stream_stage(l2, c, 80000)
        assert a["status"] == b["status"] == 0 and a["tree_end"] == b["tree_end"]
        assert a["size_book1"] > a["tree_end"] > b["size_book1"], n      # the luma book longer / shorter than the chroma table
        if not np.array_equal(a["book2"], b["book2"]):
            assert a["book2"][-2] == 128 and a["book2"][-1] == b["book2"][-1] + 1, n
            differ += 1
    assert differ >= 4


def test_capacity_cases_sit_on_both_sides_of_80000_words():
    cases, res = want_batch("capacity")
    words = sorted(r["words"] for (n, _, _), r in zip(cases, res) if n.startswith("capacity"))
    assert {79999, 80000, 80001, 80002} <= set(words), words


# ------------------------------------------------------------------------------------------------ GPU
class Stage:
    def __init__(self, n):
        import nhwcodec_amd
        self.n = n
        self.e = nhwcodec_amd.Encoder(0, max_batch=n)

    def whole_batch(self, q):
        import torch
        bgr = self.e.synth_device(self.n, seed_base=88000 + q)
        self.e.encode_device(bgr, q)
        torch.cuda.synchronize()

    def read(self, buf, i, nbytes, dt=np.uint8):
        out = np.empty(nbytes, np.uint8)
        assert self.e.lib.nhw_debug_read(self.e.h, B[buf], i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(nbytes)) == 0
        return out.view(dt)

    def write(self, buf, i, a):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            assert self.e.lib.nhw_debug_write(self.e.h, B[buf], i, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0, buf

    def run(self, form):
        n = self.n
        status, sizes = np.full(n, 99, np.int32), np.full(n, 99, np.uint32)
        rc = self.e.lib.nhw_stage_stream(self.e.h, n, form, ctypes.c_void_p(status.ctypes.data), ctypes.c_void_p(sizes.ctypes.data), None)
        assert rc == 0, "nhw_stage_stream"
        out = []
        for i in range(n):
            r = dict(status=int(status[i]), size=int(sizes[i]))
            if r["status"] == 0:
                m = self.read("META", i, 4 * META_INTS, np.int32)
                r.update({k: int(m[META[k]]) for k in SCALARS})
                r["packet"] = self.read("PACKET", i, 4 * min(max(r["size_data2"], 0), 80000), np.uint32)
                r["book1"] = self.read("BOOK1", i, min(max(r["size_book1"], 0), 708))
                r["book2"] = self.read("BOOK2", i, min(max(r["size_book2"], 0), 708))
                r["sel_word1"] = self.read("SEL1", i, min(max(r["select1"], 0), 32776))
                r["sel_word2"] = self.read("SEL2", i, min(max(r["select2"], 0), 32776))
            out.append(r)
        return out

    def form0(self, cases):
        """-> form 0's results, with the luma lists behind Y31 as a dense stream.  k_final puts the chroma part's map into B_NZS / B_VOFF, so
        Y31's lists are read behind form 2 (k_y31 alone); it rewrites the values in place, so they are written again for form 0."""
        lists = [sc.lists_from_streams(l, c) for _, l, c in cases]
        for i, L in enumerate(lists):
            self.write("NZQ", i, L["nzq"]); self.write("VALS", i, L["vals"]); self.write("CNZQ", i, L["cnzq"]); self.write("CVALS", i, L["cvals"])
        assert self.e.lib.nhw_stage_stream(self.e.h, self.n, 2, None, None, None) == 0, "nhw_stage_stream, form 2"
        luma = [sc.dense_from_lists(self.read("NZS", i, 4 * Q // 8, np.uint64), self.read("VOFF", i, 4 * Q // 16, np.uint32), self.read("VALS", i, 4 * Q))
                for i in range(self.n)]
        for i, L in enumerate(lists):
            self.write("VALS", i, L["vals"])
        got = self.run(0)
        for r, l in zip(got, luma):
            r["luma"] = l
        return got

    def form1(self, cases, want):
        for i, ((_, l, c), w) in enumerate(zip(cases, want)):
            L = sc.lists_from_rewritten(w["luma"])
            self.write("NZS", i, L["nzs"]); self.write("VOFF", i, L["voff"]); self.write("VALS", i, L["vals"])
        return self.run(1)


def same(tag, name, g, w, keys):
    bad = [k for k in keys if not (np.array_equal(g[k], w[k]) if isinstance(w[k], np.ndarray) else g[k] == w[k])]
    assert not bad, f"{tag}, case '{name}': {bad} differ" + "".join(
        f"\n  {k}: first at {np.flatnonzero(np.asarray(g[k][:min(len(g[k]), len(w[k]))]) != np.asarray(w[k][:min(len(g[k]), len(w[k]))]))[:4].tolist()} of {len(g[k])} / {len(w[k])}"
        if isinstance(w[k], np.ndarray) else f"\n  {k}: {g[k]} / {w[k]}" for k in bad)


ARRAYS = ("packet", "book1", "book2", "sel_word1", "sel_word2")


def check_against_oracle(tag, cases, got, want):
    for (name, _, _), g, w in zip(cases, got, want):
        if "luma" in g:                                          # Y31 ran, whatever the packetiser says
            same(tag, name, g, w, ("luma",))
        if w["words"] > 80000:                                   # the device's own rule: the packet block holds 80000 words
            assert (g["status"], g["size"]) == (E_SPACE, 0), f"{tag}, case '{name}' ({w['words']} words): status {g['status']} size {g['size']}"
            continue
        assert g["status"] == w["status"], f"{tag}, case '{name}': status {g['status']}, the oracle's {w['status']}"
        if w["status"]:
            assert g["size"] == 0, (tag, name)
            continue
        assert g["size"] > 4 * w["size_data2"], (tag, name)
        same(tag, name, g, w, SCALARS + ARRAYS)


def check_batch(name, q):
    cases, want = want_batch(name)
    st = Stage(len(cases))
    try:
        st.whole_batch(q)
        got0 = st.form0(cases)
        check_against_oracle(f"q{q} batch, form 0 against the oracle", cases, got0, want)
        got1 = st.form1(cases, want)
        for (cname, _, _), a, b in zip(cases, got1, got0):
            assert (a["status"], a["size"]) == (b["status"], b["size"]), f"form 1 against form 0, case '{cname}'"
            if a["status"] == 0:
                same("form 1 against form 0", cname, a, b, SCALARS + ARRAYS)
    finally:
        st.e.close()
    return cases, want, got0


@pytest.mark.gpu
@pytest.mark.parametrize("q", [20, 10])
def test_helper_lists_are_the_production_format(q):
    """Six pictures, the driver stopped behind Y31 and behind V's quantiser (debug mode writes the byte stream next to the lists): the lists
    rebuilt from B_SCAN with lists_from_streams / lists_from_rewritten equal what the device wrote, byte for byte -- so the inputs of
    every test below are in the production format.  (Y31 clears the first and the last four luma symbols in the map and leaves their values
    in the list, dead: they are put back into the byte stream from the device's list before the comparison.)"""
    import torch
    st = Stage(6)
    e = st.e
    luma_stage = 13 if q > 12 else 11
    try:
        bgr = e.synth_device(6, seed_base=91000 + q)
        e.lib.nhw_debug_stop_after(e.h, luma_stage)
        e.encode_device(bgr, q)
        torch.cuda.synchronize()
        for i in range(6):
            dense = st.read("SCAN", i, 4 * Q).copy()
            nzq, vals = st.read("NZQ", i, 32768 + 132), st.read("VALS", i, 4 * Q)
            maps = nzq[:32768].view(np.uint64)
            total = int(nzq[32768:].view(np.uint32)[32])
            head = [k for k in range(4) if (int(maps[0]) >> k) & 1]
            tail = [k for k in range(60, 64) if (int(maps[4095]) >> k) & 1]
            assert (dense[:4] == sc.Z).all() and (dense[-4:] == sc.Z).all()
            dense_q = dense.copy()
            dense_q[head] = vals[:len(head)]
            dense_q[[4 * Q - 64 + k for k in tail]] = vals[total - len(tail):total]
            L = sc.lists_from_streams(dense_q, sc.zc())
            assert np.array_equal(L["nzq"], nzq), f"q{q} image {i}: the luma map or its fbase table"
            assert total == L["vals"].size and np.array_equal(L["vals"], vals[:total]), f"q{q} image {i}: the luma values"
            R = sc.lists_from_rewritten(dense)
            nzs, voff = st.read("NZS", i, 4 * Q // 8, np.uint64), st.read("VOFF", i, 4 * Q // 16, np.uint32)
            assert np.array_equal(R["nzs"], nzs), f"q{q} image {i}: the map in stream order"
            assert np.array_equal(voff >> 29, R["voff"] >> 29), f"q{q} image {i}: the skip bits"
            assert np.array_equal((voff & 0x1FFFFFFF) - len(head), R["voff"] & 0x1FFFFFFF), f"q{q} image {i}: the value offsets"
            assert np.array_equal(sc.dense_from_lists(nzs, voff, vals), dense)
        e.lib.nhw_debug_stop_after(e.h, luma_stage + 24)
        e.encode_device(bgr, q)
        torch.cuda.synchronize()
        for i in range(6):
            chroma = st.read("SCAN", i, 6 * Q)[4 * Q:]
            cnzq, cvals = st.read("CNZQ", i, Q // 4 + 80), st.read("CVALS", i, 2 * Q)
            L = sc.lists_from_streams(sc.zl(), chroma)
            assert np.array_equal(L["cnzq"], cnzq), f"q{q} image {i}: the chroma map or its cfbase table"
            tot = L["cnzq"][Q // 4:].view(np.uint32)[16:20]
            for wv in range(4):
                assert np.array_equal(L["cvals"][32768 * wv:32768 * wv + tot[wv]], cvals[32768 * wv:32768 * wv + tot[wv]]), f"q{q} image {i}: the values of wavefront {wv}"
            assert (chroma != sc.Z).any()
    finally:
        e.lib.nhw_debug_stop_after(e.h, 0)
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.BATCHES))
def test_stream_stage_equals_the_oracle(name):
    """Every case of a batch behind a q20 batch: form 0 against the oracle's export, the lists behind Y31 against its rewritten stream, form 1
    against form 0.  One hook call a form."""
    check_batch(name, 20)


@pytest.mark.gpu
def test_random_sweep_behind_a_q10_batch():
    """The results do not depend on which batch came before: the sweep again, behind a q10 batch."""
    check_batch("sweep", 10)


@pytest.mark.gpu
def test_capacity_at_the_exact_word():
    """Dense streams cut (on the CPU, by the oracle's count) to 79997 .. 80003 and 80010 packet words, a quiet stream between every two of them.
    Up to 80000 words the device equals the oracle; from 80001 on the image reports NHW_E_SPACE with size 0; the images before and after
    it are packed as ever.  The rule pinned is the device's (word0 + last >= 80000)."""
    cases, want, got = check_batch("capacity", 20)
    seen = {w["words"]: g["status"] for (n, _, _), w, g in zip(cases, want, got) if n.startswith("capacity")}
    assert seen[80000] == 0 and seen[80001] == E_SPACE, seen
    assert all(g["status"] == 0 for (n, _, _), g in zip(cases, got) if not n.startswith("capacity"))
