"""The packetiser's chroma part as a kernel of its own (k_pack_chroma, nhw_tail.hip; pack_chroma_par / final_phase_par, nhw_tail_par.h).

The chroma part's words and ranked book entries are made by k_pack_chroma from the chroma lists alone, into memory of its own (B_CPACK,
B_CPACKET); k_final packs the luma part, makes both books, puts the chroma words behind the luma words and writes the file.  The forked
order launches the chroma kernel behind V's quantiser, beside Z1 on the LL coder's stream (NHW_PACK_FORK=1: behind Z1 on the chroma stream),
every other order directly in front of k_final; NHW_PACK_FORK=0 does the latter in the forked order too.  What is checked:

  * whole files against the oracle under every launch order that places the kernel differently, on pictures whose chroma part is empty
    (grey), dense (saturated noise) and ordinary (generator seeds);
  * one handle across a dense, an empty and a dense batch: a word count, words or book entries left by the batch before would show;
  * what coupled the two parts while one workgroup ran both, through nhw_stage_stream (forms 0 and 1) on crafted streams
    (tests/stream_cases.py): book 2's collapse reading on into book 1's bytes; the capacity rule; which part's status is reported; the
    sign symbols of a chroma stream, which must not reach the luma part's sign words.

The capacity rule, `word0 + last >= 80000`, is applied by k_final from the chroma part's total.  The cases put the 80000th word into the
chroma part (79999 and 80000 words are packed -- 80000 is the boundary: the last word of the block --, 80001 answers NHW_E_SPACE).  No
stream puts it into the LUMA part: with all 100 symbols that enter a book and take one position used equally often -- the longest codes a
part can average, 9.5 bits a symbol -- the 262144 luma symbols take 77532 words (the oracle's count, asserted below), so the luma part
always fits and the rule can only fire on the sum.  The case that comes nearest is included: that densest luma part with a chroma part
cut to 80000 and to 80001 words in all, where word0 is 77532 and the chroma part a fortieth of the file.

Status order (the luma part's, the chroma part's, the capacity rule's, the container's): both code-book failures answer NHW_E_CODEBOOK, so
the order shows where a chroma book failure meets a packet that would not fit: NHW_E_CODEBOOK, not NHW_E_SPACE."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import stream_cases as sc
from tests.enc_stages import ws_index
from tests.support import ROOT

Q = sc.Q
E_CODEBOOK, E_SPACE = -2, -3
QUALITIES = (1, 10, 17, 20, 21, 23)
SCALARS = ("select1", "select2", "size_data1", "size_data2", "size_book1", "size_book2", "tree_end", "wavelet_type")
ARRAYS = ("packet", "book1", "book2", "sel_word1", "sel_word2")
B = {k: ws_index(k) for k in ("NZQ", "NZS", "VOFF", "VALS", "CNZQ", "CVALS", "PACKET", "BOOK1", "BOOK2", "SEL1", "SEL2", "META")}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oraclepy import Oracle
    return Oracle()


def _meta_index():
    """int index of every scalar of NhwMeta (nhw_ws.h)"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "nhwcodec_amd", "csrc", "nhw_ws.h")).read(), flags=re.S)
    body = txt[txt.index("struct NhwMeta {"):]
    body = body[body.index("{") + 1:body.index("};")]
    at, out = 0, {}
    for typ, names in re.findall(r"(int|NhwPosLens)\s+([^;]+);", body):
        for nm in names.split(","):
            out[nm.strip()] = at
            at += 3 if typ == "NhwPosLens" else 1
    return out, at


META, META_INTS = _meta_index()


# ------------------------------------------------------------------------------------------------ pictures
def grey():
    return np.full((512, 512, 3), 128, np.uint8)                 # no chroma detail: an empty chroma part


def saturated(seed):
    return np.random.default_rng(seed).choice(np.array([0, 255], np.uint8), (512, 512, 3))   # every chroma cell loud: a dense chroma part


@functools.lru_cache(maxsize=None)
def pictures():
    imgs = np.stack([_oracle().synth(s) for s in (0, 7, 31, 1234, 61000, 88020)] + [grey(), saturated(5)])
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def want_files(kind, q):
    """the oracle's files, made once and shared by the tests that need them"""
    imgs = {"pictures": pictures, "dense": lambda: np.stack([saturated(s) for s in range(11, 15)]), "grey": lambda: np.stack([grey()] * 4)}[kind]()
    return imgs, tuple(_oracle().encode(im, q) for im in imgs)


def encoder(n, env=None, slice_order=0):
    """a handle made under the schedule switches of `env` (they are read when a handle is made)"""
    import nhwcodec_amd
    env = env or {}
    os.environ.update(env)
    try:
        e = nhwcodec_amd.Encoder(0, max_batch=n)
    finally:
        for k in env:
            del os.environ[k]
    if slice_order:
        assert e.lib.nhw_debug_slice_order(e.h, slice_order) == 0
    return e


ORDERS = {"default": ({}, 0), "NHW_PACK_FORK=0": ({"NHW_PACK_FORK": "0"}, 0), "NHW_PACK_FORK=1": ({"NHW_PACK_FORK": "1"}, 0),
          "NHW_CHROMA_FORK=0": ({"NHW_CHROMA_FORK": "0"}, 0), "slice order 1": ({}, 1), "slice order 2": ({}, 2)}


def test_oracle_chroma_parts_are_empty_dense_and_ordinary():
    """What the pictures are chosen for, by the oracle's own files (size_data1 / size_data2 at bytes 6 and 10 of the header): the grey picture's
    chroma part holds no symbol -- 131071 zeros, 516 runs of 254 and one of 7 at two bits each: 33 words --, the saturated one's takes
    thousands of words, a generator picture's tens."""
    for q in (1, 20):
        imgs, files = want_files("pictures", q)
        words = [int.from_bytes(f[10:14], "little") - int.from_bytes(f[6:10], "little") for f in files]
        assert words[6] == 33 and words[7] > 2000 and all(33 < w < 200 for w in words[:6]), words


@pytest.mark.gpu
@pytest.mark.parametrize("order", list(ORDERS))
def test_whole_files_equal_the_oracle(order):
    env, slice_order = ORDERS[order]
    e = encoder(8, env, slice_order)
    try:
        for q in QUALITIES:
            imgs, want = want_files("pictures", q)
            got = e.encode(imgs, q)
            bad = [i for i in range(len(want)) if got[i] != want[i]]
            assert bad == [], f"{order}, q{q}: pictures {bad} differ from the oracle's files"
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["default", "NHW_PACK_FORK=0", "NHW_CHROMA_FORK=0"])
def test_one_handle_dense_then_empty_then_dense(order):
    """Nothing of a batch's chroma part outlives it: its word count, its words and its book entries are written again by every batch."""
    e = encoder(4, ORDERS[order][0])
    try:
        for q in (20, 23, 10):
            for kind in ("dense", "grey", "dense"):
                imgs, want = want_files(kind, q)
                assert list(e.encode(imgs, q)) == list(want), f"{order}, q{q}, the {kind} batch"
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ the couplings, on crafted streams
def densest_luma():
    ok = [v for v in range(256) if _oracle().book_symbol_ok(v) and v not in (sc.Z, 132, 133, 134, 135)]
    assert len(ok) == 100
    return np.random.default_rng(1).choice(ok, sc.NL).astype(np.uint8)


def cut_to(luma, chroma, targets):
    """chroma cut short (trim_chroma) until both parts take `target` packet words, by the oracle's count"""
    words = lambda m: _oracle().stream_stage(luma, sc.trim_chroma(chroma, m), 1)["words"]
    lo, hi = 0, sc.NC
    assert words(lo) < min(targets) < max(targets) < words(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if words(mid) < min(targets) else (lo, mid)
    found, m = {}, lo
    while len(found) < len(targets) and words(m) <= max(targets):
        if words(m) in targets:
            found.setdefault(words(m), m)
        m += 1
    assert sorted(found) == sorted(targets), (sorted(found), targets)
    return [sc.trim_chroma(chroma, found[w]) for w in targets]


def sign_case():
    """A luma stream whose second rewrite leaves sign symbols (153 / 155 and 157 / 159: the rewrite-2 case with the most of them), next to a
    chroma stream that holds the same four symbols: fewer than the luma part's, as the reference sizes its two lists by the luma counts."""
    o = _oracle()
    name, luma, _ = max(sc.family("rewrite2"), key=lambda c: min(o.stream_stage(c[1], c[2], 80000)[k] for k in ("select1_pre", "select2_pre")))
    rng = np.random.default_rng(3)
    chroma = np.where(rng.random(sc.NC) < 0.3, rng.choice(sc.CHROMA_ALPHABET, sc.NC), sc.Z).astype(np.uint8)
    chroma[rng.choice(sc.NC - 8, 16, replace=False)] = np.resize(np.array([153, 155, 157, 159], np.uint8), 16)
    return ("sign symbols in both parts (" + name + ")", luma, chroma)


@functools.lru_cache(maxsize=None)
def coupling_cases():
    """-> (cases, the oracle's answers, the status each case is meant to give), made once"""
    o = _oracle()
    cases, intent = [], []
    for c in sc.stale_streams(True) + sc.stale_streams(False):
        cases.append(c); intent.append(0)
    for name, l, c, w in sc.capacity_cases(o, (79999, 80000, 80001)):
        cases.append((name + ", the 80000th word in the chroma part", l, c)); intent.append(E_SPACE if w > 80000 else 0)
    dl = densest_luma()
    for w, c in zip((80000, 80001), cut_to(dl, sc.dense_pair(77)[1], (80000, 80001))):
        cases.append((f"capacity {w} words behind the densest luma part", dl, c)); intent.append(E_SPACE if w > 80000 else 0)
    quiet_l, quiet_c = np.full(sc.NL, sc.X, np.uint8), np.full(sc.NC, sc.X, np.uint8)
    bad_l, bad_c = sc.book_stream(0, 291, "low"), sc.book_stream(1, 291, "top")
    cases += [("book failure in the luma part only", bad_l, quiet_c), ("book failure in the chroma part only", quiet_l, bad_c),
              ("book failure in both parts", bad_l, bad_c), ("book failure in the chroma part of a packet that would not fit", sc.dense_pair(77)[0], bad_c)]
    intent += [E_CODEBOOK] * 4
    cases.append(sign_case()); intent.append(0)
    res = [o.stream_stage(l, c, 80000) for _, l, c in cases]
    for (_, l, c), r in zip(cases, res):
        for a in (l, c) + tuple(r[k] for k in sc.ARRAYS):
            a.setflags(write=False)
    return cases, res, intent


def test_oracle_gives_the_intended_status_for_every_coupling_case():
    """On the CPU, the oracle alone: every case does what it is there for."""
    o = _oracle()
    assert o.stream_stage(densest_luma(), sc.zc(), 80000)["size_data1"] == 77532
    cases, res, intent = coupling_cases()
    for (name, l, c), r, st in zip(cases, res, intent):
        assert (E_SPACE if r["words"] > 80000 and r["status"] == 0 else r["status"]) == st, (name, r["status"], r["words"])
    by = {n: r for (n, _, _), r in zip(cases, res)}
    assert sorted(r["words"] for n, r in by.items() if n.startswith("capacity")) == [79999, 80000, 80000, 80001, 80001]
    assert by["book failure in the chroma part of a packet that would not fit"]["status"] == E_CODEBOOK
    assert o.stream_stage(sc.dense_pair(77)[0], sc.book_stream(1, 290, "top"), 80000)["words"] > 80000      # (it would not fit, were the book one entry shorter)
    name, l, c = cases[-1]
    r, alone = res[-1], o.stream_stage(l, sc.zc(), 80000)
    assert min(r["select1_pre"], r["select2_pre"]) > 4 and set(np.unique(c)) >= {153, 155, 157, 159}
    assert r["sel_word1"].any() and np.array_equal(r["sel_word1"], alone["sel_word1"]) and np.array_equal(r["sel_word2"], alone["sel_word2"])
    differ = sum(not np.array_equal(a["book2"], b["book2"]) for a, b in zip(res[:12], res[12:24]))
    assert differ >= 4                                           # book 2 does depend on book 1's bytes


class Stage:
    """nhw_stage_stream behind a whole batch (tests/test_stream_stage.py's hook, kept to what this file needs)"""
    def __init__(self, n, q):
        import torch
        self.n, self.e = n, encoder(n)
        self.e.encode_device(self.e.synth_device(n, seed_base=88000 + q), q)
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
        status, sizes = np.full(self.n, 99, np.int32), np.full(self.n, 99, np.uint32)
        assert self.e.lib.nhw_stage_stream(self.e.h, self.n, form, ctypes.c_void_p(status.ctypes.data), ctypes.c_void_p(sizes.ctypes.data), None) == 0
        out = []
        for i in range(self.n):
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


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_couplings_of_the_two_parts(form):
    """form 0: Y31, the chroma packetiser, k_final, from the quantisers' lists; form 1: the chroma packetiser and k_final on lists made from the
    oracle's rewritten luma stream.  Status, size, the eight scalars, the packet's words, both books and both sign words of every case."""
    cases, want, _ = coupling_cases()
    st = Stage(len(cases), 20)
    try:
        for i, ((_, l, c), w) in enumerate(zip(cases, want)):
            L = sc.lists_from_streams(l, c)
            st.write("CNZQ", i, L["cnzq"]); st.write("CVALS", i, L["cvals"])
            if form == 0:
                st.write("NZQ", i, L["nzq"]); st.write("VALS", i, L["vals"])
            else:
                R = sc.lists_from_rewritten(w["luma"])
                st.write("NZS", i, R["nzs"]); st.write("VOFF", i, R["voff"]); st.write("VALS", i, R["vals"])
        got = st.run(form)
    finally:
        st.e.close()
    for (name, _, _), g, w in zip(cases, got, want):
        if w["words"] > 80000 and w["status"] == 0:
            assert (g["status"], g["size"]) == (E_SPACE, 0), f"form {form}, '{name}' ({w['words']} words): status {g['status']} size {g['size']}"
            continue
        assert g["status"] == w["status"], f"form {form}, '{name}': status {g['status']}, the oracle's {w['status']}"
        if w["status"]:
            assert g["size"] == 0, (form, name)
            continue
        assert g["size"] > 4 * w["size_data2"], (form, name)
        bad = [k for k in SCALARS + ARRAYS if not (np.array_equal(g[k], w[k]) if isinstance(w[k], np.ndarray) else g[k] == w[k])]
        assert not bad, f"form {form}, '{name}': {bad} differ from the oracle's"
