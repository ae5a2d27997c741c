"""The chroma tail's production form (k_chroma_tail: a wavefront reads each row of the work plane once, decides the row's marks in registers and
quantises the row from those registers; B_CPROC is not written) against the staged body it replaces in a production batch, and the files
against the oracle.  The staged body is held to the oracle by the stage traces of test_gpu_parity.py.

  * crafted planes through nhw_stage_chroma_tail, form 0 (production) against form 1 (staged, every plane written, dense stream): U's parked
    bytes, the chroma part of ll_bytes, the exception list, res_u64 / res_v64, pad and the merged chroma stream in stream order, rebuilt here
    from B_CNZQ / cfbase / B_CVALS by the slice rule of pack_chroma_order -- first the situations are asserted on form 1's output;
  * whole files of the generator images against the oracle, in the forked order, in fresh child processes under NHW_CHROMA_FORK=0,
    NHW_CHROMA_TAIL_ONCE=0 and NHW_PARTS=2, and in the compatibility mode;
  * the stores are gone (B_CPROC behind form 0 is what stood there) and nobody misses them (two batches over planes filled with 0x7F and
    0x80 give the oracle's files).
Run as a script it encodes the generator images at every quality of FILE_QUALITIES in this process and compares with the oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.enc_stages import B_CL2SAVE, B_CLL1, B_CPROC, Q, Hook, chroma_images, oracle_files, ws_index
from tests.support import ROOT

N = 32
CRAFTED_QUALITIES = (11, 14, 17, 18, 20, 23)
FILE_QUALITIES = (1, 10, 14, 17, 18, 20, 22, 23)
MARK_SYMBOLS = (122, 124, 126, 130)              # what the quantiser makes of the codes 12900, 12400, 12600, 13000: no other cell gives them (every other symbol is a multiple of 8 or a big_code below 110)
META_BYTES, META_EXW_LEN, META_PAD = 128, 0, 31  # NhwMeta (nhw_ws.h) as ints
EXW_BYTES = 16384
ROWS_C = ((5, +1), (6, -1), (70, +1), (71, -1))  # class 0: (R, 0) marks its HL cell while column 127 is a pair candidate (+1) / has d == -5 (-1)
ROWS_B = (0, 1, 64, 127)                         # classes 0, 1: column 0's mark lands in LH over a cell in -7 .. -1
ROWS_E = (3, 40, 41, 90, 126)                    # classes 2, 3: rows that end in a pair mark at the last column, whatever their shift
SEAMS = (63, 127, 191)


def fork_on():
    return os.environ.get("NHW_CHROMA_FORK", "1") != "0"


def comp_buffers(comp):
    """(cproc, cll1, cl2save) of a component in the handle's order"""
    if comp and fork_on():
        return tuple(ws_index(n) for n in ("CPROC_V", "CLL1_V", "CL2SAVE_V"))
    return B_CPROC, B_CLL1, B_CL2SAVE


# ---------------------------------------------------------------------------------------------- crafted planes
def detail_values(rng, shape):
    """half the cells free for a mark (-7 .. 7, so -7 and 7 themselves get marked over), a third busy, the rest at the quantiser's thresholds
    (-8 next to -7: pair runs; 14, 15, 22, 23 in front of a 7: raises; -14, -15: the keep rules) and beyond +-127"""
    kind = rng.random(shape)
    v = rng.integers(-7, 8, shape)
    busy = rng.integers(8, 41, shape) * rng.choice((-1, 1), shape)
    v = np.where(kind > 0.45, busy, v)
    v = np.where(kind > 0.78, rng.choice((-8, -8, -7, 7, 7, 14, 15, 22, 23, -14, -15), shape), v)
    v = np.where(kind > 0.96, rng.integers(128, 420, shape) * rng.choice((-1, 1), shape), v)
    return v.astype(np.int16)


def crafted(n, seed):
    """cproc [n, 256, 256], cll1 [n, 128, 128], cl2save [n, 128, 128] of one component.  Image classes i % 4:
       0: no row ends in a pair mark, but rows ROWS_C make the last-column test fire (the evaluation pass runs and finds every shift 0);
       1: no row's last cell is a pair candidate at all (the walk starts at once);
       2, 3: ROWS_E end in a pair mark under every shift they can meet: shifts accumulate over a picture of otherwise random marks."""
    rng = np.random.default_rng(seed)
    cll1 = (128 + rng.integers(-3, 4, (n, 128, 128))).astype(np.int16)
    d = rng.integers(-9, 10, (n, 128, 128)).astype(np.int16)
    cproc = detail_values(rng, (n, 256, 256))
    l2 = detail_values(rng, (n, 128, 128))
    ll2 = rng.integers(-40, 330, (n, 64, 64))
    l2[:, :64, :64] = np.where(ll2 == 0, 1, ll2)                     # non-zero everywhere: the quantiser must read the quadrant as 0
    hl, lh, hh = cproc[:, :128, 128:], cproc[:, 128:, :128], cproc[:, 128:, 128:]
    for i in range(n):
        cls = i % 4
        if cls < 2:
            d[i, :, 127] = 0
            for R in ROWS_B:                                        # (R, 0): a single or pair mark of positive d, HL busy, LH free and negative
                d[i, R, 0] = 6; hl[i, R, 0] = 20; lh[i, R, 0] = -3
                above = -15 if R == 64 else -14                     # the cell whose look from column 255 goes to that LH cell: magnitude & 7 == 6 (the two keep rules differ) or 7 (both keep)
                if R == 0: hl[i, 127, 127] = above                  # plane row 127, across the seam into row 128
                else: hh[i, R - 1, 127] = above
            hh[i, 127, 127] = -14                                   # r = 255: the look goes behind the plane
        if cls == 0:
            for R, sign in ROWS_C:
                hl[i, R, 0] = 3; d[i, R, 0] = 6                     # (R, 0) marks its free HL cell ...
                d[i, R, 126] = 0; d[i, R, 127] = 5 * sign           # ... column 127 heads its run
                cll1[i, R + 1, 0] = -1 if sign > 0 else 10          # d1 of column 127 against the HL cell as it WAS: 3 - (-1) = 4 (pair), 3 - 10 = -7 (pair, and d == -5 with d1 < 0)
                hl[i, R, 127] = 0; lh[i, R, 127] = 20; hh[i, R, 127] = 20   # its one free detail cell
        if cls >= 2:
            for R in ROWS_E:
                cll1[i, R, 118:] = 128; cll1[i, R + 1, :12] = 128   # whatever the shift (<= 11), column 126 has d = 0 and column 127 d = 5, d1 = 4
                d[i, R, 118:] = 0; d[i, R + 1, :12] = 0
                d[i, R, 127] = 5; hl[i, R, 0] = 132; hl[i, R, 127] = 0
        for r, vals in ((80, (-7, -8, -7, -8)), (81, (0, 14, 7, 0)), (82, (-8, -7, 20, 0)), (83, (0, 23, 7, 0))):   # pair runs and raises across the lane seams, rows R and R + 128
            for s in SEAMS:
                cproc[i, r + 128, s - 1:s + 3] = vals
                if s == 63: l2[i, r, s - 1:s + 3] = vals
                elif s == 127: l2[i, r, 126:128] = vals[:2]; cproc[i, r, 128:130] = vals[2:]
                else: cproc[i, r, s - 1:s + 3] = vals
    cproc[:, :128, :128] = cll1 + d                                 # the reconstruction the marks compare with cll1
    return cproc, cll1, l2


def front_of_quantiser(cproc, l2):
    """the plane in front of the quantiser, without the marks"""
    pre = cproc.astype(np.int32).copy()
    pre[:, :128, :128] = l2
    pre[:, :64, :64] = 0
    return pre


def stream_from_list(cnzq, cfbase, cvals):
    """the merged chroma stream (2 Q symbols) from the list as the quantiser leaves it, by the slice rule of pack_chroma_order: entry e of flush
    F (lane e >> 1, half e & 1) is stream slice 64 (lane >> 1) + 4 F + 2 (lane & 1) + half, its values behind those of the entries before it
    from cfbase[F] on.  Returns the stream and the number of values of every flush."""
    out = np.full(2 * Q, 128, np.uint8)
    bits = np.unpackbits(cnzq.view(np.uint8).reshape(2048, 8), axis=1, bitorder="little")   # [entry][bit]
    counts = bits.sum(1).astype(np.int64)
    per_flush = counts.reshape(16, 128).sum(1)
    for F in range(16):
        at = int(cfbase[F])
        for e in range(128):
            k = F * 128 + e
            lane, half = e >> 1, e & 1
            S = 64 * (lane >> 1) + 4 * F + 2 * (lane & 1) + half
            c = int(counts[k])
            out[64 * S + np.flatnonzero(bits[k])] = cvals[at:at + c]
            at += c
    return out, per_flush


class Tail(Hook):
    def read8(self, buf, i, nbytes):
        return self.read(buf, i, nbytes).view(np.uint8)

    def state(self):
        """what the emission appends to: NhwMeta and the exception list of every image"""
        return [(self.read8(ws_index("META"), i, META_BYTES).copy(), self.read8(ws_index("EXW"), i, EXW_BYTES).copy()) for i in range(self.n)]

    def run_form(self, form, planes, state):
        """U then V on planes[comp] = (cproc, cll1, cl2save) from the saved state; returns per image what both forms must agree on, form 1's
        written planes / dense stream, and whether form 0 left cproc alone"""
        import torch
        for i, (meta, exw) in enumerate(state):
            self.write(ws_index("META"), i, meta); self.write(ws_index("EXW"), i, exw)
        written, untouched = {}, True
        for comp in (0, 1):
            bufs = comp_buffers(comp)
            for i in range(self.n):
                for buf, a in zip(bufs, planes[comp]):
                    self.write(buf, i, a[i])
            assert self.e.lib.nhw_stage_chroma_tail(self.e.h, self.n, comp, form, None) == 0, "nhw_stage_chroma_tail"
            torch.cuda.synchronize()
            after = np.stack([self.read(bufs[0], i, 2 * Q).reshape(256, 256) for i in range(self.n)])
            if form == 0:
                untouched &= bool((after == planes[comp][0]).all())
            written[comp] = after
        out = []
        for i in range(self.n):
            meta = self.read8(ws_index("META"), i, META_BYTES).view(np.int32)
            cn = self.read8(ws_index("CNZQ"), i, 2048 * 8 + 80)
            stream, per_flush = stream_from_list(cn[:2048 * 8].view(np.uint64), cn[2048 * 8:].view(np.uint32), self.read8(ws_index("CVALS"), i, 4 * 32768))
            cfbase = cn[2048 * 8:].view(np.uint32)
            cvals = self.read8(ws_index("CVALS"), i, 4 * 32768)
            regions = np.concatenate([cvals[32768 * w:32768 * w + int(cfbase[16 + w])] for w in range(4)])   # what the packetiser's histogram walks
            out.append({"ubytes": self.read8(ws_index("UBYTES"), i, Q), "ll_bytes": self.read8(ws_index("LLBYTES"), i, 24576)[16384:],
                        "exw_len": int(meta[META_EXW_LEN]), "exw": self.read8(ws_index("EXW"), i, EXW_BYTES)[:int(meta[META_EXW_LEN])],
                        "res_u64": self.read8(ws_index("RESU64"), i, 512), "res_v64": self.read8(ws_index("RESV64"), i, 512), "pad": int(meta[META_PAD]),
                        "stream": stream, "region_values": np.sort(regions), "fills": [int(cfbase[16 + w]) for w in range(4)], "per_flush": per_flush,
                        "dense": self.read8(ws_index("SCAN"), i, 6 * Q)[4 * Q:] if form == 1 else None})
        return out, written, untouched


def assert_situations(q, planes, written, staged, state):
    """on the staged form's output: every situation the walk has to get right occurs"""
    n = len(staged)
    for comp in (0, 1):
        cproc, cll1, l2 = planes[comp]
        S = written[comp].astype(np.int32)                          # the symbols of every cell
        pre = front_of_quantiser(cproc, l2)
        tag = f"q{q} comp {comp}:"
        mark = np.isin(S, MARK_SYMBOLS)
        assert (l2[:, :64, :64] != 0).all() and (S[:, :64, :64] == 128).all(), f"{tag} the LL2 quadrant is not read as 0"
        big = np.abs(pre) > 127
        assert (big & ~mark).sum() > 1000 and (S[big & ~mark] < 110).all(), f"{tag} values beyond +-127"
        ll2 = l2[:, :64, :64]
        assert ((ll2 > 255) | (ll2 < 0)).any() and all(s["exw_len"] > int(st[0].view(np.int32)[META_EXW_LEN]) + 4 for s, st in zip(staged, state)), f"{tag} no LL2 sample outside 0 .. 255"
        for s in SEAMS:                                             # rows 80 .. 83 of the upper and the lower half
            for half in (0, 128):
                assert (S[:, 80 + half, s - 1:s + 3] == 120).all(1).any(), f"{tag} no -7 / -8 pair run across columns {s} / {s + 1}, row {80 + half}"
                assert ((S[:, 82 + half, s - 1] == 120) & (S[:, 82 + half, s] == 120)).any(), f"{tag} no pair ending at column {s}, row {82 + half}"
                for r in (81, 83):
                    assert (S[:, r + half, s + 1] == 136).any(), f"{tag} no 7 -> 8 raise across columns {s} / {s + 1}, row {r + half}"
        if q < 18:
            assert not mark.any(), f"{tag} marks below quality 18"
            continue
        names = {"HL": mark[:, :128, 128:], "LH": mark[:, 128:, :128], "HH": mark[:, 128:, 128:]}
        for name, region in (("HL", S[:, :128, 128:]), ("LH", S[:, 128:, :128]), ("HH", S[:, 128:, 128:])):
            for code in MARK_SYMBOLS:
                assert (region == code).any(), f"{tag} no mark {code} in {name}"
        free = np.abs(cproc.astype(np.int32)) < 8
        fhl, flh = free[:, :128, 128:], free[:, 128:, :128]
        assert (names["HL"] <= fhl).all() and (names["LH"] <= (flh & ~fhl)).all() and (names["HH"] <= (free[:, 128:, 128:] & ~fhl & ~flh)).all(), f"{tag} the HL -> LH -> HH priority"
        rows_marked = names["HL"].any(2) | names["LH"].any(2) | names["HH"].any(2)          # [image][LL row]
        edge_rows = [R for R in range(128) if R % 16 in (0, 15)]    # first and last row of every 16-row flush, of every wavefront's range in either form
        assert rows_marked[:, edge_rows].any(0).all(), f"{tag} no marks in LL rows {[R for R in edge_rows if not rows_marked[:, R].any()]}"
        orig = cproc.astype(np.int32)
        pm = np.isin(orig, (-7, -8))
        nb = np.zeros_like(pm); nb[:, :, 1:] |= pm[:, :, :-1]; nb[:, :, :-1] |= pm[:, :, 1:]
        assert (mark & (orig == -7) & nb)[:, 128:].any() and (mark & (orig == -7) & nb)[:, :128, 129:].any(), f"{tag} no mark over one cell of a -7 / -8 pair"
        raiser = (orig > 6) & (orig <= 127) & ((orig & 7) >= 6)
        left = np.zeros_like(raiser); left[:, :, 1:] = raiser[:, :, :-1]
        assert (mark & (orig == 7) & left)[:, 128:].any(), f"{tag} no mark over a 7 that would have been raised"
        # column 0's mark in LH over a cell in -7 .. -1, and the look from column 255 of the row above (classes 0, 1: every shift is 0)
        for i in range(n):
            if i % 4 >= 2:
                continue
            for R in ROWS_B:
                assert cproc[i, 128 + R, 0] == -3 and S[i, 128 + R, 0] in (122, 124), f"{tag} image {i}: (R, 0) = ({R}, 0) does not mark its LH cell"
                above = int(cproc[i, 127 + R, 255])
                assert S[i, 127 + R, 255] == (120 if above == -14 else 112), f"{tag} image {i} row {127 + R}: the look from column 255 at the marked cell ({above} -> {S[i, 127 + R, 255]})"
            assert cproc[i, 255, 255] == -14
        assert {int(cproc[i, 127 + R, 255]) for i in range(0, n, 4) for R in ROWS_B} == {-14, -15}
        # (R, 0) marks its HL cell: column 127, a pair candidate / d == -5 against the cell as it was, takes no mark
        d = cproc[:, :128, :128].astype(np.int32) - cll1
        for i in range(0, n, 4):
            assert staged[i]["pad"] == 0, f"{tag} image {i}: a row ends in a pair mark"
            for R, sign in ROWS_C:
                d127, d1 = int(d[i, R, 127]), 3 - int(cll1[i, R + 1, 0])
                assert cproc[i, R, 128] == 3 and d[i, R, 126] == 0 and cproc[i, R, 255] == 0
                assert (d127 == 5 and 2 < d1 < 7) if sign > 0 else (d127 == -5 and -8 < d1 < -2), f"{tag} image {i} row {R}: column 127 is no candidate"
                # d = 5: no pair mark (124), the single mark of a positive d instead; d = -5: neither the pair mark (126) nor the single one (130), which wants d1 < 0
                assert S[i, R, 128] in MARK_SYMBOLS and S[i, R, 255] == (122 if sign > 0 else 128), f"{tag} image {i} row {R}: (R, 0) -> {S[i, R, 128]}, column 127's HL cell -> {S[i, R, 255]}"
        for i in range(n):                                          # rows that end in a pair mark: several a picture (classes 2, 3), none (0, 1)
            ev = (staged[i]["pad"] >> (8 * comp)) & 0xFF
            assert ev >= len(ROWS_E) if i % 4 >= 2 else ev == 0, f"{tag} image {i}: {ev} rows end in a pair mark"
            if i % 4 >= 2:
                assert all(S[i, R, 255] == 124 for R in ROWS_E), f"{tag} image {i}: the crafted rows do not end in a pair mark"


_crafted = {}


def crafted_planes():
    if not _crafted:
        _crafted[0] = crafted(N, 9100)
        _crafted[1] = crafted(N, 9101)
    return _crafted


@pytest.mark.gpu
@pytest.mark.parametrize("q", CRAFTED_QUALITIES)
def test_production_form_equals_the_staged_form_on_crafted_planes(q):
    planes = crafted_planes()
    h = Tail(N)
    try:
        h.e.encode(chroma_images(q, N), q)                          # the hook works at the quality of the handle's last whole batch
        state = h.state()
        staged, written, _ = h.run_form(1, planes, state)
        prod, _, untouched = h.run_form(0, planes, state)
    finally:
        h.e.close()
    for i, s in enumerate(staged):                                  # form 1's own list gives its dense stream (the slice rule, rebuilt here)
        assert (s["stream"] == s["dense"]).all(), f"q{q} image {i}: the staged form's list is not its dense stream"
    assert_situations(q, planes, written, staged, state)
    assert untouched, f"q{q}: the production form wrote B_CPROC"
    for i, (a, b) in enumerate(zip(prod, staged)):
        for key in ("ubytes", "ll_bytes", "exw", "res_u64", "res_v64", "region_values"):
            bad = np.flatnonzero(a[key] != b[key]) if a[key].shape == b[key].shape else np.array([-1])
            assert bad.size == 0, f"q{q} image {i} {key}: {bad.size} bytes differ, first {bad[:8].tolist()}"
        assert a["exw_len"] == b["exw_len"] and a["pad"] == b["pad"], f"q{q} image {i}: exw_len {a['exw_len']} / {b['exw_len']}, pad {a['pad']:#x} / {b['pad']:#x}"
        bad = np.flatnonzero(a["stream"] != b["dense"])
        assert bad.size == 0, f"q{q} image {i}: the stream differs at {bad.size} symbols, first {bad[:8].tolist()}"
        assert sum(a["fills"]) == int(a["per_flush"].sum()) == int((b["dense"] != 128).sum()), f"q{q} image {i}: cfbase[16 ..] {a['fills']}"


# ---------------------------------------------------------------------------------------------- whole files
_files = {}


def generator_case(q, n=N):
    if q not in _files:
        imgs = chroma_images(q, n)
        _files[q] = (imgs, oracle_files(imgs, q))
    return _files[q]


def encode_and_compare(q, tag):
    import nhwcodec_amd
    imgs, want = generator_case(q)
    e = nhwcodec_amd.Encoder(0, max_batch=len(imgs))
    try:
        got = e.encode(imgs, q)
    finally:
        e.close()
    bad = [i for i in range(len(imgs)) if got[i] != want[i]]
    assert not bad, f"q{q} {tag}: files {bad[:16]} differ from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("q", FILE_QUALITIES)
def test_files_equal_the_oracles(q):
    encode_and_compare(q, "forked order")


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["NHW_CHROMA_FORK=0", "NHW_CHROMA_TAIL_ONCE=0", "NHW_PARTS=2"])
def test_files_equal_the_oracles_under_a_switch(switch):
    """The switches are read when a handle is made: a fresh child process each.  NHW_PARTS=2 cuts batches of 512 images and more, so that child
    also encodes one batch of 512."""
    name, value = switch.split("=")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "chroma tail OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("q", [14, 20])
def test_files_equal_the_oracles_in_compatibility_mode(q):
    import nhwcodec_amd
    imgs = chroma_images(q, N)
    e = nhwcodec_amd.Encoder(0, max_batch=N)
    try:
        e.set_compat(True)
        got = e.encode(imgs, q)
    finally:
        e.close()
    want = oracle_files(imgs, q, True)
    bad = [i for i in range(N) if got[i] != want[i]]
    assert not bad, f"q{q} compatibility mode: files {bad[:16]} differ from the oracle"


# ---------------------------------------------------------------------------------------------- the stores are gone and nobody misses them
@pytest.mark.gpu
@pytest.mark.parametrize("q", [17, 20])
def test_production_form_leaves_the_work_plane_alone(q):
    """on the planes a batch left: B_CPROC behind form 0 is byte for byte what stood there, behind form 1 it holds the symbols"""
    import torch
    h = Tail(N)
    try:
        h.e.encode(chroma_images(q, N), q)
        before = [h.read(B_CPROC, i, 2 * Q).copy() for i in range(N)]
        for form, same in ((0, True), (1, False)):
            assert h.e.lib.nhw_stage_chroma_tail(h.e.h, N, 0, form, None) == 0
            torch.cuda.synchronize()
            for i in range(N):
                assert (h.read(B_CPROC, i, 2 * Q) == before[i]).all() == same, f"q{q} image {i} form {form}"
    finally:
        h.e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", [12, 17, 20, 23])
def test_files_over_two_fills_are_the_oracles(q):
    """a cell of a chroma work plane read without having been written in its batch differs under at least one fill"""
    imgs, want = generator_case(q) if q in FILE_QUALITIES else (chroma_images(q, N), None)
    want = want if want is not None else oracle_files(imgs, q)
    h = Tail(N)
    try:
        h.e.lib.nhw_debug_fill.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int]
        h.e.encode(imgs, q)                                         # a batch before, as in a long-running encoder
        for byte in (0x7F, 0x80):
            for name in ("CPROC", "CPROC_V"):
                assert h.e.lib.nhw_debug_fill(h.e.h, ws_index(name), byte, 2 * Q, N) == 0
            got = h.e.encode(imgs, q)
            bad = [i for i in range(N) if got[i] != want[i]]
            assert not bad, f"q{q}, the chroma work planes filled with {byte:#x}: files {bad} differ from the oracle"
    finally:
        h.e.close()


if __name__ == "__main__":
    switches = " ".join(f"{k}={v}" for k, v in os.environ.items() if k.startswith("NHW_"))
    for quality in FILE_QUALITIES:
        encode_and_compare(quality, switches)
    if os.environ.get("NHW_PARTS", "1") != "1":                     # sub-batches are cut from 512 images on: one such batch, so that the tail runs on shifted views of the workspace
        _files[20] = (chroma_images(20, 512), oracle_files(chroma_images(20, 512), 20))
        encode_and_compare(20, switches + ", 512 images")
    print("chroma tail OK")
