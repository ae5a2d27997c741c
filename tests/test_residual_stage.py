"""The luma residual passes Y19 .. Y27 on crafted planes (the kernels k_l4a / k_phase<PH_L4A>, k_phase<PH_L4B>, k_phase<PH_L4C>) behind the hook
nhw_stage_residuals (include/nhw_hip_debug.h), against the oracle's nhwo_residual_stage (oracle/nhwo.h): the very function the oracle's whole
encode runs.  Every comparison is byte equality.

Without a GPU:
  * the oracle's stage entry on the planes tapped in front of the passes of a whole encode gives the planes and lists tapped behind them;
  * over a quality's crafted set (tests/residual_cases.py) every arm counter of the passes that is live at the quality is at least 1;
  * the crafted planes stay inside the reference's own list buffers, one of them goes beyond 20 000 raw entries, and marks, codes and ripples lie in
    the edge rows and columns the builders name.
On the GPU (pytest -m gpu), one quality a test, eight planes, a handle of max_batch 8 behind a whole batch of generator pictures:
  * generator planes: the planes a debug stop behind the second level-2 synthesis leaves equal the oracle's tapped inputs, and forms 0 and 1 on
    them give its tapped outputs;
  * the crafted set at qualities 13 .. 23 through forms 0 and 1, at 7 and 12 through forms 0, 1 and 3;
  * code planes through form 2;
  * byte patterns in the outputs' and the scratch buffers and in B_META's nine list lengths in front of form 0 change nothing, and the handle
    encodes as before afterwards.

Which outputs a form defines (from the readers in nhwcodec_amd/csrc: the quantiser wave_quantise_luma and quant_load_row, Y29 luma_p4c2_par, the
container final_phase_par; nothing else reads behind Y27):
  * B_PROC's three level-1 bands, rows 256 .. 511 and columns 256 .. 511 of rows 0 .. 255, HL1's first row included: every form but 2;
  * B_PROC's level-2 block (its LL quadrant): only where Y26 copies it, above quality 21 and in form 1 -- below that the quantiser takes the block
    from B_L2SAVE, and forms 0 and 3 leave the quadrant as the reconstruction stood (form 0: with row 256 from Y22's last step);
  * B_FIRST above quality 21 (Y19's copy with Y24's feedback; Y29 reads it): forms 0, 1 and 2;
  * B_R1 / B_R3 / B_R5 LIST, BITS and WORD over the lengths in B_META, for the lists the quality makes (r1 from 13, r3 from 19, r5 from 21): forms 0, 1, 2.
    Of NhwMeta's nine lengths those of a list the quality does not make have no reader -- the container writes r3's from quality 19 and r5's from 21
    (final_phase_par) and Y25 does not set them below that -- so they are not compared; the workspace test fills all nine with a pattern first;
  * the code plane B_LL1 as Y23 leaves it, columns 0 .. 253 (Y24 and Y25 read those; Y25 does not write its follow-up codes back: nothing reads
    them): forms 0 and 1, compared with the oracle's part 0 alone.
"""
import ctypes

import numpy as np
import pytest

from tests import residual_cases as rc
from tests.enc_stages import B_JPEG, B_L2SAVE, B_LL1, B_PROC, Q, synthetic_images, ws_index

H = 256
N = rc.N_PLANES
B_FIRST, B_META, B_HS = ws_index("FIRST"), ws_index("META"), ws_index("HS")
B_LISTS = [[ws_index(f"R{k}{part}") for part in ("LIST", "BITS", "WORD")] for k in (1, 3, 5)]
LIST_BYTES = (Q + 64, 8192 + 64, 16384 + 64)                          # k_buf_bytes, nhwcodec_amd/csrc/nhw_enc.hip
SCRATCH = [(ws_index("RAW"), 2 * Q + 1024), (ws_index("PAY"), 2 * Q + 256), (ws_index("CC"), 2 * Q + 1024), (ws_index("HALF"), 2 * Q + 1024), (B_HS, 4 * Q + 256)]
CRAFTED_Q = tuple(range(13, 24))
LOW_Q = (7, 12)
CODE_Q = (13, 18, 19, 20, 21, 22, 23)
REF_LIST_BYTES = 96 * H                                               # the reference's list buffer is 96 * 256 + 1 bytes (nhw_encoder.c:1498)


def lists_made(q):
    return 0 if q <= 12 else 1 if q < 19 else 2 if q < 21 else 3


_want = {}


def want(oracle, q, kind):
    """the oracle's answers for a quality's set, computed once and shared: kind "crafted" -> per plane (whole stage, part 0 alone, part 2 alone),
    "code" -> per plane part 1 alone"""
    key = (q, kind)
    if key not in _want:
        run = lambda a, first, last: oracle.residual_stage(q, a["jpeg"], a["proc"], a["ll1"], a["l2save"], a["first_order"], first, last)
        if kind == "crafted":
            _want[key] = [(run(a, 0, 2), run(a, 0, 0), run(a, 2, 2)) for a in rc.set_for(q)]
        else:
            _want[key] = [run(a, 1, 1) for a in rc.code_set(q)]
    return _want[key]


# ---------------------------------------------------------------------------------------------- without a GPU
def texture(i):
    """a low-contrast texture of period 4 or 8 under a slow envelope: residual rules by the thousand"""
    rng = np.random.default_rng(9100 + i)
    y, x = np.mgrid[0:512, 0:512]
    w = np.sin(2 * np.pi * x / 8) * np.sin(2 * np.pi * y / 4)
    env = 0.5 + 0.5 * np.sin(2 * np.pi * (x + 2 * y) / 112)
    g = np.clip(np.rint(128 + 9 * w * env + rng.normal(0, 1.6, (512, 512))), 0, 255).astype(np.uint8)
    return np.stack([g, g, g], -1)


@pytest.mark.parametrize("q", LOW_Q + CRAFTED_Q)
def test_the_entry_is_the_whole_encodes_own_passes(oracle, q):
    """two generator pictures and a texture: the entry on the planes tapped in front of Y19 gives the planes and lists tapped behind Y27, and the
    tapped encode's file is the untapped one's (which the golden files and oracle/_ref pin)"""
    for name, img in (("seed 11", oracle.synth(11)), ("seed 12", oracle.synth(12)), ("texture", texture(5))):
        data, before, after, lists = oracle.encode_tapped(img, q)
        assert data == oracle.encode(img, q), f"q{q} {name}: the tap changes the file"
        got = oracle.residual_stage(q, before["jpeg"], before["proc"], before["ll1"], before["l2save"], before["first_order"])
        for k in after:
            bad = np.flatnonzero(got[k] != after[k])
            assert bad.size == 0, f"q{q} {name} {k}: {bad.size} cells differ, first {bad[:8].tolist()}"
        assert got["lists"] == lists, f"q{q} {name}: the position lists differ"
        # the parts compose: 0, then 1, then 2 on what the part before left
        step = dict(before)
        for part in (0, 1, 2):
            r = oracle.residual_stage(q, step["jpeg"], step["proc"], step["ll1"], step["l2save"], step["first_order"], part, part)
            step = {k: r[k] for k in after}
            if part == 1: assert r["lists"] == lists
        assert all(np.array_equal(step[k], after[k]) for k in after), f"q{q} {name}: parts 0, 1, 2 one after another differ from the whole"


@pytest.mark.parametrize("q", LOW_Q + CRAFTED_Q)
def test_the_crafted_sets_reach_every_arm(oracle, q):
    """the arm table is oracle/nhwo_internal.h's NHWO_ARMS: an arm that an earlier test of its chain shadows is not in it, and no arm is skipped here"""
    total = {}
    for whole, _, _ in want(oracle, q, "crafted"):
        for k, v in whole["arms"].items(): total[k] = total.get(k, 0) + v
    live = oracle.live_arms(q)
    assert len(live) >= 25
    assert not [k for k in live if total[k] < 1], f"q{q}: arms never taken: {[k for k in live if total[k] < 1]}"
    assert not [k for k in total if total[k] and k not in live], f"q{q}: arms taken that the table calls dead: {[k for k in total if total[k] and k not in live]}"


def y27_promises(q, planes, ws):
    """Y27 changes cells in the rows on either side of every wavefront's range, HL1's ripple reaches column 256, HL1's first row changes; and the
    ripple's look two ahead stands on both sides of its bound in every band (residual_cases.put_look_edge): at the last looking column a v1 that
    moves under a v2 <= 0 and one that stays under v2 = 1, one column further a v1 that stays under a v2 <= 0 which a look would have moved"""
    before, after = planes[5]["proc"].reshape(512, 512), ws[5][0]["proc"].reshape(512, 512)
    ch = before != after
    for r in rc.WAVE_ROWS_LH: assert ch[r, H:].any(), f"q{q}: Y27 leaves LH1 row {r} alone"
    for r in rc.WAVE_ROWS_LOW: assert ch[r, :H].any() and ch[r, H:].any(), f"q{q}: Y27 leaves row {r} alone"
    assert ch[H:, H].sum() >= 8, f"q{q}: HL1's ripple moves column 256 in {ch[H:, H].sum()} rows"
    assert ch[H, 1:H].any(), f"q{q}: Y27 leaves HL1's first row alone"
    origin = dict(lh=(0, H), hl=(H, 0), hh=(H, H))
    seen = {(b, k): set() for b in origin for k in ("moved", "stayed", "forbidden")}
    for i in (5, 6):
        into, out = planes[i]["proc"].reshape(512, 512), ws[i][0]["proc"].reshape(512, 512)
        for band, r, c1, looks, v2 in rc.look_edge_notes(q)[i]:
            r0, c0 = origin[band]
            v0, v1_in, v1 = int(out[r0 + r, c0 + c1 - 1]), int(into[r0 + r, c0 + c1]), int(out[r0 + r, c0 + c1])
            asks = v0 < -7 and (-v0 & 7) < 2                          # the cell's ripple reaches its fourth arm (Y20 and Y21 may have taken the chain apart)
            if asks and looks and v2 <= 0 and v1 == v1_in + 1: seen[band, "moved"].add(r)
            elif asks and v1 == v1_in and v1 < -14 and (-v1 & 7) < 2 and (v2 > 0 or not looks): seen[band, "stayed" if looks else "forbidden"].add(r)
    for (band, kind), rows in seen.items():
        assert rows, f"q{q}: the look two ahead of {band}: no chain that {kind}"
    edge = lambda band: set(rc.EDGE_ROWS_LH if band == "lh" else rc.EDGE_ROWS_LOW)
    if q >= 20:                                                       # no Y20: every chain stands, so both sides lie in first and last rows of the wavefronts' ranges
        for band in origin:
            assert len(seen[band, "moved"] & edge(band)) >= 3 and len(seen[band, "forbidden"] & edge(band)) >= 6, f"q{q} {band}: {seen[band, 'moved']}, {seen[band, 'forbidden']}"


@pytest.mark.parametrize("q", LOW_Q)
def test_low_sets_hold_what_they_promise(oracle, q):
    """qualities 7 and 12 run Y20, Y26 and Y27 only: Y27's part of the promises on the low set"""
    planes = rc.set_for(q)
    for a in planes: rc.check_domain(a)
    y27_promises(q, planes, want(oracle, q, "crafted"))


@pytest.mark.parametrize("q", CRAFTED_Q)
def test_crafted_planes_hold_what_they_promise(oracle, q):
    """the reference's own buffers hold every list; one plane goes beyond 20 000 raw entries; marks, codes and ripples in the named rows and columns"""
    ws = want(oracle, q, "crafted")
    planes = rc.set_for(q)
    for a in planes: rc.check_domain(a)
    raw = np.array([[l["raw_count"] for l in whole["lists"]] for whole, _, _ in ws])
    assert raw.max() <= REF_LIST_BYTES, f"q{q}: a list of {raw.max()} raw entries does not fit the reference's {REF_LIST_BYTES + 1} bytes"
    assert raw[:, 0].max() > 20000, f"q{q}: the first list's raw entries stay at {raw[:, 0].max()}"
    for w in want(oracle, q, "code"):
        assert max(l["raw_count"] for l in w["lists"]) <= REF_LIST_BYTES
    code = lambda i: ws[i][1]["ll1"].reshape(H, H)                     # the code plane as Y23 leaves it
    marks = (123, 124)
    # Y22's marks at the plane's edges: rows 0, 1, 253, 254 (a mark in row 254 writes HL1's first row) and columns 0, 1, 254, 255
    rows = set(); cols = set()
    for i in (0, 1, 2, 3, 6):
        m = np.isin(code(i), marks)
        rows |= set(np.flatnonzero(m.any(1)).tolist()); cols |= set(np.flatnonzero(m.any(0)).tolist())
    assert {0, 1, 253, 254} <= rows, f"q{q}: no mark in rows {sorted({0, 1, 253, 254} - rows)}"
    assert {0, 1, 254, 255} <= cols, f"q{q}: no mark in columns {sorted({0, 1, 254, 255} - cols)}"
    a2, after2 = planes[2], ws[2][1]
    hl0_before, hl0_after = a2["proc"].reshape(512, 512)[256, :H], after2["proc"].reshape(512, 512)[256, :H]
    assert (hl0_before != hl0_after).any(), f"q{q}: no mark of row 254 reaches HL1's first row"
    if q >= 20:                                                       # (no Y20 from quality 20 on: what differs from Y27 alone in row 256 is the marks' doing)
        marked, y27_alone = ws[3][0]["proc"].reshape(512, 512)[256, :H], ws[3][2]["proc"].reshape(512, 512)[256, :H]
        assert (marked != y27_alone).sum() >= 100 and marked[255] != y27_alone[255], f"q{q}: row 254's marks do not show in HL1's first row behind Y27"
    # the look-further arms in column 255 (its neighbour is LH1's first column minus column 0's cells) and in column 254
    assert np.isin(code(2)[:, 255], marks).sum() >= 4 and np.isin(code(2)[:, 254], marks).sum() >= 4
    if q >= 17:                                                       # Y21's marks in rows 1 and 254 and columns 1 and 254 of both bands
        p = ws[4][1]["proc"].reshape(512, 512)
        for name, band in (("LH1", p[:H, H:]), ("HL1", p[H:, :H])):
            t, centre = np.isin(band, (12700, 12900, 10100)), np.isin(band, (12700, 12900))
            assert t[1].any() and t[254].any() and t[:, :2].any() and t[:, 254:].any(), f"q{q}: no run mark at an edge of {name}"
            assert centre[:, 1].any() and centre[:, 254].any(), f"q{q}: no run centred on column 1 or 254 of {name}"
            assert not t[0].any() and not t[255].any() and not centre[:, 0].any() and not centre[:, 255].any()
    y27_promises(q, planes, ws)
    if q >= 22:                                                       # Y24: first-order cells that take two and three contributions, the last rows' spill
        cp = rc.code_set(q)[6]["ll1"].astype(np.int32)
        n = np.zeros((H, H + 2), np.int32)                            # contributions to the first-order cell (j, r), by code column j and row r
        for k, codes in enumerate(((121, 122, 123, 124, 125, 126, 140, 141, 144, 145, 148, 149), (121, 122, 123, 124, 125, 126), (123, 124))):
            n[:254, k:k + H] += np.isin(cp[:, :254], codes).T
        assert (n == 2).any() and (n == 3).any() and n[:, H:].any(), f"q{q}: no stacked contributions"


# ---------------------------------------------------------------------------------------------- on the GPU
class Stage:
    """a handle behind a whole batch of generator pictures at quality q, with the hook's planes written, run and read"""

    def __init__(self, q):
        import nhwcodec_amd
        self.q = q
        self.e = nhwcodec_amd.Encoder(0, max_batch=N)
        self.images = synthetic_images(q, N)
        self.files = self.e.encode(self.images, q)

    def close(self):
        self.e.close()

    def read(self, buf, i, nbytes, dtype=np.uint8):
        out = np.empty(nbytes, np.uint8)
        assert self.e.lib.nhw_debug_read(self.e.h, buf, i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(nbytes)) == 0
        return out.view(dtype)

    def write(self, buf, i, a):
        a = np.ascontiguousarray(a)
        assert self.e.lib.nhw_debug_write(self.e.h, buf, i, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0

    def fill(self, buf, byte, nbytes):
        assert self.e.lib.nhw_debug_fill(self.e.h, buf, byte, ctypes.c_size_t(nbytes), N) == 0

    def run(self, form, planes):
        """planes: per image the dict of residual_cases -> per image what the form leaves"""
        for i, a in enumerate(planes):
            for buf, k in ((B_JPEG, "jpeg"), (B_PROC, "proc"), (B_LL1, "ll1"), (B_L2SAVE, "l2save"), (B_FIRST, "first_order")):
                self.write(buf, i, a[k])
        return self.launch(form, len(planes))

    def launch(self, form, n):
        import torch
        assert self.e.lib.nhw_stage_residuals(self.e.h, n, form, None) == 0, "nhw_stage_residuals"
        torch.cuda.synchronize()
        out = []
        for i in range(n):
            meta = self.read(B_META, i, 64, np.int32)
            lens = meta[2:11].reshape(3, 3)
            lists = [[self.read(B_LISTS[k][part], i, LIST_BYTES[part]) for part in range(3)] for k in range(3)]
            out.append(dict(proc=self.read(B_PROC, i, 8 * Q, np.int16).reshape(512, 512), ll1=self.read(B_LL1, i, 2 * Q, np.int16).reshape(H, H),
                            first_order=self.read(B_FIRST, i, 2 * Q, np.int16).reshape(H, H), lens=lens.copy(), lists=lists))
        return out


def first_cells(a, b):
    bad = np.argwhere(a != b)
    return f"{len(bad)} cells differ, first {bad[:6].tolist()}"


def compare(q, form, got, whole, part0=None, bands=True, block=False, first=False, lists=True):
    """one plane's outputs of a form against the oracle's, by the module docstring's list; the message names quality, form, plane, buffer and cells"""
    for i, (g, w) in enumerate(zip(got, whole)):
        tag = f"q{q} form {form} plane {i}"
        wp = w["proc"].reshape(512, 512)
        if bands:
            for name, sl in (("LH1", (slice(0, H), slice(H, 512))), ("HL1", (slice(H, 512), slice(0, H))), ("HH1", (slice(H, 512), slice(H, 512)))):
                assert np.array_equal(g["proc"][sl], wp[sl]), f"{tag} B_PROC {name}: {first_cells(g['proc'][sl], wp[sl])} (band-local row, column)"
        if block:
            assert np.array_equal(g["proc"][:H, :H], wp[:H, :H]), f"{tag} B_PROC level-2 block: {first_cells(g['proc'][:H, :H], wp[:H, :H])}"
        if first:
            wf = w["first_order"].reshape(H, H)
            assert np.array_equal(g["first_order"], wf), f"{tag} B_FIRST: {first_cells(g['first_order'], wf)}"
        if part0 is not None:
            wc = part0[i]["ll1"].reshape(H, H)[:, :254]
            assert np.array_equal(g["ll1"][:, :254], wc), f"{tag} B_LL1 (the code plane behind Y23): {first_cells(g['ll1'][:, :254], wc)}"
        if lists:
            for k in range(lists_made(q)):
                wl = w["lists"][k]
                name = f"B_R{(1, 3, 5)[k]}"
                want_lens = [len(wl["list"]), len(wl["bits"]), len(wl["word"])]
                assert g["lens"][k].tolist() == want_lens, f"{tag} {name} lengths (list, bits, word): {g['lens'][k].tolist()}, oracle {want_lens}"
                for part, key in enumerate(("list", "bits", "word")):
                    a, b = g["lists"][k][part][:want_lens[part]], np.frombuffer(wl[key], np.uint8)
                    assert np.array_equal(a, b), f"{tag} {name}{key.upper()}: {first_cells(a, b)} of {len(b)} bytes"


def compare_form(q, form, got, ws):
    whole, part0, part2 = [w[0] for w in ws], [w[1] for w in ws], [w[2] for w in ws]
    if form == 3: compare(q, form, got, part2, block=q > 21, lists=False)
    else: compare(q, form, got, whole, part0 if q > 12 else None, block=q > 21 or form == 1, first=q > 21)


@pytest.mark.gpu
@pytest.mark.parametrize("q", CRAFTED_Q)
def test_crafted_planes(oracle, q):
    ws = want(oracle, q, "crafted")
    s = Stage(q)
    try:
        for form in (0, 1):
            compare_form(q, form, s.run(form, rc.set_for(q)), ws)
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", LOW_Q)
def test_crafted_planes_low_qualities(oracle, q):
    """no second closed loop below quality 13: Y20, Y26 and Y27 only"""
    ws = want(oracle, q, "crafted")
    s = Stage(q)
    try:
        for form in (0, 1, 3):
            compare_form(q, form, s.run(form, rc.set_for(q)), ws)
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", CODE_Q)
def test_code_planes(oracle, q):
    """Y24 and Y25 alone: the lists, and the first-order plane above quality 21"""
    w = want(oracle, q, "code")
    s = Stage(q)
    try:
        compare(q, 2, s.run(2, rc.code_set(q)), w, bands=False, first=q > 21)
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", (17, 20, 23))
def test_generator_planes(oracle, q):
    """the planes behind the second level-2 synthesis (a debug stop; the stage numbers are test_tail_stages_match_the_oracle_trace's) are the
    oracle's tapped inputs -- LL1 is compared at this point nowhere else --, and forms 0 and 1 on them give its tapped outputs"""
    import torch
    s = Stage(q)
    try:
        imgs = s.images[:2]
        taps = [oracle.encode_tapped(im, q) for im in imgs]
        s.e.lib.nhw_debug_stop_after(s.e.h, 12 if q < 22 else 11)
        s.e.encode_device(torch.from_numpy(imgs).cuda(), q)
        torch.cuda.synchronize()
        s.e.lib.nhw_debug_stop_after(s.e.h, 0)
        stood = []
        for i, (_, before, _, _) in enumerate(taps):
            g = dict(jpeg=s.read(B_JPEG, i, 8 * Q, np.int16).reshape(512, 512), proc=s.read(B_PROC, i, 8 * Q, np.int16).reshape(512, 512),
                     ll1=s.read(B_LL1, i, 2 * Q, np.int16).reshape(H, H), l2save=s.read(B_L2SAVE, i, 2 * Q, np.int16).reshape(H, H),
                     first_order=s.read(B_FIRST, i, 2 * Q, np.int16).reshape(H, H))
            for name, a, b in (("B_JPEG's LL quadrant", g["jpeg"][:H, :H], before["jpeg"].reshape(512, 512)[:H, :H]), ("B_PROC", g["proc"], before["proc"].reshape(512, 512)),
                               ("B_LL1", g["ll1"], before["ll1"].reshape(H, H)), ("B_L2SAVE", g["l2save"], before["l2save"].reshape(H, H))):
                assert np.array_equal(a, b), f"q{q} image {i} {name} behind the second synthesis: {first_cells(a, b)}"
            stood.append(g)
        assert s.e.encode(s.images, q) == s.files                    # the hook wants a whole batch behind it
        whole = [dict(after, lists=lists) for _, _, after, lists in taps]
        for form in (0, 1):
            compare(q, form, s.run(form, stood), whole, block=q > 21 or form == 1, first=q > 21)
    finally:
        s.e.lib.nhw_debug_stop_after(s.e.h, 0)
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", (18, 20, 23))
def test_workspace_independence(oracle, q):
    """the outputs' buffers, the nine list lengths in B_META and the scratch of Y25 (B_RAW, B_PAY, B_CC, B_HALF, B_HS) hold a byte pattern in front of
    form 0, another one the second time: the outputs are the oracle's both times, and the handle encodes a whole batch as before afterwards"""
    ws = want(oracle, q, "crafted")
    s = Stage(q)
    try:
        for byte in (0xA5, 0x3C):
            for buf, nbytes in SCRATCH: s.fill(buf, byte, nbytes)
            for k in range(3):
                for part in range(3): s.fill(B_LISTS[k][part], byte, LIST_BYTES[part])
            for i in range(N):                                        # the nine list lengths of NhwMeta, nothing else of it
                meta = s.read(B_META, i, 256).copy()
                meta[8:44] = byte
                s.write(B_META, i, meta)
            planes = [dict(a, first_order=np.full((H, H), np.int16(byte * 257 - 65536 if byte & 0x80 else byte * 257), np.int16)) if q > 21 else a for a in rc.set_for(q)]
            compare_form(q, 0, s.run(0, planes), ws)
        assert s.e.encode(s.images, q) == s.files, f"q{q}: the files of a whole batch behind the hook differ from the ones before it"
    finally:
        s.close()
