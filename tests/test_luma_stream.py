"""The luma tail's forked order: Y5 beside the first dequantiser simulation, and the LL2 bump walk made once (by the emission, for the second
simulation as well) (pytest -m gpu; the walk's port against the oracle runs on the CPU).

  * files of whole production batches (1, 5 and 64 images; the qualities at which the three parts branch) against the oracle, byte for byte;
  * the same batches from a fresh process with NHW_CHROMA_FORK=0 (the in-line order: the kernels as they were, one stream), with NHW_Y5_FORK=0
    and with NHW_LL2_ONCE=0 (the forked order with one of its two parts switched off) against the forked run's;
  * the LL2 walk behind nhw_stage_ll2_walk (include/nhw_hip_debug.h): the forked order's two kernels against the in-line order's on the same
    written planes, every cell of B_JPEG and B_PROC, the cells outside the level-2 block against what was written, the LL2 quadrants against the
    oracle's planes behind its second simulation (generator images) and against ll2_walk below with the coder's own verbatim list (planes with
    samples pushed outside 0 .. 255).  The hook launches the kernels on one stream: the production launch ORDER -- the events and the two
    streams -- is covered by the files alone (the first two items and the last);
  * one handle: q20, q10, q20 -- the third batch's files are the first's.
The forced slice orders of tests/test_gpu_schedule.py split kernels, not streams: they do not reach the new joins, and no case for them is here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.enc_stages import B_JPEG, B_L2SAVE, B_PROC, Q, Hook, oracle_files, ws_index
from tests.support import ROOT

B_LLMEM, B_META = ws_index("LLMEM"), ws_index("META")
META_LL_MEM_LEN = 18                               # NhwMeta::ll_mem_len as an int index (nhw_ws.h: two lengths, four NhwPosLens, four more lengths in front of it)

QUALITIES = (7, 12, 13, 14, 17, 18, 20, 21, 23)    # Y5 from 7, k_l2_recon<true> from 13, Y16's fork from 14, the bump walk from 18, the lists fork up to 20, Y29 from 22
BATCHES = (1, 5, 64)                               # 5: a partly filled four-image workgroup of the wavefront-per-image kernels
WALK_QUALITIES = (13, 18, 20, 23)
WALK_IMAGES = 6                                    # 4 generator images + 2 of them with samples pushed out of range


def seeds(q, n=64):
    return [74000 + 131 * q + i for i in range(n)]


# ---------------------------------------------------------------------------------------------- the walk, as the reference states it
def ll2_tags(row, q):
    """ll2 tags of one row of 128 samples as loaded (image_processing.c:2609-2640): runs of four odd samples whose ends differ by more than 1"""
    t = np.zeros(128, bool)
    starts = 0
    if q > 17:
        o = row & 1
        j = 0
        while j <= 124:
            if o[j] and o[j + 1] and o[j + 2] and o[j + 3] and abs(int(row[j]) - int(row[j + 3])) > 1:
                t[j:j + 4] = True
                starts += 1
                j += 4
            else:
                j += 1
    return t, starts

def alt_runs(c):
    out = np.zeros_like(c)
    j = 0
    while j < c.size:
        if c[j]:
            out[j] = True
            j += 2
        else:
            j += 1
    return out

def ll2_walk(plane, q):
    """plane: int [>=128, >=130] rows of the work plane before the emission.  -> final values [128,128], tags, counts"""
    v = plane[:128, :130].astype(np.int64).copy()
    v = np.concatenate([v, np.zeros((4, 130), np.int64)])
    tg = np.zeros((132, 128), bool)
    n_tag = 0
    for r in range(128):
        tg[r], s = ll2_tags(v[r, :128], q)
        n_tag += s
    n_fired = n_vf = 0
    col = np.arange(128)
    if q > 17:
        for r in range(128):
            o, o1, o2, o3 = ((v[r + k] & 1).astype(bool) for k in range(4))
            v0 = v[r]
            d2 = (np.abs(v0[:128] - v0[2:130]) > 1) | np.concatenate([tg[r, 2:], [False, False]])
            cond1 = o[:128] & o[1:129] & (col >= 1)
            hbr = cond1 & o[2:130] & (col <= 125)
            act = ~tg[r]
            fired = alt_runs(hbr & d2 & act)
            bumped = np.concatenate([[False], fired[:-1]])
            vf = np.zeros(128, bool)
            if r <= 126:
                vf = cond1 & ~hbr & o1[:128] & o1[1:129] & ~o1[2:130]
            if 1 <= r <= 124:
                vf = vf | (~cond1 & o[:128] & o1[:128] & o1[1:129] & o2[:128] & ~o3[:128])
            vf = vf & act & ~bumped & ~tg[r + 1]
            v[r, :128] += bumped
            v[r + 1, :128] += vf
            n_fired += int(fired.sum()); n_vf += int(vf.sum())
    out = v[:128, :128]
    exc = (out > 255) | (out < 0)
    exc[0, 0] = False
    return out, tg[:128], dict(fired=n_fired, vf=n_vf, res4=n_tag, exceptions=int(exc.sum()))


def oracle_walk_planes(seed, q):
    """the oracle's planes round its LL2 emission and second simulation: (jpeg, proc) in front of the emission, (jpeg, proc) behind the
    simulation, the verbatim list's length, the exception list's length in bytes"""
    from oracle.oraclepy import Oracle
    o = Oracle()
    _, tr = o.encode(o.synth(seed), q, trace=True)
    names = [n for n, _ in tr]
    k = names.index("LL2_emit_Y")
    pre = [j for j in range(k) if names[j] == "wavelet_analysis_256"][-1]
    p0 = names.index("offsetY_recons256_p0")
    plane = lambda b: np.frombuffer(b, np.int16).reshape(512, 512).copy()
    return (plane(tr[pre][1][0]), plane(tr[pre][1][1]), plane(tr[p0][1][0]), plane(tr[p0][1][1]),
            len(tr[names.index("Y_highres_compression")][1][2]) // 2, len(tr[k][1][2]))


def pushed_out(proc, rng):
    """a copy of the work plane with patches of the LL2 quadrant pushed above 255 and below 0 (odd and even steps: the parities change with them)"""
    p = proc.copy()
    for _ in range(6):
        r, c = rng.integers(0, 112, 2)
        p[r:r + 16, c:c + 16] += np.int16(rng.integers(60, 260))
        r, c = rng.integers(0, 112, 2)
        p[r:r + 16, c:c + 16] -= np.int16(rng.integers(60, 260))
    p[0, 0] = 300                                                # the first sample is never an exception (nhw_encoder.c:700)
    p[127, 120:128] = -5
    return p


def walk_inputs(q):
    """per image (jpeg, proc, oracle's jpeg | None, oracle's proc | None, walk's values, walk's tags), and the counts of what the inputs take"""
    rng = np.random.default_rng(8800 + q)
    out = []
    total = dict(fired=0, vf=0, res4=0, exceptions=0, verbatim=0)
    real = [oracle_walk_planes(s, q) for s in seeds(q, WALK_IMAGES - 2)]
    for jpeg, proc, oj, op, mem, exw in real:
        v, tg, cnt = ll2_walk(proc, q)
        assert exw == 3 * cnt["exceptions"]
        assert np.array_equal(v, op[:128, :128]), "the walk's port against the oracle's work plane"
        for k in cnt: total[k] += cnt[k]
        total["verbatim"] += mem
        out.append((jpeg, proc, oj, op, v, tg))
    for jpeg, proc, *_ in real[:2]:
        p = pushed_out(proc, rng)
        v, tg, cnt = ll2_walk(p, q)
        for k in cnt: total[k] += cnt[k]
        out.append((jpeg, p, None, None, v, tg))
    return out, total


def needed(q):
    """what a quality's inputs must take: exceptions always; verbatim samples where the coder sends any (q > 15); the bump walk from q18"""
    return ("exceptions",) + (("verbatim",) if q > 15 else ()) + (("fired", "vf", "res4") if q > 17 else ())


@pytest.mark.parametrize("q", WALK_QUALITIES)
def test_walk_inputs_take_every_branch_and_the_port_is_the_oracle(q):
    _, total = walk_inputs(q)
    for k in needed(q):
        assert total[k] > 0, f"q{q}: the inputs take no {k}"


# ---------------------------------------------------------------------------------------------- GPU part
_forked = {}


def images(q):
    from oracle.oraclepy import Oracle
    o = Oracle()
    return np.stack([o.synth(s) for s in seeds(q)])


def forked_files(q):
    """the production (forked) files of quality q, per batch size, one handle for the three: made once, shared by the tests"""
    if q not in _forked:
        import nhwcodec_amd
        imgs = images(q)
        e = nhwcodec_amd.Encoder(0, max_batch=max(BATCHES))
        try:
            _forked[q] = {n: e.encode(imgs[:n], q) for n in BATCHES}
        finally:
            e.close()
    return _forked[q]


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_forked_batches_equal_the_oracle(q):
    want = oracle_files(images(q), q)
    for n, files in forked_files(q).items():
        bad = [i for i in range(n) if files[i] != want[i]]
        assert not bad, f"q{q} batch {n}: files {bad[:16]} differ from the oracle"


CHILD = """
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %r)
import nhwcodec_amd
from tests.test_luma_stream import BATCHES, QUALITIES, images
e = nhwcodec_amd.Encoder(0, max_batch=max(BATCHES))
out = {}
for q in QUALITIES:
    imgs = images(q)
    for n in BATCHES:
        out["%%d %%d" %% (q, n)] = [hashlib.sha256(f).hexdigest() for f in e.encode(imgs[:n], q)]
e.close()
print("FILES " + json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["NHW_CHROMA_FORK", "NHW_Y5_FORK", "NHW_LL2_ONCE"])
def test_switched_off_gives_the_same_files(switch):
    """the schedule switches are read when a handle is made: a fresh process, every quality and batch size in one"""
    import hashlib
    import json
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("FILES "))[6:])
    for q in QUALITIES:
        for n, files in forked_files(q).items():
            assert got[f"{q} {n}"] == [hashlib.sha256(f).hexdigest() for f in files], f"q{q} batch {n}: the files with {switch}=0 differ from the forked order's"


class WalkHook(Hook):
    def run_walk(self, form, inputs):
        import torch
        for i, (jpeg, proc, *_) in enumerate(inputs):
            self.write(B_JPEG, i, jpeg)
            self.write(B_PROC, i, proc)
            self.write(B_L2SAVE, i, proc[:256, :256])
        assert self.e.lib.nhw_stage_ll2_walk(self.e.h, self.n, form, None) == 0, "nhw_stage_ll2_walk"
        torch.cuda.synchronize()
        return [(self.read(B_JPEG, i, 8 * Q).reshape(512, 512), self.read(B_PROC, i, 8 * Q).reshape(512, 512)) for i in range(self.n)]

    def verbatim(self, i):
        """the LL coder's list of verbatim samples of image i (indices into the 128 x 128 quadrant), as the last hook call left it"""
        n = int(self.read(B_META, i, 4 * (META_LL_MEM_LEN + 1)).view(np.int32)[META_LL_MEM_LEN])
        return self.read(B_LLMEM, i, 2 * n + 2).view(np.uint16)[:n].astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("q", WALK_QUALITIES)
def test_one_walk_leaves_what_two_left(q):
    inputs, total = walk_inputs(q)
    for k in needed(q):
        assert total[k] > 0, f"q{q}: the inputs take no {k}"
    n = len(inputs)
    h = WalkHook(n)
    try:
        h.e.encode(images(q)[:n], q)                                # the hook works at the quality of the handle's last whole batch
        two = h.run_walk(1, inputs)
        one = h.run_walk(0, inputs)
        sent = [h.verbatim(i) for i in range(n)]
        two_deferred = h.run_walk(3, inputs)
        one_deferred = h.run_walk(2, inputs)
    finally:
        h.e.close()
    ll = (slice(0, 128), slice(0, 128))
    for i, (jpeg, proc, oj, op, v, tg) in enumerate(inputs):
        for name, a, b, src in (("jpeg", one[i][0], two[i][0], jpeg), ("proc", one[i][1], two[i][1], proc)):
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"q{q} image {i} {name}: {len(bad)} cells differ between one walk and two, first {bad[:6].tolist()}"
            outside = a.copy(); outside[:256, :256] = src[:256, :256]
            assert np.array_equal(outside, src), f"q{q} image {i} {name}: cells outside the level-2 block are touched"
        for name, a, b in (("jpeg", one_deferred[i][0], two_deferred[i][0]), ("proc", one_deferred[i][1], two_deferred[i][1])):
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"q{q} image {i} {name} behind the synthesis: {len(bad)} cells differ between one walk and two, first {bad[:6].tolist()}"
        assert np.array_equal(one[i][1][ll], v), f"q{q} image {i}: the work plane's LL2 quadrant is not the walk's"
        rounded = np.where(tg, v, np.where((v > 0) & (v < 256), v & 0xFFFE, v))
        got = one[i][0][ll]
        want = rounded.copy().reshape(-1)
        want[sent[i]] = v.reshape(-1)[sent[i]]                     # (the coder's list: its port is the oracle's, checked by the files)
        assert np.array_equal(got.reshape(-1), want), f"q{q} image {i}: the reconstruction plane's LL2 quadrant is not the rounded walk with the verbatim samples put back"
        assert q <= 15 or sent[i].size, f"q{q} image {i}: no verbatim sample"
        if oj is not None:
            assert np.array_equal(got, oj[ll]) and np.array_equal(one[i][1][ll], op[ll]), f"q{q} image {i}: the LL2 quadrants differ from the oracle's"


@pytest.mark.gpu
def test_a_handle_reused_across_qualities():
    """q20, q10 (no second loop, the emission's own zeros), q20 again: the events Y5's fork and join wait on are this batch's"""
    import nhwcodec_amd
    a, b = images(20)[:21], images(10)[:21]
    e = nhwcodec_amd.Encoder(0, max_batch=21)
    try:
        first, low, third = e.encode(a, 20), e.encode(b, 10), e.encode(a, 20)
    finally:
        e.close()
    assert third == first
    assert first == forked_files(20)[64][:21]
    assert low == oracle_files(b, 10)
