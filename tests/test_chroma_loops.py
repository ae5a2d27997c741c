"""k_chroma_loops (both closed loops of a chroma component on one LDS residency of the level-2 block) against the seven staged kernels it
replaces in production, plane by plane and cell by cell, and the files against the oracle.

What is compared, for every image of every case:
  * B_CL2SAVE (U, with the chroma fork) and B_CL2SAVE_V / B_CL2SAVE (V, with / without the fork) as a whole production batch leaves them;
  * behind nhw_stage_chroma_loops (the production launches of one component's head, on the handle's first plane set): the whole of B_CPROC
    (the reconstructed LL1 block AND every cell outside it), B_CL2SAVE and B_CLL1 with the neighbour cell behind it;
  * ... with what the staged path leaves in the same planes at the stop behind the component's second level-2 synthesis;
  * the files with the oracle's.
Run as a script it makes the same checks in this process (the NHW_CHROMA_FORK=0 case starts it as a fresh child)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.enc_stages import B_CL2SAVE, B_CLL1, B_CPROC, N_IMAGES, Q, chroma_images, oracle_files, ws_index
from tests.support import ROOT

QUALITIES = (1, 10, 14, 15, 16, 17, 18, 20, 22, 23)   # the q <= 15 branch of the first simulation, both res_uv settings, the q >= 22 path


def _luma_stages(q):
    """the stage count behind Y31 (fewer stages where a closed loop is missing); a chroma sequence has 12, the second synthesis is its 11th"""
    return 12 if q >= 22 else 13 if q > 12 else 11 if q > 6 else 7


def threshold_planes(n, seed):
    """LL1 blocks [n, 128, 128] and cproc planes [n, 256, 256] written straight into the workspace, aimed at the constants of
    dequant_sim_chroma_par and chroma_p3_par: noise of eight amplitudes round 128 and round 255 / 256 (LL2 cells on both sides of the
    0 < v < 256 test; reconstruction errors of every size up to +-12), the last four rows stepping down by 7 .. 9 on every odd row (the
    level-2 details of columns 126 and 127 sit at -7 / -8: pairs that end at the last column), and small values of both signs in cproc
    outside the block (column 128 is the right neighbour of column 127 in all three pointwise passes)."""
    rng = np.random.default_rng(seed)
    ll1 = np.empty((n, 128, 128), np.int16)
    for i in range(n):
        amp = (1, 2, 3, 4, 6, 8, 12, 16)[(i // 2) % 8]
        ll1[i] = (256 if i % 2 else 128) + rng.integers(-amp, amp + 1, (128, 128))
        edge = ll1[i, 124].astype(np.int32) // 2 + ll1[i, 123].astype(np.int32) // 2
        ll1[i, 124] = edge; ll1[i, 126] = edge
        ll1[i, 125] = edge - rng.integers(7, 10, 128); ll1[i, 127] = edge - rng.integers(7, 10, 128)
    cproc = rng.integers(-12, 13, (n, 256, 256)).astype(np.int16)
    return ll1, cproc


def check_threshold_planes(q, n=32):
    """The fused kernel alone against the seven staged kernels alone on written planes; first the staged planes must show every situation."""
    import torch
    import nhwcodec_amd
    ll1, cproc = threshold_planes(n, 4100 + q)
    e = nhwcodec_amd.Encoder(0, max_batch=n)

    def rd(buf, i, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert e.lib.nhw_debug_read(e.h, buf, i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(nbytes)) == 0
        return out.view(np.int16)

    def run(comp, form):
        for i in range(n):
            for buf, a in ((B_CLL1, ll1[i]), (B_CPROC, cproc[i])):
                a = np.ascontiguousarray(a)
                assert e.lib.nhw_debug_write(e.h, buf, i, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0
        assert e.lib.nhw_stage_chroma_loops(e.h, n, comp, form, None) == 0
        torch.cuda.synchronize()
        return [(rd(B_CPROC, i, 2 * Q).reshape(256, 256), rd(B_CL2SAVE, i, Q // 2).reshape(128, 128), rd(B_CLL1, i, Q // 2 + 2)) for i in range(n)]

    try:
        e.encode(chroma_images(q, n), q)                         # the hook works at the quality of the handle's last whole batch
        for comp in (0, 1):
            recon1 = np.stack([p[0][:128, :128] for p in run(comp, 4)]).astype(np.int32)   # behind the first synthesis
            staged = run(comp, 8)
            fused = run(comp, 1)
            # ---- the situations, read off the staged planes
            o = ll1.astype(np.int32)
            d = recon1 - o                                          # chroma_p3_par's difference ...
            o_next = np.concatenate([o.reshape(n, -1)[:, 128::128], np.zeros((n, 1), np.int32)], 1)        # the LL1 cell behind a row's last; behind the block: the neighbour cell (0)
            nx = np.concatenate([d[:, :, 1:], (cproc[:, :128, 128].astype(np.int32) - o_next)[:, :, None]], 2)   # ... and the right neighbour's, column 128 behind column 127
            for v in (3, 4, 7, 10, -3, -4, -7, -10):
                assert (d == v).any(), f"q{q} comp {comp}: no pre-compensation difference of exactly {v}"
            for v in (3, -3):                                       # where the step depends on the neighbour, and on the component at nx == 0
                assert ((d == v) & (nx == 0)).any() and ((d == v) & (nx > 0)).any() and ((d == v) & (nx < 0)).any(), f"q{q} comp {comp}: d == {v} not met with every sign of nx"
            assert (np.abs(d[:, :, 127]) == 3).any(), f"q{q} comp {comp}: no |d| == 3 in column 127 (the neighbour outside the block decides)"
            save = np.stack([p[1] for p in staged]).astype(np.int32)          # the coefficient block the second simulation reads
            m = (save == -7) | (save == -8)
            m[:, :64, :64] = False
            assert (m[:, :, 126] & m[:, :, 127]).any(), f"q{q} comp {comp}: no -7 / -8 pair ending at column 127"
            assert (m[:, :, :-1] & m[:, :, 1:]).sum() > 100
            ll = save[:, :64, :64]
            assert (ll == 255).any() and (ll == 256).any(), f"q{q} comp {comp}: no LL cell of exactly 255 and 256 ({(ll == 255).sum()}, {(ll == 256).sum()})"
            # ---- every cell of every plane
            for i in range(n):
                for name, got, want in zip(("cproc", "cl2save", "cll1 + neighbour"), fused[i], staged[i]):
                    bad = np.flatnonzero(got.ravel() != want.ravel())
                    assert bad.size == 0, f"q{q} comp {comp} image {i} {name}: {bad.size} cells differ, first {bad[:8].tolist()}"
    finally:
        e.close()
    return n


def check_case(imgs, q, compat=False):
    """every plane the fused kernel writes, every cell of every image; returns the number of images compared"""
    import torch
    import nhwcodec_amd
    n = len(imgs)
    fork_on = os.environ.get("NHW_CHROMA_FORK", "1") != "0"
    e = nhwcodec_amd.Encoder(0, max_batch=n)

    def rd(buf, i, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert e.lib.nhw_debug_read(e.h, buf, i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(nbytes)) == 0
        return out.view(np.int16)

    try:
        if compat:
            e.set_compat(True)
        files = e.encode(imgs, q)                                   # the production path
        prod_save = {0: [rd(B_CL2SAVE, i, Q // 2) for i in range(n)] if fork_on else None,   # (in line, V's block has gone over U's in the one plane set)
                     1: [rd(ws_index("CL2SAVE_V") if fork_on else B_CL2SAVE, i, Q // 2) for i in range(n)]}
        fused = {}
        for comp in (0, 1):
            assert e.lib.nhw_stage_chroma_loops(e.h, n, comp, 0, None) == 0, "nhw_stage_chroma_loops"
            torch.cuda.synchronize()
            fused[comp] = [(rd(B_CPROC, i, 2 * Q), rd(B_CL2SAVE, i, Q // 2), rd(B_CLL1, i, Q // 2 + 2)) for i in range(n)]
        d_in = torch.from_numpy(imgs).cuda()
        try:
            for comp in (0, 1):
                e.lib.nhw_debug_stop_after(e.h, _luma_stages(q) + 12 * comp + 11)   # the staged kernels, stopped behind the second synthesis
                e.encode_device(d_in, q)
                torch.cuda.synchronize()
                for i in range(n):
                    staged = (rd(B_CPROC, i, 2 * Q), rd(B_CL2SAVE, i, Q // 2), rd(B_CLL1, i, Q // 2 + 2))
                    for name, got, want in (("cproc", fused[comp][i][0], staged[0]), ("cl2save", fused[comp][i][1], staged[1]),
                                            ("cll1 + neighbour", fused[comp][i][2], staged[2])) + \
                            ((("cl2save of the production batch", prod_save[comp][i], staged[1]),) if prod_save[comp] is not None else ()):
                        bad = np.flatnonzero(got != want)
                        assert bad.size == 0, f"q{q} compat={compat} fork={fork_on} comp {comp} image {i} {name}: {bad.size} cells differ, first {bad[:8].tolist()}"
        finally:
            e.lib.nhw_debug_stop_after(e.h, 0)
    finally:
        e.close()
    want = oracle_files(imgs, q, compat)
    bad = [i for i in range(n) if files[i] != want[i]]
    assert not bad, f"q{q} compat={compat} fork={fork_on}: files {bad[:16]} differ from the oracle"
    return n


def run_all_qualities():
    for q in QUALITIES:
        assert check_case(chroma_images(q), q) == N_IMAGES


@pytest.mark.gpu
@pytest.mark.parametrize("q", QUALITIES)
def test_fused_chroma_loops_equal_the_staged_kernels(q):
    """64 generator images a quality, chroma fork on (V in its own plane set in the production batch)."""
    assert check_case(chroma_images(q), q) == N_IMAGES


@pytest.mark.gpu
def test_fused_chroma_loops_without_the_chroma_fork():
    """NHW_CHROMA_FORK=0: U and V share one plane set and run in line.  The switch is read when a handle is made: a fresh child process."""
    env = dict(os.environ, NHW_CHROMA_FORK="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "chroma loops OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("q", [14, 20])
def test_fused_chroma_loops_in_compatibility_mode(q):
    """The cell behind cll1 holds two stale bytes of the 4:2:0 U plane; images 110 .. 931 are ones where that neighbour matters."""
    from oracle.oraclepy import Oracle
    o = Oracle()
    imgs = np.stack([o.synth(i) for i in (110, 117, 924, 925, 931, 0, 1, 2)])
    assert check_case(imgs, q, compat=True) == len(imgs)


@pytest.mark.gpu
@pytest.mark.parametrize("q", [15, 20])
def test_fused_chroma_loops_on_threshold_planes(q):
    """LL1 and the cells round the block written directly (threshold_planes): -7 / -8 pairs ending at column 127, LL cells of 255 and 256,
    pre-compensation differences of exactly 3, 4, 7, 10 -- each asserted on the staged kernels' planes, then every cell compared.  The staged
    kernels themselves are held to the oracle by the stage traces of test_gpu_parity.py; q15 / q20: both forms of the first simulation."""
    assert check_threshold_planes(q) == 32


if __name__ == "__main__":
    run_all_qualities()
    print("chroma loops OK")
