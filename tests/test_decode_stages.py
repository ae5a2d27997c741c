"""The decoder stage by stage against the oracle's checkpoints (pytest -m gpu).

nhw_dec_debug_stop_after ends a batch behind one stage, nhw_dec_debug_read copies a workspace buffer out, and the oracle's decode_probe
gives the same buffer at the same point of decode_image: STAGES (tests/dec_stages.py, shared with tests/test_decode_values.py) is the table
stop -> buffer -> probe id, every row bit for bit.
Stops 4, 5 and 6 are the three instantiations of k_dec_luma_l2q (the block as the shrink leaves it, after the synthesis, production);
they and the whole decode run again under both forced slice orders (nhw_dec_debug_slice_order), the quarters of a file one per launch,
ascending and descending, where a quarter that wrote what another one reads would show.

One batch serves everything: the oracle's files of FILES.  The qualities cross every rule of level 2 that changes with the quality: the
shrink's diagonal threshold (16 up to q16, 8 above), res1 (open above q12; amplitude 9, 7, 5 by quality), res3 (from q19), res5 (from q21).
The seeds were picked on the CPU, from the oracle's probes alone, so that the whole of FILES meets reach() below.  Seeds 0 and 1 of every
quality meet all of it but seven conditions of the shrink: a shrunk cell in block columns 31, 32, 63, 64, 95, 96 (the low band's cells
beside a quarter's border, where a file has a handful of shrunk cells in all) and one in row 127.  Over seeds 0 .. 299 of the six
qualities, a greedy cover (the file that adds most conditions first, the lower seed on a tie, four files a quality at most) took three
files, all of q20: seeds 67, 222 and 277, in place of 0 and 1.  reach() is what keeps the comparisons from passing on files that never
take a path: it caps what the test can miss, it is no tolerance, and it fails the tests, never skips them.
"""
import numpy as np
import pytest

from tests.dec_stages import PROBES, STAGES, run_to as _run

FILES = [(q, seed) for q, seeds in ((10, (0, 1)), (13, (0, 1)), (16, (0, 1)), (17, (0, 1)), (20, (67, 222, 277)), (23, (0, 1))) for seed in seeds]


def reach(files, probes):
    """What the batch must exercise, from the oracle's probes alone -> the list of conditions it misses (empty: none).

    The shrink (probe 3 -> 4), over all files together: a changed cell in both windows of every quarter (block columns 32 p .. 32 p + 31
    and 128 + 32 p ..), in the columns either side of a quarter's border that two quarters decide (32 p - 1, 32 p and the same of the
    high band), in the rows either side of a wavefront's border, whose masks travel through s_edge, and in row 128 and column 128,
    next to the LL2 quadrant.  The residual lists (probe 5 -> 50: res5, 50 -> 51: res1, 51 -> 6: res3), for every file and every list
    that is open at its quality: a changed cell in each band of 64 rows, a quarter's share.  And res3 over all files together: an entry
    of the last row of a band whose second cell lies in the next band, which the kernel's quarters share between them -- an odd change
    in row 64, 128 or 192, since of res3's steps (4, 3, 2) only the 3 is odd and it is the step of an entry's second row."""
    missed = []
    shrunk = np.zeros((256, 256), bool)
    for pr in probes:
        d = pr[3].reshape(512, 512) != pr[4].reshape(512, 512)
        if d[256:].any() or d[:, 256:].any() or d[:128, :128].any():
            missed.append("the shrink changed a cell outside the three detail quadrants of the block")
        shrunk |= d[:256, :256]
    for p in range(4):
        for w, c0 in enumerate((32 * p, 128 + 32 * p)):
            if not shrunk[:, c0:c0 + 32].any():
                missed.append(f"shrink: no cell in window {w} of quarter {p}")
    for c in [c for p in (1, 2, 3) for c in (32 * p - 1, 32 * p, 128 + 32 * p - 1, 128 + 32 * p)] + [128]:
        if not shrunk[:, c].any():
            missed.append(f"shrink: no cell in block column {c}")
    for r in (63, 64, 127, 128, 191, 192):
        if not shrunk[r].any():
            missed.append(f"shrink: no cell in block row {r}")
    across = np.zeros(512, bool)
    for (q, seed), pr in zip(files, probes):
        across |= (((pr[6].astype(np.int32) - pr[51]) & 1) != 0).reshape(512, 512).any(1)
        for name, a, b, open_ in (("res5", 5, 50, q >= 21), ("res1", 50, 51, q > 12), ("res3", 51, 6, q >= 19)):
            d = (pr[a] != pr[b]).reshape(512, 512)
            if not open_:
                if d.any():
                    missed.append(f"q{q} seed {seed}: {name} is closed and changed a cell")
                continue
            for band in range(4):
                if not d[64 * band:64 * band + 64, :256].any():
                    missed.append(f"q{q} seed {seed}: {name} changed no cell of rows {64 * band} .. {64 * band + 63}")
    for r in (64, 128, 192):
        if not across[r]:
            missed.append(f"res3: no entry of row {r - 1} that steps row {r} too")
    return missed


@pytest.fixture(scope="module")
def batch(oracle):
    """(files, per file {probe id: int16 array}, per file the oracle's pixels): computed once, read only"""
    files = [oracle.encode(oracle.synth(seed), q) for q, seed in FILES]
    probes = [{i: np.frombuffer(oracle.decode_probe(f, i), np.int16) for i in PROBES} for f in files]
    missed = reach(FILES, probes)
    assert not missed, "FILES no longer reaches what the stage checks are there for:\n  " + "\n  ".join(missed)
    return files, probes, [oracle.decode(f) for f in files]


@pytest.fixture(scope="module")
def dec():
    import nhwcodec_amd
    d = nhwcodec_amd.Decoder(0, max_batch=len(FILES))
    yield d
    d.close()


def test_files_reach_every_rule(batch):
    """reach() on the CPU (the fixture asserts it): a change to the oracle or to FILES that empties a condition shows without a GPU"""
    assert len(batch[0]) == len(FILES)


@pytest.mark.gpu
@pytest.mark.parametrize("stop,mode", [(s, 0) for s in sorted(STAGES)] + [(s, m) for m in (1, 2) for s in (4, 5, 6)])
def test_stage_matches_oracle(dec, batch, stop, mode):
    files, probes, _ = batch
    _run(dec, files, stop, mode)
    bad = []
    for i, (q, seed) in enumerate(FILES):
        for tag, gpu, want in STAGES[stop]:
            pr = probes[i].__getitem__
            g, o = gpu(dec, i, pr), want(pr)
            if g.shape != o.shape:
                bad.append(f"q{q} seed {seed}, {tag}: shape {g.shape}, the oracle's {o.shape}")
            elif not np.array_equal(g, o):
                at = np.argwhere(g != o)
                bad.append(f"q{q} seed {seed}, {tag}: {len(at)} cells differ, first {at[0].tolist()} (GPU {g[tuple(at[0])]}, oracle {o[tuple(at[0])]}), "
                           f"spanning {at.min(0).tolist()} .. {at.max(0).tolist()}")
    assert not bad, f"stop {stop}, slice order {mode}:\n  " + "\n  ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_pixels_match_oracle(dec, batch, mode):
    """stop 0, the whole decode, on the handle the stops have just been through"""
    files, _, want = batch
    px, qs = _run(dec, files, 0, mode)
    for i, (q, seed) in enumerate(FILES):
        assert qs[i] == want[i][1] == q and np.array_equal(px[i], want[i][0]), f"slice order {mode}: q{q} seed {seed} decodes differently from the oracle"
