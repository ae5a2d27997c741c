"""The carry paths of pass A of the quality 1..16 pre-filter (k_low_pre): which of them a picture takes, counted on the CPU.

A band's go-back beyond the row above it, its stop at row 0, and the open lanes' hand-over inside a row run only on pictures whose carry never
merges.  tests/prefilter_cases.py makes four such pictures (P1 .. P4) and restates the look-back in numpy; this module asserts, per quality, that
the pictures reach the paths (so that tests/test_prefilter_carry.py runs them on the GPU), that a wrong state on each path would change map
cells, and -- the record of why the pictures are needed -- that the suite's own pictures reach none of them.  The restatement qualifies the inputs
and gives no expected value; its map is checked against the oracle's pass A on every picture.  Run with -s for the census.  No GPU needed."""
import os

import numpy as np
import pytest

from tests import prefilter_cases as pc

TO_ROW_0 = [32 * b + 1 for b in range(1, pc.NB)]


def _census(name, luma, q):
    c = pc.Census(luma, q)
    om = pc.oracle_pass_a(luma, q)
    rewritten = pc.map_agrees(c, om)                                     # the restated map is the oracle's, cell for cell
    s = c.summary()
    print(f"q{q} {name}: depths {s['depths']}; open lanes a row {s['open_min']}..{s['open_max']}, runs >= {s['runs_min']}, longest run "
          f"{s['longest_min']}..{s['longest_max']}; marker rows {c.marker_rows(om)}, cells the marker rule rewrote {rewritten}; cells changed by far "
          f"lanes entered in 0 / in state + 8: {s['far0']} / {s['far_other']} (open lanes alone: {s['open0']} / {s['open_other']})")
    return c, om, s


def _band_sensitivity(name, c, bands):
    """every one of these bands: some other entry state changes cells of the band's first row -> the count of such states a band"""
    out = {}
    for b in bands:
        ch = c.band_entry_changes(b)
        out[b] = sum(1 for v in ch.values() if v)
        assert out[b] > 0, f"{name}: no entry state changes a cell of band {b}'s first row"
    print(f"   {name}: of the 15 other entry states, those that change cells of the band's first row: {out}")
    return out


@pytest.mark.parametrize("q", range(1, 17))
def test_crafted_pictures_reach_the_carry_paths(q):
    lumas = pc.crafted_lumas(q)
    o = pc._oracle()
    for (name, _), y, img in zip(pc.CRAFTED, lumas, pc.crafted_pictures(q)):
        assert img.shape == (512, 512, 3) and np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
        assert np.array_equal(o.color(img, q)[0].astype(np.int64), y.reshape(-1)), f"{name}: the colour stage does not give the luma plane back"
    (c1, _, s1), (c2, _, s2), (c3, _, s3), (c4, om4, s4) = (_census(n, y, q) for (n, _), y in zip(pc.CRAFTED, lumas))

    # P1: every band goes back to row 0, and the state it comes forward with shows in the band's first row
    assert s1["depths"] == TO_ROW_0
    assert len({int(c1.entry[1 + 32 * b]) for b in range(1, pc.NB)}) > 1, "P1: every band starts from the same state"
    _band_sensitivity("P1", c1, range(1, pc.NB))

    # P2: the go-back stops in the middle: either side of the forced three rows, either side of the step into the second band above
    for b, d in pc.P2_DEPTHS.items():
        assert s2["depths"][b - 1] == d, (b, d, s2["depths"])
    assert set(pc.P2_DEPTHS.values()) == {2, 3, 4, 31, 32, 33}
    _band_sensitivity("P2", c2, pc.P2_DEPTHS)

    # P3: open lanes in every row, in many runs, one of them long enough for a third round of the hand-over
    for r, (n_open, runs, longest) in enumerate(c3.open_rows(), 1):
        assert n_open >= 32 and runs >= 8 and longest >= 3, (r, n_open, runs, longest)
    # P4: the same beside noise: rows with markers, open lanes in front of the noise, and (this picture's last lane never merges) the way to row 0
    assert all(n_open >= 1 for n_open, _, _ in c4.open_rows())
    assert c4.open[1:-1, 16].all(), "P4: the noise is not entered from an open lane"
    assert c4.marker_rows(om4) >= 255, "P4: markers in fewer than half of the rows"
    assert s4["depths"] == TO_ROW_0
    for name, s in (("P3", s3), ("P4", s4)):
        assert s["far0"] >= 10000 and s["far_other"] >= 10000, (name, s)
        assert s["open0"] >= 10000 and s["open_other"] >= 10000, (name, s)      # what a hand-over that brought a wrong state would change


def test_the_suites_own_pictures_reach_none_of_these_paths():
    """the record: on the pictures the pre-filter, fallback and encode tests run on, every band's go-back is one row deep and no row has an open
    lane (quality 10; the luma plane of the other qualities is this one scaled)"""
    q = pc.SUITE_Q
    o = pc._oracle()
    for name, img in pc.suite_pictures():
        _, _, s = _census(name, o.color(img, q)[0], q)
        assert max(s["depths"]) == 1 and s["open_max"] == 0, (name, s)


@pytest.mark.parametrize("q", [1, 10, 16])
def test_oracle_follows_the_stock_binary_on_the_crafted_pictures(q):
    """the oracle has never seen such pictures either: its files in the GLIBC_ONESHOT mode against the stock reference binary, outside the bytes
    that binary leaves to un-initialised memory"""
    from oracle.harness import STOCK_ENC, stock_encode, uninitialised_positions
    if not os.path.exists(STOCK_ENC):
        pytest.skip("no stock reference binary")
    o = pc._oracle()
    imgs = pc.crafted_pictures(q)
    o.set_oob_mode(True)
    try:
        want = [o.encode(im, q) for im in imgs]
    finally:
        o.set_oob_mode(False)
    for (name, _), im, w in zip(pc.CRAFTED, imgs, want):
        stock = stock_encode(im, q)
        assert len(stock) == len(w), name
        pad = uninitialised_positions(stock)
        assert [k for k in range(len(stock)) if stock[k] != w[k] and k not in pad] == [], name
