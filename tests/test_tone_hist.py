"""Histograms and the tables made from them on the device, on the MI355X: k_hist_bytes behind nhw_hist_device against
numpy.bincount, k_tone_from_hist behind nhw_tone_from_hist_device against tone_cases' numpy restatement of equalize and autocontrast on crafted
histograms that need not come from a picture, and the Equalize recipe of tone_from_hist_device's docstring end to end against the whole chain
in numpy.  Every output lies between guards and is filled with garbage first."""
import numpy as np
import pytest

from tests.colour_cases import colour_views, picture_table
from tests.grey_picture_cases import grey_views
from tests.tensor_cases import expected_tensor, tensor_bits, tensor_format
from tests.tone_cases import (AUTOCONTRAST, EQUALIZE, HISTS, KEEP, NHW_E_ARG, apply_tone, autocontrast_row, equalize_row, hist_words, random_hists)

pytestmark = pytest.mark.gpu
# W, H, pitch extra, misalignment: one pixel; an odd address; a padded pitch; one that holds every byte value; a constant one, where every add
# lands on one bin; a tall one, many bands of several rows; a wide one, one row
SOURCES = [(1, 1, 0, 0), (37, 23, 0, 1), (517, 301, 11, 4), (32, 24, 0, 0), (517, 301, 0, 0), (3, 1000, 5, 2), (65535, 1, 0, 3)]
CONSTANT, PADDED = 4, 2
GUARD = 1024                                                          # words


class Sources:
    pass


@pytest.fixture(scope="module")
def sources():
    import torch
    import nhwcodec_amd as na
    s = Sources()
    s.bufs, s.views = {}, {}
    for C in (3, 1):
        buf, views = colour_views(SOURCES, 2521)[:2] if C == 3 else grey_views(SOURCES, 2522)[:2]
        views[CONSTANT].fill_(201)
        v = views[PADDED]
        v.copy_(v % 200)                                             # the padding of the padded-pitch picture holds a value the picture does not
        w, h, extra, _ = SOURCES[PADDED]
        pad = buf.as_strided((h, extra), (C * w + extra, 1), v.storage_offset() + C * w)
        pad.fill_(255)
        assert v.stride(0) == C * w + extra and int(v.max()) < 200 and views[1].data_ptr() % 2 == 1
        s.bufs[C], s.views[C] = buf, views
    s.table = lambda C, which: picture_table([s.views[C][k] for k in which], na)
    s.want = {C: [np.stack([np.bincount(v.cpu().numpy().reshape(-1, C)[:, c], minlength=256) for c in range(C)]) for v in s.views[C]] for C in (3, 1)}
    assert s.want[3][CONSTANT][:, 201].tolist() == [517 * 301] * 3 and s.want[1][PADDED][0, 255] == 0
    return s


def _hist(table, channels):
    """nhw_hist_device over a host picture table into garbage between two guards -> (rc, uint32 [n, C, 256], guards intact)"""
    import torch
    import nhwcodec_amd as na
    L = na._library()
    n = len(table)
    words = n * channels * 256
    host = np.full(2 * GUARD + words, 0x5A5A5A5A, np.uint32)
    host[GUARD:GUARD + words] = np.random.default_rng(2523).integers(1, 1 << 32, words, dtype=np.uint64).astype(np.uint32)      # garbage: the call overwrites
    buf = torch.from_numpy(host.view(np.int32)).cuda()
    d_tab = torch.from_numpy(np.ascontiguousarray(table).view(np.int64).copy()).cuda()
    rc = L.nhw_hist_device(d_tab.data_ptr(), n, channels, buf.data_ptr() + 4 * GUARD, None)
    torch.cuda.synchronize()
    back = buf.cpu().numpy().view(np.uint32)
    intact = bool((back[:GUARD] == 0x5A5A5A5A).all() and (back[GUARD + words:] == 0x5A5A5A5A).all())
    return rc, back[GUARD:GUARD + words].reshape(n, channels, 256), intact


@pytest.mark.parametrize("channels", (3, 1))
def test_histograms_equal_bincount(sources, channels):
    which = list(range(len(SOURCES)))
    table = sources.table(channels, which)
    rc, got, intact = _hist(table, channels)
    assert rc == 0 and intact
    for i, k in enumerate(which):
        assert np.array_equal(got[i], sources.want[channels][k]), f"picture {k} ({SOURCES[k][0]} x {SOURCES[k][1]})"
        assert int(got[i].sum()) == channels * SOURCES[k][0] * SOURCES[k][1]
    rc, again, intact = _hist(table, channels)                       # twice: integer sums, the same words
    assert rc == 0 and intact and np.array_equal(got, again)
    one = _hist(table[PADDED:PADDED + 1], channels)                     # one picture: 64 bands
    assert one[0] == 0 and one[2] and np.array_equal(one[1][0], sources.want[channels][PADDED])


@pytest.mark.parametrize("channels", (3, 1))
def test_entries_that_count_nothing_and_many_entries(sources, channels):
    which = [1, 3, 2, 1, 3]
    table = sources.table(channels, which)
    table[1]["addr"] = 0                                              # a zero address between two real ones
    table[3]["width"] = 0
    table[4]["height"] = 65536
    rc, got, intact = _hist(table, channels)
    assert rc == 0 and intact
    for i, k in enumerate(which):
        if i in (1, 3, 4):
            assert not got[i].any(), f"entry {i} counted something"
        else:
            assert np.array_equal(got[i], sources.want[channels][k]), i
    # more entries than the band rule has workgroups for: one band a picture
    n = 8200
    which = [(1, 3, 0, 5)[i % 4] for i in range(n)]
    rc, got, intact = _hist(sources.table(channels, which), channels)
    assert rc == 0 and intact
    want = np.stack([sources.want[channels][k] for k in which])
    assert np.array_equal(got, want)


def test_hist_refusals_and_the_python_layer(sources):
    import torch
    import nhwcodec_amd as na
    L = na._library()
    table = sources.table(3, [1, 3])
    d_tab = torch.from_numpy(np.ascontiguousarray(table).view(np.int64).copy()).cuda()
    out = torch.full((2 * 3 * 256,), 7, dtype=torch.int32, device="cuda")
    for args in ((None, 2, 3, out.data_ptr()), (d_tab.data_ptr(), 2, 3, None), (d_tab.data_ptr(), 0, 3, out.data_ptr()), (d_tab.data_ptr(), (1 << 24) + 1, 3, out.data_ptr()),
                 (d_tab.data_ptr(), 2, 0, out.data_ptr()), (d_tab.data_ptr(), 2, 2, out.data_ptr()), (d_tab.data_ptr(), 2, 4, out.data_ptr())):
        assert L.nhw_hist_device(*args, None) == NHW_E_ARG, args[1:3]
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                    # nothing was zeroed, nothing launched
    for C in (3, 1):
        h = na.hist_device([sources.views[C][k] for k in (2, 3, 4)])
        assert h.dtype == torch.int64 and tuple(h.shape) == (3, C, 256) and h.is_cuda
        assert np.array_equal(h.cpu().numpy(), np.stack([sources.want[C][k] for k in (2, 3, 4)]))
    with pytest.raises(na.NhwError):
        na.hist_device([sources.views[3][1], sources.views[1][1]])


# ---------------------------------------------------------------- tables from histograms
def _crafted(channels):
    """the crafted histograms and seeded ones as [n][C][256]"""
    hists = list(HISTS.values()) + random_hists(3 * 8 - len(HISTS) % 3, 2524)
    hists = hists[:len(hists) // channels * channels]
    return np.stack(hists).reshape(-1, channels, 256)


def _tone_from_hist(hists, ops, channels, seed=2525):
    """nhw_tone_from_hist_device over uploaded histograms into seeded garbage tables between two guards -> (rc, uint8 [n, 768], the garbage, guards intact)"""
    import torch
    import nhwcodec_amd as na
    n = len(hists)
    guard = 4096
    garbage = np.random.default_rng(seed).integers(0, 256, n * 768, dtype=np.uint8)
    host = np.concatenate([np.full(guard, 0xA5, np.uint8), garbage, np.full(guard, 0xA5, np.uint8)])
    buf = torch.from_numpy(host).cuda()
    d_h = torch.from_numpy(hist_words(hists)).cuda()
    d_ops = torch.tensor(ops, dtype=torch.uint8).cuda()
    rc = na._library().nhw_tone_from_hist_device(d_h.data_ptr(), n, channels, d_ops.data_ptr(), buf.data_ptr() + guard, None)
    torch.cuda.synchronize()
    back = buf.cpu().numpy()
    intact = bool((back[:guard] == 0xA5).all() and (back[guard + n * 768:] == 0xA5).all())
    return rc, back[guard:guard + n * 768].reshape(n, 768), garbage.reshape(n, 768), intact


@pytest.mark.parametrize("channels", (3, 1))
def test_tables_from_crafted_histograms(channels):
    hists = _crafted(channels)
    n = len(hists)
    assert n * channels >= len(HISTS)
    rules = {EQUALIZE: equalize_row, AUTOCONTRAST: autocontrast_row}
    for ops in ([EQUALIZE] * n, [AUTOCONTRAST] * n, [(KEEP, EQUALIZE, AUTOCONTRAST, 3, 255, AUTOCONTRAST, EQUALIZE, 128)[i % 8] for i in range(n)]):
        rc, got, garbage, intact = _tone_from_hist(hists, ops, channels)
        assert rc == 0 and intact
        for k in range(n):
            if ops[k] in rules:
                for c in range(channels):
                    assert np.array_equal(got[k, 256 * c:256 * (c + 1)], rules[ops[k]](hists[k, c])), (ops[k], k, c)
                assert np.array_equal(got[k, 256 * channels:], garbage[k, 256 * channels:]), f"sample {k}: a row beyond the {channels} channels was written"
            else:                                                    # keep, and every op that is none of the three: byte for byte as it was
                assert np.array_equal(got[k], garbage[k]), (ops[k], k)


def test_table_refusals_and_the_python_layer():
    import torch
    import nhwcodec_amd as na
    L = na._library()
    hists = _crafted(3)
    n = len(hists)
    d_h = torch.from_numpy(hist_words(hists)).cuda()
    d_ops = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_t = torch.full((n, 768), 9, dtype=torch.uint8, device="cuda")
    for args in ((None, n, 3, d_ops.data_ptr(), d_t.data_ptr()), (d_h.data_ptr(), n, 3, None, d_t.data_ptr()), (d_h.data_ptr(), n, 3, d_ops.data_ptr(), None),
                 (d_h.data_ptr(), 0, 3, d_ops.data_ptr(), d_t.data_ptr()), (d_h.data_ptr(), n, 2, d_ops.data_ptr(), d_t.data_ptr())):
        assert L.nhw_tone_from_hist_device(*args, None) == NHW_E_ARG
    torch.cuda.synchronize()
    assert bool((d_t == 9).all())
    h64 = torch.from_numpy(hists.astype(np.int64)).cuda()
    ops = [("keep", "equalize", "autocontrast")[i % 3] for i in range(n)]
    rules = {"equalize": equalize_row, "autocontrast": autocontrast_row}
    ident = np.arange(256, dtype=np.uint8)
    kept = [np.stack([np.roll(ident, 5 * k + c) for c in range(3)]) for k in range(n)]                   # R, G, B rows for the samples that keep theirs
    for tones in (None, kept):
        t = na.tone_from_hist_device(h64, ops, tones=tones)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (n, 768) and t.is_cuda
        t = t.cpu().numpy().reshape(n, 3, 256)
        for k in range(n):
            for c in range(3):
                want = rules[ops[k]](hists[k, c]) if ops[k] in rules else ident if tones is None else kept[k][2 - c]
                assert np.array_equal(t[k, c], want), (ops[k], k, c)
    again = na.tone_from_hist_device(torch.from_numpy(hist_words(hists)).cuda(), ops)                   # the uint32 words as int32
    assert np.array_equal(again.cpu().numpy(), na.tone_from_hist_device(h64, ops).cpu().numpy())
    g = na.tone_from_hist_device(h64[:, :1].contiguous(), ["equalize"] * n)
    g = g.cpu().numpy()
    assert all(np.array_equal(g[k, :256], equalize_row(hists[k, 0])) and np.array_equal(g[k, 256:], np.tile(ident, 2)) for k in range(n))
    for bad in (dict(ops=ops[:-1]), dict(ops=["keep"] * (n - 1) + ["invert"]), dict(ops="equalize"), dict(h=h64.cpu()), dict(h=h64.to(torch.float32)), dict(h=h64[:, :2]),
                dict(h=h64[..., :255]), dict(tones=kept[:-1])):
        with pytest.raises(na.NhwError):
            na.tone_from_hist_device(bad.get("h", h64), bad.get("ops", ops), tones=bad.get("tones"))


# ---------------------------------------------------------------- end to end
def test_the_equalize_recipe():
    """tone_from_hist_device's docstring: a uint8 HWC batch, its histograms, its tables, and the identity resample of the same views with the
    tables into the final format -- against bincount, the numpy rules, a gather and the value rule"""
    import torch
    import nhwcodec_amd as na
    rng = np.random.default_rng(2526)
    h, w = 48, 64
    smooth = np.clip(rng.normal(110, 30, (70, 90, 3)), 0, 255).astype(np.uint8)
    few = rng.choice(np.array([3, 90, 91, 200], np.uint8), (50, 60, 3))                                  # few distinct values
    dark = (rng.integers(0, 256, (80, 100, 3)) // 4 + 20).astype(np.uint8)
    pics = [torch.from_numpy(p).cuda() for p in (smooth, few, dark)]
    bytes_fmt, final = tensor_format("uint8", "HWC", "BGR", "file"), tensor_format("float16", "CHW", "RGB", "reversed")
    batch = na.resize_to_tensor_device(pics, (h, w), bytes_fmt, filter="area")                           # 1. the crops as a uint8 HWC batch
    views = list(batch)
    hist = na.hist_device(views)                                                                         # 2.
    px = batch.cpu().numpy()
    want_hist = np.stack([np.stack([np.bincount(px[k, :, :, c].ravel(), minlength=256) for c in range(3)]) for k in range(3)])
    assert np.array_equal(hist.cpu().numpy(), want_hist)
    for ops, rule in ((["equalize"] * 3, equalize_row), (["autocontrast"] * 3, autocontrast_row)):
        tables = na.tone_from_hist_device(hist, ops)                                                     # 3.
        out = na.resize_to_tensor_device(views, (h, w), final, tones=tables)                             # 4. the identity resample, the table, the value rule
        assert np.array_equal(na.resize_to_tensor_device(views, (h, w), bytes_fmt).cpu().numpy(), px)     # (the identity it is)
        bits = tensor_bits(out)
        for k in range(3):
            table = np.stack([rule(want_hist[k, c]) for c in range(3)])
            assert np.array_equal(tables[k].cpu().numpy().reshape(3, 256), table), (ops[0], k)
            assert np.array_equal(bits[k], expected_tensor(apply_tone(px[k], table), final)), (ops[0], k)
        assert not np.array_equal(tables[2].cpu().numpy().reshape(3, 256)[0], np.arange(256))          # the dark picture is stretched under either rule
