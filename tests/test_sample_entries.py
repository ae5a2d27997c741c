"""The twenty public entries of the samplers (DESIGN.md sections 18 to 25) -- ten over device pictures (nhw_*_to_tensor_device), ten over .nhwp
containers (nhw_dec_crops_*, nhw_dec_warps_*) -- at their checks, and a small walk over every arm of the one launch behind them.

The entries are one body a side and a row of a descriptor table each; what a caller sees of a refusal is the return code and the text of
nhw_last_error / nhw_dec_last_error, and both are pinned here for every entry and every refusal: a filter that does not exist, each required
pointer NULL in turn, counts of 0 and 2^24 + 1, output sides of 0 and 4097, a format of the other family, a tensor address that is no multiple
of the element size.  The expected texts are written out below, taken from the sources as they were before the entries shared a body; none is
derived from the code under test.  Every refusal comes before anything is launched or uploaded: the destination bytes and the statuses are
looked at afterwards.

The walk is two pictures of 5 x 3 and 9 x 7 into 4 x 4 tensors, one of them mirrored: each filter and the warp, colour and grey, uint8 HWC and
float32 CHW, without tables, with maps, with tone tables, with both.  Each direct entry is compared with the same call through the Python
layer, and the calls with tables -- the identity map, tone_identity() -- with the call without: the bytes sections 24 and 25 define to be equal.
9 x 7 to 4 x 4 is inside the area and cubic filters' limits; a 4-wide output is narrower than one pass of a band, so the band rule's least
rows and the walk's `c += 1 << lg` tail both run.  One warp is steep enough for the block walk, the other is not."""
import ctypes

import numpy as np
import pytest

from tests.support import CANARY

pytestmark = pytest.mark.gpu
NHW_E_ARG = -4
MANY = (1 << 24) + 1

BAD = "bad argument"
THREE = ": the filter must be NHW_FILTER_TWO_TAP, NHW_FILTER_AREA or NHW_FILTER_CUBIC"
TWO = ": the filter must be NHW_FILTER_TWO_TAP or NHW_FILTER_AREA"
SIDES = ": an output side outside 1 .. 4096"
NOT_COLOUR = "tensor format: unknown dtype, layout, channels or rows value"
NOT_GREY = "tensor format: a grey decode takes NHW_T_GREY, not NHW_T_BGR or NHW_T_RGB"
DEST = ": a destination needs an address that is a multiple of the element size"
BY_FILTER = ("nhw_resize_to_tensor_device", "nhw_area_to_tensor_device", "nhw_resample_to_tensor_device")


class Entry:
    """name: the C entry; args: its arguments in order, by the names of a call's values; family: "colour", "grey" or "format" (by the format);
    filter_who: the entry a filter's refusal names; sides_who: the entry the sides' refusal names, or one a filter; two: it takes two filters"""

    def __init__(self, name, args, family, filter_who=None, sides_who=None, two=False):
        self.name, self.args, self.family, self.two = name, args.split(), family, two
        self.filter_who, self.sides_who = filter_who or name, sides_who or name
        self.count = "nr" if "rects" in self.args else "n"
        self.host = "rects" in self.args
        # every pointer but the flags, the stream and a toned entry's maps
        self.required = [a for a in self.args if a in ("d", "blob", "off", "rects", "status", "pics", "addr", "warps", "tones") or (a == "maps" and "tones" not in self.args)]


DEVICE = [
    Entry("nhw_resize_to_tensor_device", "pics n ow oh fmt flags addr stream", "colour"),
    Entry("nhw_area_to_tensor_device", "pics n ow oh fmt flags addr stream", "colour"),
    Entry("nhw_resample_to_tensor_device", "pics n ow oh filter fmt flags addr stream", "colour", sides_who=BY_FILTER),
    Entry("nhw_warp_to_tensor_device", "pics n ow oh fmt warps addr stream", "colour"),
    Entry("nhw_resample_grey_to_tensor_device", "pics n ow oh filter fmt flags addr stream", "grey"),
    Entry("nhw_warp_grey_to_tensor_device", "pics n ow oh fmt warps addr stream", "grey"),
    Entry("nhw_resample_mapped_to_tensor_device", "pics n ow oh filter fmt flags maps addr stream", "format"),
    Entry("nhw_warp_mapped_to_tensor_device", "pics n ow oh fmt warps maps addr stream", "format"),
    Entry("nhw_resample_toned_to_tensor_device", "pics n ow oh filter fmt flags maps tones addr stream", "format"),
    Entry("nhw_warp_toned_to_tensor_device", "pics n ow oh fmt warps maps tones addr stream", "format"),
]
HEAD = "d blob off nc rects nr scale ow oh fmt "
HOST = [
    Entry("nhw_dec_crops_to_device", HEAD + "flags addr status", "colour"),
    Entry("nhw_dec_crops_to_device_filter", HEAD + "flags addr status filter", "colour", filter_who="nhw_dec_crops_to_device", sides_who="nhw_dec_crops_to_device", two=True),
    Entry("nhw_dec_crops_to_device_resample", HEAD + "flags addr status filter", "colour", sides_who="nhw_dec_crops_to_device"),
    Entry("nhw_dec_warps_to_device", HEAD + "warps addr status", "colour"),
    Entry("nhw_dec_crops_grey_to_device", HEAD + "flags addr status filter", "grey"),
    Entry("nhw_dec_warps_grey_to_device", HEAD + "warps addr status", "grey"),
    Entry("nhw_dec_crops_mapped_to_device", HEAD + "flags maps addr status filter", "format"),
    Entry("nhw_dec_warps_mapped_to_device", HEAD + "warps maps addr status", "format"),
    Entry("nhw_dec_crops_toned_to_device", HEAD + "flags maps tones addr status filter", "format"),
    Entry("nhw_dec_warps_toned_to_device", HEAD + "warps maps tones addr status", "format"),
]


def refusals(e, formats):
    """(what, the values that differ from a good call's, the message) of every refusal of entry e; formats: name -> the format's C struct"""
    sides = lambda f: (e.sides_who if isinstance(e.sides_who, str) else e.sides_who[f]) + SIDES   # noqa: E731
    if "filter" in e.args:
        for f in (-1, 3):
            yield f"filter {f}", dict(filter=f), e.filter_who + (TWO if e.two else THREE)
    if e.two:
        yield "the cubic filter", dict(filter=2), e.filter_who + TWO
    for p in e.required:
        yield f"{p} NULL", {p: None}, BAD
    for n in (0, MANY):
        yield f"{e.count} = {n}", {e.count: n}, BAD
    for f in ((0, 1, 2) if not isinstance(e.sides_who, str) else (0,)):
        yield f"a width of 0, filter {f}", dict(ow=0, filter=f), sides(f)
        yield f"a height of 4097, filter {f}", dict(oh=4097, filter=f), sides(f)
    if e.family == "colour":
        yield "a grey format", dict(fmt=formats["grey"]), NOT_COLOUR
    if e.family == "grey":
        yield "a BGR format", dict(fmt=formats["bgr"]), NOT_GREY
    if e.host:
        yield "a misaligned float32 tensor", dict(fmt=formats["grey f32" if e.family == "grey" else "bgr f32"], addr="misaligned"), e.sides_who + DEST


def _formats(na):
    f = {"bgr": na.TensorFormat("uint8", "HWC", "BGR", "file"), "grey": na.TensorFormat("uint8", "HWC", "GREY", "file"),
         "bgr f32": na.TensorFormat("float32", "CHW", "RGB", "reversed", scale=(0.5, 0.25, 2.0), bias=(1.0, -3.0, 0.125)),
         "grey f32": na.TensorFormat("float32", "CHW", "GREY", "reversed", scale=0.5, bias=-3.0)}
    return f, {k: ctypes.pointer(v.c_struct()) for k, v in f.items()}


def test_the_tables_name_the_twenty_entries():
    import nhwcodec_amd as na
    L = na._library()
    names = [e.name for e in DEVICE + HOST]
    assert len(set(names)) == 20 and all(hasattr(L, n) for n in names)


def test_device_entries_refuse_in_their_own_words():
    import torch
    import nhwcodec_amd as na
    L = na._library()
    _, structs = _formats(na)
    out = torch.full((2 * 4 * 4 * 3 * 4 + 16,), CANARY, dtype=torch.uint8, device="cuda")
    one = [torch.zeros(1, dtype=torch.uint8, device="cuda") for _ in range(4)]          # what a table's pointer is where the call never reads it
    addr = torch.tensor([out.data_ptr(), out.data_ptr() + 4 * 4 * 3 * 4], dtype=torch.int64, device="cuda")
    good = dict(pics=one[0].data_ptr(), n=2, ow=4, oh=4, filter=0, flags=None, warps=one[1].data_ptr(), maps=one[2].data_ptr(), tones=one[3].data_ptr(),
                addr=addr.data_ptr(), stream=None)
    done = 0
    for e in DEVICE:
        fmt = structs["grey" if e.family == "grey" else "bgr"]
        for what, change, words in refusals(e, structs):
            v = dict(good, fmt=fmt)
            v.update(change)
            assert L.nhw_hist_device(one[0].data_ptr(), 1, 2, one[1].data_ptr(), None) == NHW_E_ARG                 # another message in between
            assert L.nhw_last_error().decode() == "nhw_hist_device: channels must be 3 or 1"
            rc = getattr(L, e.name)(*[v[a] for a in e.args])
            assert (rc, L.nhw_last_error().decode()) == (NHW_E_ARG, words), (e.name, what)
            done += 1
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and done == 86


@pytest.fixture(scope="module")
def decoder():
    import nhwcodec_amd as na
    d = na.Decoder(0, max_batch=2)
    yield d
    d.close()


def _host_values(na, out):
    """a good call's values for the container entries, but for a container that is none: 8 bytes no refusal here gets to"""
    keep = dict(blob=np.zeros(8, np.uint8), off=np.array([0, 8], np.uint64), rects=np.zeros(1, na.RECT_DTYPE), status=np.full(1, 99, np.int32),
                warps=np.zeros(1, na.WARP_DTYPE), maps=np.zeros(1, na.COLOUR_DTYPE), tones=np.zeros((1, 768), np.uint8), addr=np.array([out.data_ptr()], np.uint64),
                misaligned=np.array([out.data_ptr() + 2], np.uint64))
    keep["rects"][0] = (0, 0, 0, 8, 8)
    v = {k: a.ctypes.data for k, a in keep.items()}
    v.update(nc=1, nr=1, scale=1, ow=4, oh=4, filter=0, flags=None)
    return keep, v


def _stamp(dec, v):
    """leaves another message in nhw_dec_last_error"""
    assert dec.lib.nhw_dec_batch_scaled(dec.h, v["blob"], v["off"], 1, 3, v["blob"], v["status"], None) == NHW_E_ARG
    assert dec.lib.nhw_dec_last_error().decode() == "the scale must be 1, 2 or 4"


def test_container_entries_refuse_in_their_own_words(decoder):
    import torch
    import nhwcodec_amd as na
    _, structs = _formats(na)
    out = torch.full((4 * 4 * 3 * 4 + 16,), CANARY, dtype=torch.uint8, device="cuda")
    keep, good = _host_values(na, out)
    L, done = decoder.lib, 0
    for e in HOST:
        fmt = structs["grey" if e.family == "grey" else "bgr"]
        for what, change, words in refusals(e, structs):
            v = dict(good, d=decoder.h, fmt=fmt)
            v.update(change)
            if v["addr"] == "misaligned":
                v["addr"] = good["misaligned"]
            _stamp(decoder, good)
            rc = getattr(L, e.name)(*[v[a] for a in e.args])
            assert (rc, L.nhw_dec_last_error().decode()) == (NHW_E_ARG, words), (e.name, what)
            done += 1
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and keep["status"].tolist() == [99] and done == 135


def test_two_mistakes_at_once_tell_the_crop_entries_apart(decoder):
    """a filter that does not exist together with a NULL dst_addr: the newest entry looks at the filter first, the two older ones at dst_addr
    (nhw_dec_crops_to_device takes no filter: there the NULL dst_addr is the one mistake)"""
    import torch
    import nhwcodec_amd as na
    _, structs = _formats(na)
    out = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
    keep, good = _host_values(na, out)
    L = decoder.lib
    for e, words in zip(HOST[:3], (BAD, BAD, "nhw_dec_crops_to_device_resample" + THREE)):
        v = dict(good, d=decoder.h, fmt=structs["bgr"], filter=3, addr=None)
        _stamp(decoder, good)
        rc = getattr(L, e.name)(*[v[a] for a in e.args])
        assert (rc, L.nhw_dec_last_error().decode()) == (NHW_E_ARG, words), e.name
    assert keep["status"].tolist() == [99]


# ---------------------------------------------------------------- every arm of the launch
SIZE = (4, 4)
FLIPS = [True, False]
KINDS = ("two_tap", "area", "cubic", "warp")


class Walk:
    pass


@pytest.fixture(scope="module")
def walk():
    import torch
    import nhwcodec_amd as na
    w = Walk()
    rng = np.random.default_rng(2801)
    w.pics = {3: [torch.from_numpy(rng.integers(0, 256, (h, wd, 3), dtype=np.uint8)).cuda() for wd, h in ((5, 3), (9, 7))],
              1: [torch.from_numpy(rng.integers(0, 256, (h, wd), dtype=np.uint8)).cuda() for wd, h in ((5, 3), (9, 7))]}
    # a gentle turn of the mirrored 5 x 3 picture (the row walk: |d| <= 1/4) and a steep one of the 9 x 7 one (the block walk); both reach outside
    w.mats = [na.crop_warp(0, 0, 5, 3, SIZE, angle=0.05, flip=True), na.crop_warp(0, 0, 9, 7, SIZE, angle=1.2)]
    fixed = [na.warp_fixed(m) for m in w.mats]
    assert abs(fixed[0][3]) <= 16384 < abs(fixed[1][3])
    w.fill = {3: (201, 17, 94), 1: 201}
    w.warps = {c: na._warp_table(fixed, na._warp_border(w.fill[c], "fill", "walk", c)[0], 0) for c in (3, 1)}
    w.colours = {3: [np.eye(3, 4)] * 2, 1: [(1.0, 0.0)] * 2}
    w.tones = {3: [na.tone_identity()] * 2, 1: [np.arange(256, dtype=np.uint8)] * 2}
    return w


def _direct(w, name, channels, fmt, kind, tables):
    """one of the ten device entries, called as C callers do -> the tensor's bits"""
    import torch
    import nhwcodec_amd as na
    from tests.tensor_cases import tensor_bits
    L = na._library()
    table, _, dev = na._picture_table(w.pics[channels], "walk", channels=channels)
    out = torch.empty((2,) + fmt.shape(*SIZE), dtype=fmt.dtype, device=dev)
    addr = torch.tensor([out[i].data_ptr() for i in range(2)], dtype=torch.int64, device=dev)
    c = fmt.c_struct()
    held = []
    for kind_of, t in tables:
        if t is None:
            held.append(None)
        elif kind_of == "maps":
            held.append(na._device_table(na._colour_table(t, 2, "walk", channels), dev))
        else:
            held.append(torch.from_numpy(na._tone_arg(t, 2, "walk", channels)).to(dev))
    extra = [t.data_ptr() if t is not None else None for t in held]
    if kind == "warp":
        d_w = torch.from_numpy(w.warps[channels].view(np.int64).copy()).to(dev)
        rc = getattr(L, name)(table.data_ptr(), 2, SIZE[1], SIZE[0], ctypes.byref(c), d_w.data_ptr(), *extra, addr.data_ptr(), None)
    else:
        flags = torch.tensor(FLIPS, dtype=torch.uint8, device=dev)
        f = () if name in BY_FILTER[:2] else (na.RESAMPLERS[kind],)
        rc = getattr(L, name)(table.data_ptr(), 2, SIZE[1], SIZE[0], *f, ctypes.byref(c), flags.data_ptr(), *extra, addr.data_ptr(), None)
    assert rc == 0, (name, L.nhw_last_error())
    torch.cuda.synchronize()
    return tensor_bits(out)


def _python(w, channels, fmt, kind, colours, tones):
    """the same call through the Python layer -> the tensor's bits"""
    import nhwcodec_amd as na
    from tests.tensor_cases import tensor_bits
    if kind == "warp":
        call = na.warp_to_tensor_device if channels == 3 else na.warp_grey_to_tensor_device
        return tensor_bits(call(w.pics[channels], w.mats, SIZE, fmt, fill=w.fill[channels], border="fill", colours=colours, tones=tones))
    call = na.resize_to_tensor_device if channels == 3 else na.resize_grey_to_tensor_device
    return tensor_bits(call(w.pics[channels], SIZE, fmt, flips=FLIPS, filter=kind, colours=colours, tones=tones))


@pytest.mark.parametrize("channels", (3, 1))
def test_every_arm_lands_where_it_did(walk, channels):
    import nhwcodec_amd as na
    fmts, _ = _formats(na)
    stem = {"warp": "nhw_warp"}
    plain_bytes = {}
    for fmt in (fmts["bgr" if channels == 3 else "grey"], fmts["bgr f32" if channels == 3 else "grey f32"]):
        for kind in KINDS:
            s = stem.get(kind, "nhw_resample")
            plain = _direct(walk, f"{s}{'_grey' if channels == 1 else ''}_to_tensor_device", channels, fmt, kind, ())
            assert plain.shape == (2,) + fmt.shape(*SIZE)
            if channels == 3 and kind in ("two_tap", "area"):        # the two older entries are their filter of the newest
                assert np.array_equal(_direct(walk, BY_FILTER[na.RESAMPLERS[kind]], 3, fmt, kind, ()), plain), (kind, fmt.dtype)
            if fmt.dtype_name == "uint8":
                plain_bytes[kind] = plain
            maps, tones = walk.colours[channels], walk.tones[channels]
            for what, entry, tables, colours, tabs in (("plain", None, (), None, None),
                                                       ("mapped", f"{s}_mapped_to_tensor_device", (("maps", maps),), maps, None),
                                                       ("toned, no maps", f"{s}_toned_to_tensor_device", (("maps", None), ("tones", tones)), None, tones),
                                                       ("toned, with maps", f"{s}_toned_to_tensor_device", (("maps", maps), ("tones", tones)), maps, tones)):
                if entry is not None:
                    assert np.array_equal(_direct(walk, entry, channels, fmt, kind, tables), plain), (kind, fmt.dtype, what, "the direct entry")
                assert np.array_equal(_python(walk, channels, fmt, kind, colours, tabs), plain), (kind, fmt.dtype, what, "through Python")
    # four rules, four kernels: on the 9 x 7 picture no two of them give the same bytes
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(plain_bytes[KINDS[a]][1], plain_bytes[KINDS[b]][1]), (KINDS[a], KINDS[b])
