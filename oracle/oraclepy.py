"""ctypes binding of oracle/liboracle.so (the plain-C CPU restatement).  Test infrastructure only."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "liboracle.so")
P = ctypes.c_void_p


class _Trace(ctypes.Structure):
    _fields_ = [("buf", P), ("cap", ctypes.c_size_t), ("len", ctypes.c_size_t), ("count", ctypes.c_int)]


class _StreamInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("status", "select1_pre", "select2_pre", "select1", "select2", "size_data1", "size_data2",
                                            "size_book1", "size_book2", "tree_end", "wavelet_type", "words")]


Q = 65536
ARM_MAX = 128


class _ResidualList(ctypes.Structure):
    _fields_ = [("list_len", ctypes.c_int), ("bits_len", ctypes.c_int), ("word_len", ctypes.c_int), ("raw_count", ctypes.c_int),
                ("list", ctypes.c_uint8 * (Q + 64)), ("bits", ctypes.c_uint8 * (Q // 8 + 64)), ("word", ctypes.c_uint8 * (Q // 4 + 64))]


class _ResidualOut(ctypes.Structure):
    _fields_ = [("pl", _ResidualList * 3), ("arm", ctypes.c_uint32 * ARM_MAX)]


class _ResidualPlanes(ctypes.Structure):
    _fields_ = [("jpeg", ctypes.c_int16 * (4 * Q)), ("proc", ctypes.c_int16 * (4 * Q)), ("ll1", ctypes.c_int16 * Q),
                ("l2save", ctypes.c_int16 * Q), ("first_order", ctypes.c_int16 * Q)]


class _ResidualTap(ctypes.Structure):
    _fields_ = [("inp", _ResidualPlanes), ("out", _ResidualPlanes), ("lists", _ResidualOut)]


RESIDUAL_PLANES = ("jpeg", "proc", "ll1", "l2save", "first_order")


def _planes_dict(p):
    return {k: np.frombuffer(getattr(p, k), np.int16).copy() for k in RESIDUAL_PLANES}


def _lists_dict(out, arm_names=None):
    """nhwo_residual_out -> {"lists": three dicts (list, bits, word as bytes; raw_count), "arms": {name: count}}"""
    r = {"lists": [{"list": bytes(l.list[:l.list_len]), "bits": bytes(l.bits[:l.bits_len]), "word": bytes(l.word[:l.word_len]),
                    "raw_count": l.raw_count} for l in out.pl]}
    if arm_names is not None:
        r["arms"] = {n: int(out.arm[i]) for i, n in enumerate(arm_names)}
    return r


class Oracle:
    def __init__(self, so_path: str = SO):
        L = self.lib = ctypes.CDLL(so_path)
        L.nhwo_synth_image.argtypes = [ctypes.c_uint32, P]
        L.nhwo_color.argtypes = [P, ctypes.c_int, P, P, P]
        L.nhwo_prefilter.argtypes = [P, ctypes.c_int]
        L.nhwo_analysis.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
        L.nhwo_synthesis.argtypes = [P, P, ctypes.c_int, ctypes.c_int]
        L.nhwo_quality_supported.argtypes = [ctypes.c_int]
        L.nhwo_encode.restype = ctypes.c_int
        L.nhwo_encode.argtypes = [P, ctypes.c_int, P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_Trace)]
        L.nhwo_decode.restype = ctypes.c_int
        L.nhwo_decode.argtypes = [P, ctypes.c_size_t, P, ctypes.POINTER(ctypes.c_int)]
        L.nhwo_decode_planes.restype = ctypes.c_int
        L.nhwo_decode_planes.argtypes = [P, ctypes.c_size_t, P, ctypes.POINTER(ctypes.c_int)]
        L.nhwo_dec_bmp_header.argtypes = [P]
        self._out = ctypes.create_string_buffer(1 << 20)

    def decode(self, nhw: bytes, planes: bool = False):
        """.nhw bytes -> uint8[512,512,3] in nhw-dec's output byte order (planes=True: uint8[3,512,512] Y,U,V before the colour matrix)"""
        out = np.empty((3, 512, 512) if planes else (512, 512, 3), np.uint8)
        q = ctypes.c_int(0)
        buf = ctypes.create_string_buffer(bytes(nhw), len(nhw))
        fn = self.lib.nhwo_decode_planes if planes else self.lib.nhwo_decode
        rc = fn(ctypes.cast(buf, P), len(nhw), out.ctypes.data, ctypes.byref(q))
        if rc != 0:
            raise RuntimeError(f"oracle decode failed rc={rc}")
        return out, q.value

    def decode_probe(self, nhw: bytes, probe_id: int, cap: int = 1 << 20) -> bytes:
        """one intermediate buffer of the decode of `nhw` (ids: see probe() calls in nhwo_dec.c)"""
        buf = ctypes.create_string_buffer(cap)
        self.lib.nhwo_dec_probe.argtypes = [ctypes.c_int, P, ctypes.c_size_t]
        self.lib.nhwo_dec_probe_len.restype = ctypes.c_size_t
        self.lib.nhwo_dec_probe(probe_id, ctypes.cast(buf, P), cap)
        try:
            self.decode(nhw, planes=True)
            n = self.lib.nhwo_dec_probe_len()
        finally:
            self.lib.nhwo_dec_probe(0, None, 0)
        return buf.raw[:n]

    def bmp_header(self) -> bytes:
        h = ctypes.create_string_buffer(54)
        self.lib.nhwo_dec_bmp_header(ctypes.cast(h, P))
        return h.raw

    def set_oob_mode(self, glibc_oneshot: bool):
        """False: canonical (out-of-bounds reads see zeros).  True: NHWO_OOB_GLIBC_ONESHOT, the stock binary's heap neighbours (nhwo.h)."""
        ctypes.c_int.in_dll(self.lib, "nhwo_oob_mode").value = 1 if glibc_oneshot else 0

    def synth(self, seed: int) -> np.ndarray:
        b = np.empty((512, 512, 3), np.uint8)
        self.lib.nhwo_synth_image(seed, b.ctypes.data)
        return b

    def color(self, img, q):
        img = np.ascontiguousarray(img, np.uint8)
        y = np.empty(512 * 512, np.int16); u = np.empty(65536, np.uint8); v = np.empty(65536, np.uint8)
        self.lib.nhwo_color(img.ctypes.data, q, y.ctypes.data, u.ctypes.data, v.ctypes.data)
        return y, u, v

    def prefilter(self, y, q):
        y = np.ascontiguousarray(y, np.int16).copy()
        self.lib.nhwo_prefilter(y.ctypes.data, q)
        return y

    def analysis(self, jpeg, stride, n, final_level, keep=False):
        jpeg = np.ascontiguousarray(jpeg, np.int16).copy()
        proc = np.zeros_like(jpeg)
        k = np.zeros(2 * 65536, np.int16) if keep else None
        self.lib.nhwo_analysis(jpeg.ctypes.data, proc.ctypes.data, stride, n, final_level, k.ctypes.data if keep else None)
        return (jpeg, proc, k) if keep else (jpeg, proc)

    def synthesis(self, jpeg, stride, n):
        jpeg = np.ascontiguousarray(jpeg, np.int16).copy()
        proc = np.zeros_like(jpeg)
        self.lib.nhwo_synthesis(jpeg.ctypes.data, proc.ctypes.data, stride, n)
        return jpeg, proc

    def stream_stage(self, luma, chroma, packet_cap: int = 80000) -> dict:
        """nhwo_stream_stage: the symbol rewrites and the packetiser on a stream of the caller's (luma: uint8[262144] as the gather leaves
        it, chroma: uint8[131072] as the chroma quantisers leave it).  -> the rewritten luma part, the packet words (the first
        min(words, packet_cap)), both books, both sign-word arrays and every scalar of nhwo_stream_info."""
        luma = np.ascontiguousarray(luma, np.uint8); chroma = np.ascontiguousarray(chroma, np.uint8)
        assert luma.size == 4 * 65536 and chroma.size == 2 * 65536
        out = np.empty(4 * 65536, np.uint8)
        s1 = np.zeros(4 * 65536 // 8 + 8, np.uint8); s2 = np.zeros_like(s1)
        pk = np.zeros(packet_cap, np.uint32)
        b1 = np.zeros(708, np.uint8); b2 = np.zeros(708, np.uint8)
        info = _StreamInfo()
        fn = self.lib.nhwo_stream_stage
        fn.restype = ctypes.c_int
        fn.argtypes = [P, P, P, P, P, P, ctypes.c_size_t, P, P, ctypes.POINTER(_StreamInfo)]
        rc = fn(luma.ctypes.data, chroma.ctypes.data, out.ctypes.data, s1.ctypes.data, s2.ctypes.data, pk.ctypes.data, packet_cap,
                b1.ctypes.data, b2.ctypes.data, ctypes.byref(info))
        r = {k: getattr(info, k) for k, _ in _StreamInfo._fields_}
        assert rc == r["status"]
        r.update(luma=out, packet=pk[:min(r["words"], packet_cap)], book1=b1[:r["size_book1"]], book2=b2[:r["size_book2"]],
                 sel_word1=s1[:r["select1"]], sel_word2=s2[:r["select2"]])
        return r

    def arm_names(self):
        L = self.lib
        L.nhwo_arm_name.restype = ctypes.c_char_p
        return [L.nhwo_arm_name(i).decode() for i in range(L.nhwo_arm_count())]

    def live_arms(self, q: int):
        """the arm counters (by name) whose arm can be taken at quality q"""
        return [n for i, n in enumerate(self.arm_names()) if self.lib.nhwo_arm_live(i, int(q))]

    def residual_stage(self, q, jpeg, proc, ll1, l2save, first_order=None, first=0, last=2) -> dict:
        """nhwo_residual_stage: parts first .. last (0: Y19 .. Y23, 1: Y24 and Y25, 2: Y26 and Y27) of the residual passes on planes of the
        caller's (int16; jpeg, proc: 512 x 512; ll1, l2save, first_order: 256 x 256).  -> the five planes behind the passes (flat), "lists"
        (res1, res3, res5: list, bits and word bytes, the raw entry count) and "arms" (the arm counters of this call by name)."""
        a = [np.ascontiguousarray(x, np.int16).ravel().copy() for x in
             (jpeg, proc, ll1, l2save, np.zeros(Q, np.int16) if first_order is None else first_order)]
        assert [x.size for x in a] == [4 * Q, 4 * Q, Q, Q, Q]
        out = _ResidualOut()
        fn = self.lib.nhwo_residual_stage
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P, P, ctypes.POINTER(_ResidualOut)]
        rc = fn(int(q), int(first), int(last), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data,
                ctypes.byref(out))
        if rc != 0:
            raise RuntimeError(f"oracle residual stage failed rc={rc}")
        r = dict(zip(RESIDUAL_PLANES, a))
        r.update(_lists_dict(out, self.arm_names()))
        return r

    def encode_tapped(self, img, q):
        """the whole encode with the residual tap set -> (file bytes, planes in front of Y19 .. Y27, planes behind them, the three lists)"""
        tap = _ResidualTap()
        ptr = ctypes.c_void_p.in_dll(self.lib, "nhwo_residual_tap_ptr")
        ptr.value = ctypes.addressof(tap)
        try:
            data = self.encode(img, q)
        finally:
            ptr.value = None
        return data, _planes_dict(tap.inp), _planes_dict(tap.out), _lists_dict(tap.lists)["lists"]

    def book_symbol_ok(self, v: int) -> bool:
        return bool(self.lib.nhwo_book_symbol_ok(int(v)))

    def supported(self, q: int) -> bool:
        return bool(self.lib.nhwo_quality_supported(q))

    def encode(self, img, q, trace=False):
        from .harness import parse_trace
        img = np.ascontiguousarray(img, np.uint8)
        n = ctypes.c_size_t(0)
        tr = None
        tbuf = None
        if trace:
            tbuf = ctypes.create_string_buffer(96 << 20)
            tr = _Trace(ctypes.cast(tbuf, P), len(tbuf), 0, 0)
        rc = self.lib.nhwo_encode(img.ctypes.data, q, ctypes.cast(self._out, P), len(self._out), ctypes.byref(n), ctypes.byref(tr) if trace else None)
        if rc != 0:
            raise RuntimeError(f"oracle encode failed rc={rc}")
        data = self._out.raw[: n.value]
        if trace:
            return data, parse_trace(tbuf.raw[: tr.len], tr.count)
        return data
