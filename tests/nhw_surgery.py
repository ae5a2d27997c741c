"""Files no encoder writes, for tests/test_decode_surgery.py: a reader and writer of the .nhw layout, the prefix code and the code books in
plain Python (after parse_header / k_dec_vlc in nhwcodec_amd/csrc/nhw_dec.hip and parse_container / build_book / vlc_luma in oracle/nhwo_dec.c),
and the fixed list of case builders.  Every builder is a deterministic function of committed golden files.

    python -m tests.nhw_surgery --write      classify every case with the sanitizer build of the oracle (oracle/_asan/nhwo_dec_asan) and
                                             rewrite tests/golden/dec/surgery.json
"""
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "dec")
RECORD = os.path.join(GOLD, "surgery.json")
ASAN_DIR = os.path.join(ROOT, "oracle", "_asan")
ASAN_EXE = os.path.join(ASAN_DIR, "nhwo_dec_asan")

DQ = 65536
OUT_STRIDE = 512 << 10                       # include/nhw_hip.h: NHW_OUT_STRIDE
P16_CAP, P6_CAP, PK_WORDS, BOOK_STAGE = 65536 + 64, 131072 + 64, 98304, 2048     # nhw_dec.hip


def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


# ---------------------------------------------------------------------------------------------- the layout
def header_fields(q):
    """(name, bytes) of the header fields behind res_high and q, in file order"""
    f = [("book1_len", 2), ("book2_len", 2), ("data1", 4), ("data2", 4), ("tree_end", 2), ("exw_len", 2)]
    if q > 12: f += [("res1_len", 2)]
    if q >= 19: f += [("res3_len", 2), ("res3_bits", 2)]
    if q > 17: f += [("res4_len", 2)]
    if q > 12: f += [("res1_bits", 2)]
    if q >= 21: f += [("res5_len", 2), ("res5_bits", 2)]
    if q > 21: f += [("res6_len", 4), ("res6_bits", 2), ("char_res1_len", 2)]
    if q > 22: f += [("qs3_len", 2)]
    f += [("select1", 2), ("select2", 2)]
    if q > 15: f += [("ll_word_len", 2)]
    f += [("ch_res_len", 2)]
    return f


def sections(q):
    """(section, header field that counts it or None, bytes per count) in file order"""
    s = [("book1", "book1_len", 1), ("book2", "book2_len", 1), ("exw", "exw_len", 1)]
    if q > 12: s += [("res1", "res1_len", 1), ("res1_bit", "res1_bits", 1), ("res1_word", "res1_bits", 1)]
    if q > 17: s += [("res4", "res4_len", 1)]
    if q >= 19: s += [("res3", "res3_len", 1), ("res3_bit", "res3_bits", 1), ("res3_word", "res3_bits", 2)]
    if q >= 21: s += [("res5", "res5_len", 1), ("res5_bit", "res5_bits", 1), ("res5_word", "res5_bits", 1)]
    if q > 21: s += [("res6", "res6_len", 1), ("res6_bit", "res6_bits", 1), ("res6_word", "res6_bits", 1), ("char", "char_res1_len", 2)]
    if q > 22: s += [("qs3", "qs3_len", 4)]
    s += [("sel1", "select1", 1), ("sel2", "select2", 1)]
    if q > 15: s += [("u64", None, 512), ("v64", None, 512), ("llword", "ll_word_len", 1)]
    s += [("chres", "ch_res_len", 1), ("packet1", "data1", 4), ("packet2", None, 4)]
    return s


class NhwFile:
    """res_high, q, h: the other header fields as stored, s: section name -> bytes, tail: what lies behind packet2"""

    def __init__(self, res_high, q, h, s, tail=b""):
        self.res_high, self.q, self.h, self.s, self.tail = res_high, q, dict(h), dict(s), tail

    def copy(self):
        return NhwFile(self.res_high, self.q, self.h, self.s, self.tail)


def read(data):
    res_high, q = data[0], data[1]
    at, h, s = 2, {}, {}
    for name, n in header_fields(q):
        h[name] = int.from_bytes(data[at:at + n], "little")
        at += n
    for name, field, unit in sections(q):
        n = unit if field is None else h[field] * unit
        if name == "packet2":
            n = (h["data2"] - h["data1"]) * 4
        assert at + n <= len(data), f"section {name} does not fit"
        s[name] = data[at:at + n]
        at += n
    return NhwFile(res_high, q, h, s, data[at:])


def write(f, **explicit):
    """the file's bytes; header lengths recomputed from the sections, except the fields named in `explicit` (res_high and q among them)"""
    h = dict(f.h)
    for name, field, unit in sections(f.q):
        if field is not None and not name.endswith("_word"):      # (a word string is counted by its bit string's field)
            h[field] = len(f.s[name]) // unit
    h["data2"] = h["data1"] + len(f.s["packet2"]) // 4
    res_high, q = explicit.pop("res_high", f.res_high), explicit.pop("q", f.q)
    h.update(explicit)
    out = bytearray([res_high & 255, q & 255])
    for name, n in header_fields(f.q):
        out += (h[name] & ((1 << (8 * n)) - 1)).to_bytes(n, "little")
    for name, _, _ in sections(f.q):
        out += f.s[name]
    return bytes(out + f.tail)


def section_ends(f):
    """byte offset of the end of the header and of every section, by name, as write(f) lays them out"""
    at = 2 + sum(n for _, n in header_fields(f.q))
    ends = {"header": at}
    for name, _, _ in sections(f.q):
        at += len(f.s[name])
        ends[name] = at
    return ends


# ---------------------------------------------------------------------------------------------- the prefix code and the books
RUNS = [(0x0000, 2, 1), (0x0002, 3, 1), (0x0004, 3, 1), (0x000a, 4, 2), (0x0006, 4, 2), (0x0018, 5, 3), (0x0036, 6, 2), (0x0070, 7, 2),
        (0x00e8, 8, 12), (0x01c8, 9, 8), (0x01e8, 9, 8), (0x03e8, 10, 8), (0x03e4, 10, 4), (0x07c0, 11, 2), (0x07e0, 11, 2),
        (0x07f0, 11, 16), (0x07e8, 11, 8), (0x0f88, 12, 8), (0x0fc8, 12, 8), (0x1f08, 13, 4), (0x3f10, 14, 8),
        (0x1f0c0, 17, 64), (0x1f8c0, 17, 46), (0x3f1dc, 18, 12), (0x7e3d0, 19, 38), (0xfc7ec, 20, 20)]


def rank_of(look20):
    """(rank, length) of the code word that heads 20 bits, (-1, 0) if none does"""
    rank = 0
    for first, ln, count in RUNS:
        v = look20 >> (20 - ln)
        if first <= v < first + count:
            return rank + v - first, ln
        rank += count
    return -1, 0


def word_of(code_rank):
    """(value, length) of the code word of a rank of the code (0 .. 289)"""
    for first, ln, count in RUNS:
        if code_rank < count:
            return first + code_rank, ln
        code_rank -= count
    raise ValueError("no such rank")


def book_word(zoned, index):
    """(value, length) of the bits that select book entry `index` of a luma stream"""
    if not zoned or index < 110:
        return word_of(index)
    if index < 174:
        return (1 << 6) | (index - 110), 15
    return word_of(index - 64)


def unpack_book(raw, chroma, tree_end=0):
    """oracle build_book: packed bytes -> list of (symbol, run length)"""
    rep = 128 if chroma else 3
    flat = expanded_book(raw, rep)[:1000]
    e = min(tree_end if chroma else len(flat), 708)
    flat += [0] * 1024
    inter = [0] * 1024
    j = 0
    for i in range(0, e, 2):
        inter[i] = flat[j]; j += 1
    for i in range(1, e, 2):
        inter[i] = flat[j]; j += 1
    book, i = [], 0
    while i < e:
        b = inter[i]
        if not chroma:
            if b == 3: book.append((128, inter[i + 1])); i += 1
            else: book.append((b, 1))
        else:
            if not b & 1: book.append((b, inter[i + 1])); i += 1
            else: book.append((b & 0xfe, 1))
        i += 1
    return book


def pack_book(inter, rep):
    """the entry bytes of a book (what unpack_book walks) -> packed bytes: even positions, then odd ones, every `rep` byte as a marker + count"""
    flat = list(inter[0::2]) + list(inter[1::2])
    raw, i = bytearray(), 0
    while i < len(flat):
        if flat[i] == rep:
            n = 1
            while i + n < len(flat) and flat[i + n] == rep and n < 255:
                n += 1
            raw += bytes([rep, n])
            i += n
        else:
            raw.append(flat[i])
            i += 1
    return bytes(raw)


def expanded_book(raw, rep):
    """the bytes a packed book expands to (flat order)"""
    flat, i = [], 0
    while i < len(raw):
        if raw[i] == rep:
            flat += [rep] * (raw[i + 1] if i + 1 < len(raw) else 0)
            i += 2
        else:
            flat.append(raw[i])
            i += 1
    return flat


def book_entry_bytes(raw, rep):
    """the entry bytes of a luma book, in entry order (the inverse of pack_book for an expansion of at most 708 bytes)"""
    flat = expanded_book(raw, rep)
    e = len(flat)
    assert e <= 708
    inter = [0] * e
    inter[0::2] = flat[:(e + 1) // 2]
    inter[1::2] = flat[(e + 1) // 2:]
    return inter


class Bits:
    """a packet as the decoder reads it: little-endian 32-bit words, most significant bit first; zero bits behind the end"""

    def __init__(self, packet):
        self.n = 8 * len(packet)
        self.big = int.from_bytes(np.frombuffer(packet, "<u4").astype(">u4").tobytes() + bytes(16), "big")
        self.total = self.n + 128

    def peek(self, at, n):
        return (self.big >> (self.total - at - n)) & ((1 << n) - 1) if at + n <= self.total else 0


def bits_to_words(bitstring):
    """a string of '0' / '1' -> packet bytes, padded with zero bits to whole words"""
    bitstring += "0" * (-len(bitstring) % 32)
    be = int(bitstring, 2).to_bytes(len(bitstring) // 8, "big") if bitstring else b""
    return np.frombuffer(be, ">u4").astype("<u4").tobytes()


def packet_bits(packet, nbits):
    b = Bits(packet)
    return format(b.peek(0, nbits), f"0{nbits}b") if nbits else ""


def luma_walk(f, upto=None):
    """oracle vlc_luma in Python -> (symbols, e, status): symbols = a list of (start bit, book index, cell before, word); status 0 or -1.
    upto: stop in front of the first symbol at or behind that bit (status 1): where an unfinished stream stands"""
    book = unpack_book(f.s["book1"], False) + [(0, 0)] * 720
    bits = Bits(f.s["packet1"])
    nwords = len(f.s["packet1"]) // 4
    zoned = f.res_high < 4
    limit = 4 * DQ - 1
    out = np.zeros(4 * DQ + 1024, np.int16)
    sel1, sel2 = f.s["sel1"], f.s["sel2"]
    bit_of = lambda s, k: (s[k >> 3] >> (7 - (k & 7))) & 1 if (k >> 3) < len(s) else 0
    z = lambda i: i < 0 or out[i] == 0
    e = mem = mem2 = ac1 = t = t2 = 0
    run_over = -257
    at, syms = 0, []
    while e < limit:
        if upto is not None and at >= upto:
            return syms, e, 1
        if at >= (nwords + 2) * 32:
            return syms, e, -1
        start = at
        if zoned and bits.peek(at, 9) == 1:
            rank = 110 + bits.peek(at + 9, 6); at += 15
        else:
            rank, ln = rank_of(bits.peek(at, 20))
            if rank < 0:
                return syms, e, -1
            at += ln
            if zoned and rank >= 110:
                rank += 64
        word, rle = book[rank]
        syms.append((start, rank, e, word))
        if word == 128:
            put = neg = 0
            mem += 1
            if mem2 == 1:
                if (e >= 5 and z(e - 2) and z(e - 3) and z(e - 4) and z(e - 5)) or (rle >= 4 and z(e - 2)):
                    put = 1; neg = not bit_of(sel2, t2); t2 += 1
                mem2 = 0
            else:
                room = rle >= 4 and e > 0 and z(e - 1) and not ac1 and (e + rle - 257) >= run_over
                if mem == 2 and not ac1:
                    if (e >= 4 and z(e - 1) and z(e - 2) and z(e - 3) and z(e - 4) and (e + rle - 257) >= run_over) or room:
                        put = 1; neg = bit_of(sel1, t); t += 1; mem = 1
                elif room:
                    put = 1; neg = bit_of(sel1, t); t += 1; mem = 1
            if put:
                out[e] = -11 if neg else 11; e += 1
            if rle == 254:
                ac1 = 1; mem = 0; run_over = e
            else:
                ac1 = 0
            e += rle
        else:
            mem = mem2 = ac1 = 0
            if word in (136, 120):
                out[e] = 11; e += 1; mem2 = 1
            elif 132 <= word <= 135:
                out[e] = 11; e += 4; out[e] = 11; e += 1
            else:
                out[e] = 1; e += 1          # (only whether a cell is zero matters to the walk; no level of the code is zero)
    return syms, e, 0


# ---------------------------------------------------------------------------------------------- the cases
# Group A: well-formed by the oracle's rules, never written by an encoder.  Group B: damaged; the oracle decides which are refused.
# A case is (name, group, bytes, gpu_cap): gpu_cap names the cap of the GPU decoder that refuses a file the oracle
# takes, None for every other case.
def _pad_book(raw, rep, target, where):
    """a packed book brought to `target` bytes with marker + count-0 pairs, which expand to nothing; an odd difference leaves a lone marker
    as the book's last byte (its count reads as 0).  where: 'front', 'behind', or 'edge': a marker of the book itself at index BOOK_STAGE - 1"""
    need = target - len(raw)
    assert need >= 0
    pairs, lone = bytes([rep, 0]) * (need // 2), bytes([rep]) * (need % 2)
    if where == "front":
        return pairs + raw + lone
    if where == "behind":
        return raw + pairs + lone
    marks, i = [], 0                                              # the book's own markers with a count above 0
    while i < len(raw):
        if raw[i] == rep:
            if i + 1 < len(raw) and raw[i + 1]:
                marks.append(i)
            i += 2
        else:
            i += 1
    m = next(m for m in marks if (BOOK_STAGE - 1 - m) % 2 == 0 and BOOK_STAGE - 1 - m <= len(pairs))
    front = BOOK_STAGE - 1 - m
    out = pairs[:front] + raw + pairs[front:] + lone
    assert out[BOOK_STAGE - 1] == rep and out[BOOK_STAGE] == raw[m + 1] and len(out) == target
    return out


def _with(f, **sections_):
    g = f.copy()
    g.s.update(sections_)
    return g


def _last_cell_tails(f):
    """packet1 rewritten behind a late symbol so that the last symbol the walk takes is a 132..135 word that starts at cell 4 DQ - 5 .. 4 DQ - 2:
    runs up to 13 cells before the end, then plain literals (a cell each, never with a value put in front), then the word"""
    book = unpack_book(f.s["book1"], False)
    zoned = f.res_high < 4
    syms, _, st = luma_walk(f)
    assert st == 0
    fives = [i for i, (w, _) in enumerate(book) if 132 <= w <= 135]
    plain = next(i for i, (w, r) in enumerate(book) if w != 128 and not 120 <= w <= 136)
    runs = sorted(((r, i) for i, (w, r) in enumerate(book) if w == 128 and r != 254), reverse=True)
    enc = lambda i: format(book_word(zoned, i)[0], f"0{book_word(zoned, i)[1]}b")
    keep = max(k for k, s in enumerate(syms) if s[2] <= 4 * DQ - 600)
    bits = packet_bits(f.s["packet1"], syms[keep][0])
    stop = 4 * DQ - 13
    for _ in range(64):                                             # the walk says where a candidate stands: a run may bring a value with it
        e = luma_walk(_with(f, packet1=bits_to_words(bits)), len(bits))[1]
        if e >= stop - 8:
            break
        bits += enc(next(i for r, i in runs if r <= stop - 8 - e or r == runs[-1][0]))
    out = []
    for k, five in enumerate(fives[:4]):
        start = 4 * DQ - 5 + k
        e, b = luma_walk(_with(f, packet1=bits_to_words(bits)), len(bits))[1], bits
        assert e <= start
        b += enc(plain) * (start - e) + enc(five)
        g = _with(f, packet1=bits_to_words(b))
        s2, e2, st2 = luma_walk(g)
        assert st2 == 0 and s2[-1][2] == start and s2[-1][1] == five and e2 == start + 5, (start, s2[-3:], e2, st2)
        out.append((f"last_cell_{4 * DQ - start}_word{book[five][0]}", g))
    return out


def _cases():
    q20, q10, q23, q01 = (read(golden(n)) for n in ("q20_0.nhw", "q10_0.nhw", "q23_0.nhw", "q01_0.nhw"))
    A, B = [], []
    a = lambda name, f, **kw: A.append((name, write(f, **kw) if isinstance(f, NhwFile) else f, None))
    b = lambda name, f, cap=None, **kw: B.append((name, write(f, **kw) if isinstance(f, NhwFile) else f, cap))

    # ---- A: long books
    for tag, base, sec, rep in (("book1", q20, "book1", 3), ("book2", q10, "book2", 128)):
        for target in (2046, 2047, 2048, 2049, 2050, 4001):
            for where in ("front", "behind"):
                a(f"long_{tag}_{target}_{where}", _with(base, **{sec: _pad_book(base.s[sec], rep, target, where)}))
        for target in (2300, 4001):                                  # (far enough over BOOK_STAGE that padding lies on both sides of the book)
            a(f"long_{tag}_{target}_edge", _with(base, **{sec: _pad_book(base.s[sec], rep, target, "edge")}))
        a(f"{tag}_ends_on_marker", _with(base, **{sec: base.s[sec] + bytes([rep])}))
    a("long_book1_q23_3000_edge", _with(q23, book1=_pad_book(q23.s["book1"], 3, 3000, "edge")))
    a("long_book2_q23_2051_front", _with(q23, book2=_pad_book(q23.s["book2"], 128, 2051, "front")))

    # ---- book caps.  An expansion is cut at 708 bytes BEFORE its even and odd halves are put together again, so a book that is longer
    # than that only reads as its writer meant if the first 708 bytes are the two halves of a 708-byte book: those are group A (what lies
    # behind is dropped); the others read as another book, and the oracle says what becomes of the file (group B)
    inter1 = book_entry_bytes(q20.s["book1"], 3)
    lit1 = lambda n: [131 + ((i % 97) | 1) for i in range(n)]                     # one-byte entries, none of them the marker
    full1 = pack_book(inter1 + lit1(708 - len(inter1)), 3)                        # more than 354 entries
    assert len(expanded_book(full1, 3)) == 708 and len(inter1) < 700
    a("book1_expands_to_707", _with(q20, book1=pack_book(inter1 + lit1(707 - len(inter1)), 3)))
    a("book1_expands_to_708", _with(q20, book1=full1))
    a("book1_708_and_1_dropped", _with(q20, book1=full1 + bytes([201])))
    a("book1_708_and_52_dropped", _with(q20, book1=full1 + bytes(200 + (i % 50) for i in range(52))))
    a("book1_708_and_marker_run_dropped", _with(q20, book1=full1 + bytes([3, 20])))
    a("book1_708_and_1000_and_beyond", _with(q20, book1=full1 + bytes([3, 255]) * 3 + bytes(200 + (i % 50) for i in range(300))))
    for total in (709, 800):
        b(f"book1_expands_to_{total}", _with(q20, book1=pack_book(inter1 + lit1(total - len(inter1)), 3)))
    flat1 = expanded_book(q20.s["book1"], 3)
    b("book1_marker_run_crosses_708", _with(q20, book1=q20.s["book1"] + bytes(200 + (i % 50) for i in range(700 - len(flat1))) + bytes([3, 20])))
    exp2 = len(expanded_book(q20.s["book2"], 128))
    assert exp2 == q20.h["tree_end"]
    inter2 = book_entry_bytes(q20.s["book2"], 128)
    lit2 = lambda n: [1 + 2 * (i % 100) for i in range(n)]                        # odd bytes: one-byte entries
    full2 = pack_book(inter2 + lit2(708 - exp2), 128)
    a("book2_expands_to_708", _with(q20, book2=full2), tree_end=708)
    for te in (708, 709, 720, 65535):
        a(f"book2_708_and_12_dropped_tree_end_{te}", _with(q20, book2=full2 + bytes(lit2(12))), tree_end=te)
    a("book2_708_and_marker_run_dropped", _with(q20, book2=full2 + bytes([128, 30])), tree_end=738)
    a("book2_dropped_behind_tree_end", _with(q20, book2=q20.s["book2"] + bytes(lit2(720 - exp2))), tree_end=exp2)
    for te in (0, 1, exp2 - 1, exp2 + 1, exp2 + 2, 708, 709, 65535):
        b(f"book2_tree_end_{te}", q20, tree_end=te)
    b("book2_expands_to_709", _with(q20, book2=pack_book(inter2 + lit2(709 - exp2), 128)), tree_end=709)

    # ---- A: trailing slack
    for n in (1, 3, 4096):
        g = q20.copy(); g.tail = bytes(0xEE for _ in range(n))
        a(f"slack_{n}", g)

    # ---- A: empty and short side strings
    for tag, base in (("q20", q20), ("q10", q10), ("q23", q23)):
        a(f"{tag}_select1_0", _with(base, sel1=b""))
        a(f"{tag}_select2_0", _with(base, sel2=b""))
        a(f"{tag}_exw_0", _with(base, exw=b""))
    a("q01_select1_0", _with(q01, sel1=b""))
    a("q01_select2_0", _with(q01, sel2=b""))
    a("q01_exw_0", _with(q01, exw=b""))
    g = q01.copy(); g.tail = bytes([0xEE]) * 3
    a("q01_slack_3", g)
    a("q01_book1_ends_on_marker", _with(q01, book1=q01.s["book1"] + bytes([3])))
    a("long_book1_q01_2049_behind", _with(q01, book1=_pad_book(q01.s["book1"], 3, 2049, "behind")))
    a("long_book2_q01_2300_front", _with(q01, book2=_pad_book(q01.s["book2"], 128, 2300, "front")))
    a("q20_select1_half", _with(q20, sel1=q20.s["sel1"][:len(q20.s["sel1"]) // 2]))
    for tag, base in (("q20", q20), ("q23", q23)):
        a(f"{tag}_ll_word_0", _with(base, llword=b""))
        a(f"{tag}_ll_word_half", _with(base, llword=base.s["llword"][:len(base.s["llword"]) // 2]))
    a("q20_res1_len_0", _with(q20, res1=b""))
    a("q20_res3_len_0", _with(q20, res3=b""))
    for k in (1, 3, 5, 6):
        a(f"q23_res{k}_len_0", _with(q23, **{f"res{k}": b""}))

    # ---- A: lists at the cap: a column byte, then step bytes of no step, two entries each, more of them than the bit string has room for
    for k, nbytes, steps in ((1, (P16_CAP - 64) // 8, 65534), (3, (P16_CAP - 64) // 8, 65534), (5, (P16_CAP - 64) // 8, 65534), (6, (P6_CAP - 64) // 8, 70000)):
        word = bytes(4) + bytes([0xAA]) * (nbytes * (2 if k == 3 else 1) - 4)          # signs that nearly cancel: no cell leaves the 16-bit range for good
        g = _with(q23, **{f"res{k}": bytes([5]) + bytes([0x80]) * steps, f"res{k}_bit": bytes(nbytes), f"res{k}_word": word})
        assert 1 + 2 * steps > nbytes * 8
        a(f"q23_res{k}_at_cap", g)
        over = _with(g, **{f"res{k}_bit": bytes(nbytes + 1), f"res{k}_word": word + bytes([0xAA]) * (2 if k == 3 else 1)})
        b(f"q23_res{k}_bits_over_cap", over, cap="P6_CAP" if k == 6 else "P16_CAP")

    # ---- A: the last cells
    for name, g in _last_cell_tails(q20):
        a(name, g)

    # ---- B: header lengths one more than fits, sections cut one byte short
    for field, _ in header_fields(23):
        if field == "tree_end":
            continue
        kw = {field: write_fields(q23)[field] + 1}
        if field == "data1":
            kw["data2"] = q23.h["data2"] + 1
        b(f"q23_{field}_plus_1", q23, **kw)
    whole = write(q23)
    for sec, end in section_ends(q23).items():
        b(f"q23_cut_in_{sec}", whole[:end - 1])
    whole = write(q01)
    for sec, end in section_ends(q01).items():
        b(f"q01_cut_in_{sec}", whole[:end - 1])
    for field, _ in header_fields(1):
        if field not in ("tree_end", "data1"):
            b(f"q01_{field}_plus_1", q01, **{field: write_fields(q01)[field] + 1})
    b("q01_ch_res_half", _with(q01, chres=q01.s["chres"][:len(q01.s["chres"]) // 2]))      # the low-quality LL2 coder runs off its bytes: they read 0
    b("q10_ch_res_half", _with(q10, chres=q10.s["chres"][:len(q10.s["chres"]) // 2]))
    b("res_high_7", q20, res_high=7)
    b("q_0", q20, q=0)
    b("q_24", q20, q=24)
    b("data2_below_data1", q20, data2=q20.h["data1"] - 1)
    b("data1_negative", q20, data1=0xFFFFFFFF, data2=0xFFFFFFFF)
    for total, cap in ((PK_WORDS - 8, None), (PK_WORDS - 7, "PK_WORDS")):
        grow = total - q20.h["data2"]
        b(f"data2_{total}", _with(q20, packet1=q20.s["packet1"] + bytes(4 * grow)), cap=cap)

    # ---- B: packets that end early
    for tag, base in (("q20", q20), ("q10", q10), ("q01", q01)):
        for sec in ("packet1", "packet2"):
            for drop in (1, 3, 8, 9, 64, 200):
                n = len(base.s[sec]) // 4
                if drop <= n:
                    b(f"{tag}_{sec}_minus_{drop}", _with(base, **{sec: base.s[sec][:4 * (n - drop)]}))
            b(f"{tag}_{sec}_emptied", _with(base, **{sec: b""}))         # (stands for the drops of more words than a short packet has)
    # ---- B: a damaged word in the stream.  No pattern is "no code word" (the code is complete: test_prefix_code_is_complete), so the words
    # written are the code's longest and rarest ones, twenty 1 bits and 0xfc7ec: the walk loses step there and finds it again, or does not
    for tag, base in (("q20", q20), ("q10", q10), ("q01", q01)):
        for pname, pat in (("ones", 0xFFFFF), ("fc7ec", 0xFC7EC)):
            word = ((pat << 12) | 0xFFF if pname == "ones" else pat << 12).to_bytes(4, "little")
            n1, n2 = len(base.s["packet1"]) // 4, len(base.s["packet2"]) // 4
            for sec, at, where in (("packet1", 0, "first"), ("packet1", n1 // 2, "middle"), ("packet2", n2 // 2, "middle")):
                if tag != "q20" and (where == "first" or pname == "fc7ec"):
                    continue
                pk = base.s[sec]
                b(f"{tag}_{sec}_{where}_word_{pname}", _with(base, **{sec: pk[:4 * at] + word + pk[4 * at + 4:]}))
    # rank 0 a run of 254, the stream cut in half: what decodes from the zero bits behind a stream's end
    lit = [3, 254] + [141 + 2 * (i % 50) for i in range(706)]
    half = q20.s["packet1"][:4 * (len(q20.s["packet1"]) // 8)]
    b("book1_rank0_254_half_stream", _with(q20, book1=pack_book(lit, 3), packet1=half))
    b("book1_rank0_254_whole_stream", _with(q20, book1=pack_book(lit, 3)))
    b("book1_rank0_254_no_stream", _with(q20, book1=pack_book(lit, 3), packet1=b""))
    return A, B


def write_fields(f):
    """the header fields as write(f) stores them"""
    return read(write(f)).h


_CACHE = []


def cases():
    """[(name, group, bytes, gpu_cap)], a fixed list in a fixed order"""
    if not _CACHE:
        A, B = _cases()
        out = [(n, "A", d, c) for n, d, c in A] + [(n, "B", d, c) for n, d, c in B]
        assert len({n for n, *_ in out}) == len(out)
        assert len({d for _, _, d, _ in out}) == len(out), "two cases are the same file"
        assert all(len(d) < OUT_STRIDE for _, _, d, _ in out)
        _CACHE.extend(out)
    return list(_CACHE)


# ---------------------------------------------------------------------------------------------- classification
def can_sanitize():
    """whether this machine's compiler can link and run a sanitized program at all: a one-line program says so"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "probe.c")
        with open(src, "w") as fp:
            fp.write("int main(void) { return 0; }\n")
        try:
            probe = subprocess.run(["gcc", "-fsanitize=address,undefined", "-o", os.path.join(tmp, "probe"), src], capture_output=True)
            can = probe.returncode == 0 and subprocess.run([os.path.join(tmp, "probe")], capture_output=True).returncode == 0
        except OSError:
            can = False
    return can


def build_asan():
    """the sanitizer build of the oracle's decoder; None where can_sanitize() says no; any other failure of the build is an error"""
    if not can_sanitize():
        return None
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"], capture_output=True, text=True)
    if p.returncode != 0 or not os.path.exists(ASAN_EXE):
        raise RuntimeError("make -C oracle asan failed:\n" + p.stderr[-2000:])
    return ASAN_EXE


def classify_one(exe, data, tmpdir, key):
    """-> ('defined', quality, pixels) / ('refused', None, None) / ('undefined', None, report)"""
    path = os.path.join(tmpdir, f"{key}.nhw")
    with open(path, "wb") as fp:
        fp.write(data)
    p = subprocess.run([exe, path], capture_output=True, timeout=120)
    os.unlink(path)
    if p.returncode == 0 and len(p.stdout) == 1 + 786432 and not p.stderr:
        return "defined", p.stdout[0], p.stdout[1:]
    if p.returncode == 3 and not p.stderr:
        return "refused", None, None
    return "undefined", None, p.stderr.decode(errors="replace")[:400]


def classify_all(exe, tmpdir, workers=8):
    cs = cases()
    with ThreadPoolExecutor(max_workers=workers) as ex:
        res = list(ex.map(lambda kc: classify_one(exe, kc[1][2], tmpdir, kc[0]), enumerate(cs)))
    return cs, res


NEIGHBOURS = ("q20_0.nhw", "q10_0.nhw", "q23_0.nhw", "q01_0.nhw", "q16_0.nhw")      # the golden files the GPU batches put between the cases


def load_record():
    """(cases: name -> record, neighbours: golden name -> the digests of its scaled pictures)"""
    with open(RECORD) as f:
        rec = json.load(f)
    return rec["cases"], rec["neighbours"]


def ll_verbatim_tokens(f):
    """how many verbatim tokens (a byte from 128 on) the luma part of the LL2 walk takes: each of them takes a byte of ll_word when q > 15"""
    code, mode, fine = f.s["chres"], f.res_high & 3, f.q > 15
    i, j, n = 1, 1, 0
    while j < DQ // 4:
        c = code[i] if i < len(code) else 0
        if c >= 128:
            n += 1; j += 2 if fine else 1
        elif c >= 64 and mode != 2 or mode == 2 and c >= 64:
            i += 1; j += 3
        elif mode in (0, 3):
            j += (((c >> 3) & 1) + 2 + (0, 1, 2, 2, 2, 2, 1, 1)[c & 7]) if c < 16 else 2
        elif mode == 1:
            j += (((c >> 2) & 7) + 2 + (1 if c & 3 else 0)) if c < 32 else 2
        else:
            j += (c & 63) + 2
        i += 1
    return n


def main():
    import tempfile
    from tests.conftest import ROOT as _  # noqa: F401  (the repository root on sys.path)
    from oracle.oraclepy import Oracle
    from tests.tensor_cases import expected
    exe = build_asan()
    assert exe, "no sanitizer build"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    oracle = Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
    sha = lambda x: hashlib.sha256(x).hexdigest()
    with tempfile.TemporaryDirectory() as tmp:
        cs, res = classify_all(exe, tmp)
    rec = {}
    for (name, group, data, cap), (cls, q, px) in zip(cs, res):
        r = {"group": group, "class": cls, "nhw_sha256": sha(data), "bytes": len(data)}
        if cap:
            r["gpu_cap"] = cap
        if cls == "defined":
            r["quality"] = q
            r["pixels_sha256"] = sha(px)
            got, gq = oracle.decode(data)
            assert gq == q and got.tobytes() == px, name
            for s in (2, 4):
                r[f"scale{s}_sha256"] = sha(expected(oracle, data, s).tobytes())
        if cls == "undefined":
            print(name, px)
        rec[name] = r
    nb = {g: {f"scale{s}_sha256": sha(expected(oracle, golden(g), s).tobytes()) for s in (2, 4)} for g in NEIGHBOURS}
    with open(RECORD, "w") as f:
        json.dump({"cases": rec, "neighbours": nb}, f, indent=1, sort_keys=True)
        f.write("\n")
    n = {c: sum(1 for r in rec.values() if r["class"] == c) for c in ("defined", "refused", "undefined")}
    print(len(rec), "cases", n)
    for name, r in rec.items():
        print(f"{r['group']} {r['class']:9s} {r.get('gpu_cap', ''):8s} {name}")


if __name__ == "__main__":
    main()
