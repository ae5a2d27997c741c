"""Well-formed files whose VALUES are extreme, for tests/test_decode_values.py (DESIGN.md section 7.1b has the bounds): whole .nhw files built on
the CPU from crafted content -- the two symbol streams, the LL2 section, the exception triples, the q > 21 corrections -- on the header of a golden
file of the same quality, next to tests/nhw_surgery.py, whose reader / writer, prefix code and code-book packer they use.  A second source is the
oracle's own encoder on adversarial pictures (what a real encoder emits at its worst).  Every builder is deterministic.

The streams are written here and not by the encoder's packetiser (Oracle.stream_stage): that one rewrites the symbols it is given (the folds of
+-8 into runs, the pattern symbols) and refuses levels no quantiser emits, which are the ones wanted.  The writer uses only what the walk of
oracle/nhwo_dec.c:vlc_luma cannot answer with a value of its own: a zero gap is a chain of 254-runs and at most one shorter run, which never
meets the conditions under which a run brings a +-11 with it (after a 254-run `ac1` is set, after a literal the cell before is not zero), and
the words 120, 132 .. 136 are never written.  Both selection strings are therefore empty.

    python -m tests.nhw_values --write       classify every case with the sanitizer build of the oracle and rewrite tests/golden/dec/values.json
"""
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import nhw_surgery as S

RECORD = os.path.join(S.GOLD, "values.json")
QUALITIES = (10, 16, 17, 20, 23)
BASE = {q: f"q{q:02d}_0.nhw" for q in QUALITIES}
NEIGHBOURS = ("q20_0.nhw", "q10_0.nhw")                      # the golden files the GPU batches put between the cases
DQ = S.DQ

# ---------------------------------------------------------------------------------------------- the bounds
LEVEL_MAX, LEVEL_MIN = 275, -275            # plain_level: the escape words, +-(123 + 8 * 19)
LUMA_TAG_MAX = 1011                         # a pattern symbol the passes of :493-616 leave standing (1010 / 1011 in rows 256 .. 511)
CHROMA_TAG_MAX = 5006                       # a correction symbol in the level-2 bands of a chroma plane, which no pass takes out
EX_MAX, EX_MIN = 510, -255                  # an exception sample: 255 + byte, -byte
LL_MAX, LL_MIN = 255, 0                     # an LL2 sample of the luma (a byte); chroma: the byte + 1 up to q15


def plain_level(word):
    """oracle plain_level / extra_level"""
    x = 0
    if word < 110 and 10 <= word <= 108 and (word & 7) in (2, 4, 6):
        n = ((word >> 3) - 1) * 3 + ((word & 7) >> 1)
        x = n if n <= 19 else -(n - 19)
    if x > 0:
        return 123 + (x << 3)
    if x < 0:
        return (x << 3) - 123
    return word - 125 if word > 128 else word - 131


def _alphabets():
    """value -> the word that carries it, luma and chroma: the smallest word of each value; never 3 (luma: the book's repeat marker), 128 (a run),
    nor the words whose walk state the writer stays clear of"""
    luma, chroma = {}, {}
    special = {127: 1008, 129: 1009, 125: 1006, 126: 1007, 121: 1010, 122: 1011, 124: 11, 123: -11}
    for w in range(256):
        if w in (3, 128, 120, 132, 133, 134, 135, 136):
            continue
        luma.setdefault(special.get(w, plain_level(w)), w)
    cspecial = {124: 5005, 126: 5006, 122: 5003, 130: 5004}
    for w in range(0, 256, 2):
        if w != 128:
            chroma.setdefault(cspecial.get(w, plain_level(w)), w)
    return luma, chroma


LUMA_WORD, CHROMA_WORD = _alphabets()
assert max(v for v in LUMA_WORD if v < 1000) == LEVEL_MAX and min(LUMA_WORD) == LEVEL_MIN and max(LUMA_WORD) == LUMA_TAG_MAX
assert max(v for v in CHROMA_WORD if v < 5000) == LEVEL_MAX and min(CHROMA_WORD) == LEVEL_MIN and max(CHROMA_WORD) == CHROMA_TAG_MAX


# ---------------------------------------------------------------------------------------------- streams
def luma_stream(plane):
    """int [512, 512] -> the 262144 cells in stream order: strips of 4 columns, two rows a step, the second one backwards (nhwo_dec.c:487)"""
    a = np.asarray(plane).reshape(256, 2, 128, 4)
    s = np.empty((128, 256, 8), np.int64)
    s[:, :, :4] = a[:, 0].transpose(1, 0, 2)
    s[:, :, 4:] = a[:, 1, :, ::-1].transpose(1, 0, 2)
    return s.reshape(-1)


def chroma_stream(u, v):
    """two int [256, 256] -> the 131072 cells in stream order: strips of 8 columns, U on even and V on odd positions (nhwo_dec.c:686)"""
    out = np.empty((65536, 2), np.int64)
    for c, p in enumerate((u, v)):
        a = np.asarray(p).reshape(128, 2, 32, 8)
        s = np.empty((32, 128, 16), np.int64)
        s[:, :, :8] = a[:, 0].transpose(1, 0, 2)
        s[:, :, 8:] = a[:, 1, :, ::-1].transpose(1, 0, 2)
        out[:, c] = s.reshape(-1)
    return out.reshape(-1)


def _run_tokens(gap):
    return [256 + 254] * (gap // 254) + ([256 + gap % 254] if gap % 254 else [])


def pack_stream(cells, limit, words, chroma, zoned):
    """cells in stream order, of which the walk takes those in front of `limit` -> (packed code book, packet bytes, bytes the book expands to).
    A token is a literal word or a run (256 + length); the most frequent token gets the shortest code word."""
    cells = np.asarray(cells)[:limit]
    nz = np.flatnonzero(cells)
    lut = np.full(int(max(words)) - int(min(words)) + 1, -1, np.int64)
    for val, w in words.items():
        lut[val - min(words)] = w
    lit = lut[cells[nz] - min(words)]
    assert (lit >= 0).all(), "a value no word carries"
    gaps = np.diff(np.concatenate(([-1], nz))) - 1
    chunks, last = [], 0
    for t in np.flatnonzero(gaps):
        chunks += [lit[last:t], np.array(_run_tokens(int(gaps[t])), np.int64)]
        last = t
    chunks.append(lit[last:])
    end = int(nz[-1]) + 1 if len(nz) else 0
    chunks.append(np.array(_run_tokens(limit - end), np.int64))
    tokens = np.concatenate(chunks).astype(np.int64)
    uniq, counts = np.unique(tokens, return_counts=True)
    order = uniq[np.argsort(-counts, kind="stable")]
    if zoned and not chroma:
        # a zoned walk (res_high < 4) reads eight 0 bits and a 1 as the head of a 15-bit word, and only rank 0's word, `00`, can make up that pattern
        # together with its neighbours (no other word ends or starts with more than six 0 bits): rank 0 goes to a run the stream does not use
        order = np.concatenate(([next(t for t in range(256 + 253, 256, -1) if t not in uniq)], order))
    assert len(order) <= (354 if zoned and not chroma else 290), "more tokens than the code has words"
    rank = np.zeros(512, np.int64)
    rank[order] = np.arange(len(order))
    inter = []
    for tok in order.tolist():
        if tok >= 256:
            inter += [128 if chroma else 3, tok - 256]
        else:
            inter.append(tok | 1 if chroma else tok)
    assert len(inter) <= 708
    code = [S.word_of(r) if chroma else S.book_word(zoned, r) for r in range(len(order))]
    val, ln = np.array([c[0] for c in code], np.int64), np.array([c[1] for c in code], np.int64)
    r = rank[tokens]
    lens, vals = ln[r], val[r]
    start = np.cumsum(lens) - lens
    total = int(lens.sum())
    bits = np.zeros(total + (-total % 32), np.uint8)
    for b in range(int(lens.max())):
        m = lens > b
        bits[start[m] + b] = (vals[m] >> (lens[m] - 1 - b)) & 1
    packet = np.packbits(bits).view(">u4").astype("<u4").tobytes()
    return S.pack_book(inter, 128 if chroma else 3), packet, len(inter)


# ---------------------------------------------------------------------------------------------- the LL2 section and the exception list
def _sdiff(a, b):
    """b - a as the byte arithmetic of ll_expand sees it, in -128 .. 127"""
    return ((int(b) - int(a) + 128) & 255) - 128


def ll_section(q, luma, u, v, verbatim=False):
    """The bytes of ch_res and ll_word that make ll_expand (nhwo_dec.c:114) give the 16384 luma and 2 x 4096 chroma samples asked for, never a
    sample more (the walks end on their last cell exactly).  Luma: differences in three-sample tokens (bytes 64 .. 127, the same in every mode
    of res_high), or `verbatim`: a token from 128 on (one even sample; with its fine byte in front when q > 15).  Chroma: two-sample difference
    tokens, runs of three, verbatim samples (multiples of 4).  -> (ch_res, ll_word)"""
    luma, fine = [int(x) for x in luma], q > 15
    assert len(luma) == DQ // 4 and len(u) == len(v) == DQ // 16
    code, word, j = [luma[0]], [], 1

    def triple(j):
        d = [_sdiff(luma[j - 1], luma[j]), _sdiff(luma[j], luma[j + 1]), _sdiff(luma[j + 1], luma[j + 2])]
        ok = all(x % 2 == 0 for x in d) and -32 <= d[0] <= 30 and -16 <= d[1] <= 14 and -32 <= d[2] <= 30
        assert ok, f"LL2 samples {j} ..: no token gives the steps {d}"
        c1, c2, c3 = (d[0] + 32) >> 1, (d[1] + 16) >> 1, (d[2] + 32) >> 1
        return [64 + ((c1 << 1) | (c2 >> 3)), ((c2 & 7) << 5) | c3]

    if verbatim:
        if fine:                                                   # 16383 samples: a triple, then 8190 pairs
            code += triple(1); j = 4
        while j < DQ // 4:
            if fine:
                word.append(luma[j]); j += 1
            assert luma[j] % 2 == 0 and luma[j] < 256, "a verbatim sample is even"
            code.append(128 + (luma[j] >> 1)); j += 1
    else:
        while j < DQ // 4:
            code += triple(j); j += 3
    assert j == DQ // 4
    ch = [int(x) for x in u] + [int(x) for x in v]
    code.append(ch[0])
    j, n = 1, len(ch)
    while j < n:
        left = n - j
        d0 = _sdiff(ch[j - 1], ch[j])
        if left % 2 == 1:                                          # an odd rest: three equal samples, or one verbatim
            if left >= 3 and ch[j] == ch[j + 1] == ch[j + 2] == ch[j - 1]:
                code.append(64 + 8); j += 3; continue
            assert ch[j] % 4 == 0, f"chroma LL2 sample {j}: no token"
            code.append(128 + (ch[j] >> 2)); j += 1; continue
        d1 = _sdiff(ch[j], ch[j + 1])
        if d0 % 4 == 0 and d1 % 4 == 0 and -16 <= d0 <= 12 and -16 <= d1 <= 12:
            code.append((((d0 + 16) >> 2) << 3) | ((d1 + 16) >> 2)); j += 2
        else:
            assert ch[j] % 4 == 0, f"chroma LL2 sample {j}: no token"
            code.append(128 + (ch[j] >> 2)); j += 1
    assert j == n
    return bytes(code), bytes(word)


def ex_bytes(luma=(), u=(), v=()):
    """the exception list: (row, column, value) triples of the luma plane (stride 512, columns 0 .. 127), two zero bytes, those of U (stride 256),
    two zero bytes, those of V to the end of the bytes.  value: 255 .. 510 or -255 .. 0"""
    def part(ts):
        out = []
        for row, col, val in ts:
            assert 0 <= row < 256 and 0 <= col < 128 and (255 <= val <= 510 or -255 <= val <= 0)
            t = [row, col + 128, val - 255] if val >= 255 else [row, col, -val]
            assert t[0] or t[1], "a triple that starts with two zero bytes ends the list"
            out += t
        return out
    return bytes(part(luma) + [0, 0] + part(u) + [0, 0] + part(v))


# ---------------------------------------------------------------------------------------------- a file
EMPTY = ("res1", "res1_bit", "res1_word", "res3", "res3_bit", "res3_word", "res4", "res5", "res5_bit", "res5_word", "res6", "res6_bit", "res6_word",
         "char", "qs3", "sel1", "sel2")


def build(q, luma, u, v, ll, llu, llv, verbatim=False, ex=None, qs3=(), char=(), u64=None, v64=None, lists=None):
    """a whole file of quality q on the header of that quality's golden: luma [512, 512], u, v [256, 256] the cells of the two streams as values (the
    LL2 quadrants are overwritten by the samples and stay 0 here), ll / llu / llv the LL2 samples, ex = (luma, u, v) exception triples, qs3: 32-bit
    words (cell << 1 | sign) and char: 16-bit words of the q > 21 corrections.  Every residual list is empty but those `lists` names (section name -> bytes)."""
    f = S.read(S.golden(BASE[q]))
    luma, u, v = np.array(luma, np.int64), np.array(u, np.int64), np.array(v, np.int64)
    assert luma.shape == (512, 512) and u.shape == v.shape == (256, 256)
    luma[:128, :128] = 0; u[:64, :64] = 0; v[:64, :64] = 0
    book1, packet1, _ = pack_stream(luma_stream(luma), 4 * DQ - 1, LUMA_WORD, False, f.res_high < 4)
    book2, packet2, tree_end = pack_stream(chroma_stream(u, v), 2 * DQ - 2, CHROMA_WORD, True, False)
    chres, llword = ll_section(q, np.asarray(ll).reshape(-1), np.asarray(llu).reshape(-1), np.asarray(llv).reshape(-1), verbatim)
    sec = {name: b"" for name in EMPTY if name in f.s}
    sec.update(book1=book1, book2=book2, packet1=packet1, packet2=packet2, chres=chres, exw=ex_bytes(*(ex or ((), (), ()))))
    if q > 15:
        sec.update(llword=llword, u64=bytes(u64) if u64 is not None else bytes(512), v64=bytes(v64) if v64 is not None else bytes(512))
    if q > 22:
        sec["qs3"] = b"".join(int(w).to_bytes(4, "little") for w in qs3)
    if q > 21:
        sec["char"] = b"".join(int(w).to_bytes(2, "little") for w in char)
    sec.update(lists or {})
    g = S._with(f, **sec)
    data = S.write(g, tree_end=tree_end)
    assert S.read(data).h["data2"] <= S.PK_WORDS - 8 and len(data) < S.OUT_STRIDE
    return data


# ---------------------------------------------------------------------------------------------- content
def _signs(kind, n):
    i, j = np.mgrid[0:n, 0:n]
    return {"plus": np.ones((n, n), np.int64), "minus": -np.ones((n, n), np.int64), "rows": 1 - 2 * (i & 1), "cols": 1 - 2 * (j & 1),
            "checker": 1 - 2 * ((i + j) & 1)}[kind]


def _flat(q, val=128):
    """LL2 samples of a flat grey picture"""
    return np.full(DQ // 4, val), np.full(DQ // 16, 128), np.full(DQ // 16, 128)


def _details(kind, level=LEVEL_MAX):
    return _signs(kind, 512) * level, _signs(kind, 256) * level, _signs(kind, 256) * level


def _ll_pattern(kind):
    """(luma, u, v) LL2 samples: all at the top, all at the bottom, or the two alternating (even values: both kinds of token can write them)"""
    if kind == "max":
        return np.full(DQ // 4, 255), np.full(DQ // 16, 255), np.full(DQ // 16, 255)
    if kind == "min":
        return np.zeros(DQ // 4, np.int64), np.zeros(DQ // 16, np.int64), np.zeros(DQ // 16, np.int64)
    i, j = np.mgrid[0:128, 0:128]
    a = np.where((i + j) & 1, 0, 254).reshape(-1)
    i, j = np.mgrid[0:64, 0:64]
    c = np.where((i + j) & 1, 0, 252).reshape(-1)
    return a, c, c[::-1].copy()


def _edge_exceptions():
    """exception samples at both extremes on the corners and edges of every band they can reach: luma rows 0 .. 255 x columns 0 .. 127 (the LL2
    quadrant and the level-2 band under it), chroma rows 0 .. 255 x columns 0 .. 127 of the 256-wide plane"""
    lu = [(0, 0, 510), (0, 1, -255), (0, 127, 510), (127, 0, -255), (127, 127, 510), (64, 0, 510), (0, 64, -255), (127, 63, -255), (63, 127, -255),
          (128, 0, 510), (128, 127, -255), (255, 0, -255), (255, 127, 510), (191, 64, 510), (60, 60, 255), (61, 61, -1)]
    ch = [(0, 0, 510), (0, 1, -255), (0, 63, 510), (63, 0, -255), (63, 63, 510), (0, 64, -255), (0, 127, 510), (63, 64, 510), (63, 127, -255),
          (64, 0, 510), (64, 127, -255), (127, 0, -255), (127, 127, 510), (128, 0, 510), (255, 127, -255), (255, 0, -255), (128, 127, 510)]
    return lu, ch, [(r, c, val if (r, c) == (0, 0) else 510 if val < 0 else -255) for r, c, val in ch]     # V: the same cells, the other extreme


def _one_sided(q):
    """the left half of the picture far below 0, the right half far above 255, in the luma and in both chroma planes: LL2 at 0 / 255 with exception
    samples of -255 / 510 in a grid and details whose signs push the same way"""
    ll = np.zeros((128, 128), np.int64); ll[64:, :] = 254                      # (the LL2 quadrant is the picture transposed: rows here are columns there)
    cu = np.zeros((64, 64), np.int64); cu[:, 32:] = 252
    cv = np.full((64, 64), 252); cv[:, 32:] = 0
    lu = [(r, c, 510 if r >= 64 else -255) for r in range(2, 128, 9) for c in range(1, 128, 11)]
    eu = [(r, c, 510 if c >= 32 else -255) for r in range(1, 64, 7) for c in range(1, 64, 5)]
    ev = [(r, c, -255 if c >= 32 else 510) for r in range(1, 64, 7) for c in range(1, 64, 5)]
    luma = np.zeros((512, 512), np.int64)
    luma[:256, :256] = -LEVEL_MAX; luma[128:256, :256] = LEVEL_MAX             # level 2: the bands beside and under the quadrant
    luma[:, 256:] = np.where(np.arange(512)[:, None] < 256, LEVEL_MAX, -LEVEL_MAX)
    luma[256:, :256] = np.where(np.arange(256)[None, :] < 128, LEVEL_MAX, -LEVEL_MAX)
    u = np.where(np.arange(256)[None, :] % 128 < 64, LEVEL_MAX, -LEVEL_MAX) * np.ones((256, 1), np.int64)
    return dict(luma=luma, u=u, v=-u, ll=ll, llu=cu, llv=cv, ex=(lu, eu, ev))


def _lone_groups(q):
    """a luma plane that is zero but for lone groups of eight cells, +-275 in cells 0 and 7 of each: k_dec_final's piece() takes a group and the
    two cells either side of it only where the row's group word says so.  Rows below 256 have groups 32 .. 63 (the detail half; half 0 of the kernel),
    rows from 256 on all 64 (half 1); band b of the output reads groups b and 32 + b"""
    luma = np.zeros((512, 512), np.int64)
    def put(row, *groups):
        for g in groups:
            luma[row, 8 * g] = LEVEL_MAX; luma[row, 8 * g + 7] = LEVEL_MIN
    put(300, 0); put(301, 63); put(302, 17); put(303, 45); put(304, 31); put(305, 32); put(306, 31, 32); put(307, 9, 10); put(308, 50, 51); put(309, 62, 63)
    put(310, 0, 1); put(500, 1); put(510, 62)
    put(10, 63); put(11, 40); put(12, 32); put(13, 45, 46); put(14, 62, 63); put(15, 32, 33); put(200, 33); put(255, 63); put(254, 32)
    u = np.zeros((256, 256), np.int64); v = u.copy()
    u[200, 8] = LEVEL_MAX; u[200, 15] = LEVEL_MIN; v[40, 248] = LEVEL_MIN; v[40, 255] = LEVEL_MAX
    ll, cu, cv = _flat(q)
    return dict(luma=luma, u=u, v=v, ll=ll, llu=cu, llv=cv)


LONE_ROWS = {"g0": (300,), "g63": (301, 10, 255), "interior": (302, 303, 11, 200), "pair": (307, 308, 13)}


def _corrections(many):
    """q23: corrections on one cell again and again (32-bit words of qs3: cell << 1 | sign, +-56; 16-bit words of char_res1: +-32), and corrections in
    the first and the last row a band of k_dec_final takes (columns r0 - 1 and r0 + 15 of the plane between the two directions)"""
    cell = lambda line, col: line * 512 + col
    qs3 = [cell(100, 40) << 1] * many + [(cell(300, 41) << 1) | 1] * many
    for line in (0, 5, 255, 256, 511):
        for col in (0, 14, 15, 16, 17, 31, 32, 255, 256, 495, 496, 510, 511):
            qs3.append((cell(line, col) << 1) | (col & 1))
    char = [4 * k for k in range(8, 40)] * 3 + [4 * k + 1 for k in range(200, 230)] + [4 * k + 2 for k in range(2000, 2010)] * 5 + [4 * k + 3 for k in range(16000, 16383, 7)]
    return qs3, char


def res1_on_cells(cells):
    """res1 (open above q12) as entries on chosen cells of the level-1 LL: cells = [(row, column, entries, sign)] in raster order, entries odd, sign +1
    (the list adds its step) or -1.  A cell is a column byte and step bytes of no step, two entries each; bytes of 127 count the rows; an odd
    column comes from the bit string (nhwo_dec.c:poslist_decode).  A column byte cannot be 127 and a step that reaches column 254 ends the row, so
    the lists reach columns 0 .. 253 only."""
    lst, bits, signs, row, lastcol = [], [], [], 0, -1
    for r, c, n, sg in cells:
        assert n % 2 == 1 and 0 <= c <= 253 and (r > row or (r == row and (c & ~1) >= lastcol))
        if not lst and r == 0:
            pass
        lst += [127] * (r - row) + [c >> 1] + [0x80] * (n // 2)
        bits += [c & 1] * n; signs += [0 if sg > 0 else 1] * n
        row, lastcol = r, c & ~1
    assert lst[0] != 127 or cells[0][0] > 0
    nbytes = -(-len(bits) // 8) + 1                                # (the lists take (bytes - 1) * 8 entries)
    assert nbytes <= (S.P16_CAP - 64) // 8
    pad = nbytes * 8 - len(bits)
    bits += [0] * pad; signs += [k & 1 for k in range(pad)]        # (entries the list does not reach land on cell (0, 0): they cancel but for one step)
    return dict(res1=bytes(lst), res1_bit=np.packbits(np.array(bits, np.uint8)).tobytes(), res1_word=np.packbits(np.array(signs, np.uint8)).tobytes())


def _marks_values(q):
    """cells a residual list drives above 10000, where the reference's mark list takes a cell by its value (nhwo_dec.c:630): inside the plane, two of them
    side by side, in column 0, and in rows 0 and 255, which the list's walk leaves out; one cell far below 0"""
    n = 2001                                                       # 128 + 2001 * 5 = 10133, * 7 = 14135
    return res1_on_cells([(0, 20, n, 1), (10, 0, n, 1), (10, 20, n, 1), (10, 21, n, 1), (10, 200, n, -1), (11, 0, n, 1), (12, 0, n, 1), (131, 253, n, 1),
                          (254, 0, n, 1), (254, 252, n, 1), (255, 30, n, 1)])


def _marks_plateau(q, up=True, down=False):
    """3 x 6 cells at one height beyond 16767 (and / or below -6000), the second cell of the pair (41, 42) of the middle row two steps further out and a
    neighbour of it likewise: its Laplacian is 14 steps (70 or 98), the first cell's -2 steps, so the pair rule marks it -- and 16000 more wraps"""
    amp = 5 if q >= 18 else 7
    cells = []
    def plateau(r0, n, sg):
        for r in range(r0, r0 + 3):
            for c in range(40, 46):
                cells.append((r, c, n + (2 if (r, c) in ((r0 + 1, 42), (r0, 43)) else 0), sg))
    if up: plateau(100, 3401 if amp == 5 else 2401, 1)
    if down: plateau(150, 1401 if amp == 5 else 1001, -1)
    return res1_on_cells(cells)


def _marks_edges(low):
    """the two edges of the value test, each the only cell of its file outside -5999 .. 10000 (amplitude 5, on a flat LL of 125 or 126).
    low: a 3 x 6 plateau at -5990 with the first cell of the pair (41, 42) of its middle row at -6000: Laplacians -80 and +10, so the pair rule marks it, it
    stands at exactly 10000, stays off the list and keeps that; and a lone cell at exactly 10000, which no rule touches.  not low (on 126): a lone cell at 10001,
    which the list takes."""
    if not low:
        return res1_on_cells([(50, 60, 1975, 1)])
    return res1_on_cells([(50, 60, 1975, 1)] + [(r, c, 1225 if (r, c) == (101, 41) else 1223, -1) for r in range(100, 103) for c in range(40, 46)])


def _pictures():
    """adversarial pictures for the oracle's encoder: a full-swing checkerboard, lone impulses, saturated fields"""
    i, j = np.mgrid[0:512, 0:512]
    chk = np.where((i + j) & 1, 255, 0).astype(np.uint8)
    imp = np.zeros((512, 512), np.uint8); imp[7::61, 5::53] = 255
    sat = np.zeros((512, 512, 3), np.uint8); sat[:, :256, 0] = 255; sat[256:, :, 1] = 255; sat[:256, 256:, 2] = 255
    blk = np.where(((i >> 3) + (j >> 3)) & 1, 255, 0).astype(np.uint8)
    return {"checkerboard": np.repeat(chk[:, :, None], 3, 2), "impulses": np.repeat(imp[:, :, None], 3, 2), "saturated": sat,
            "blocks8": np.stack([blk, 255 - blk, blk], 2)}


def _cases(oracle):
    out = []
    add = lambda name, family, q, data: out.append((name, family, q, data))
    for q in QUALITIES:
        ll, cu, cv = _flat(q)
        # all-maximal details; signs that maximise 6 h0 - hp - hm and (h0 + hm) << 1 in both directions at once
        for kind in ("plus", "minus"):
            l, u, v = _details(kind)
            add(f"q{q}_all_{kind}", "all_maximal", q, build(q, l, u, v, ll, cu, cv))
        for kind in {10: ("checker",), 16: ("checker",), 17: ("checker",), 20: ("checker", "rows", "cols"), 23: ("checker",)}[q]:
            l, u, v = _details(kind)
            a, b, c = _ll_pattern("max" if kind == "checker" else "min")
            add(f"q{q}_signs_{kind}", "filter_signs", q, build(q, l, u, v, a, b, c))
        # LL2 extremes, by differences and by verbatim tokens, with exception samples on the corners and edges of the bands
        z, zc = np.zeros((512, 512), np.int64), np.zeros((256, 256), np.int64)
        for kind, verbatim, ex in (("max", False, True), ("min", False, False), ("alt", True, True)):
            if kind == "min" and q in (16, 17, 20):
                continue
            a, b, c = _ll_pattern(kind)
            if verbatim and kind == "alt" and q > 15:
                a = a.copy(); a[4::2] |= 1                         # the fine bytes (samples 4, 6, ..) at 255 / 1, the verbatim samples behind them even
            add(f"q{q}_ll_{kind}{'_verbatim' if verbatim else ''}{'_ex' if ex else ''}", "ll2_extremes", q,
                build(q, z, zc, zc, a, b, c, verbatim=verbatim, ex=_edge_exceptions() if ex else None))
        add(f"q{q}_one_sided", "one_sided", q, build(q, **_one_sided(q)))
        add(f"q{q}_lone_groups", "lone_groups", q, build(q, **_lone_groups(q)))
        # the wrap cases of DESIGN.md section 7.1b.  Luma level 2 and both directions of level 1 wrap on the all-maximal and sign cases above (reach()
        # holds them to it); the smallest content named there, one at a time:
        l = np.zeros((512, 512), np.int64); l[0:128, 128:256] = LEVEL_MIN; l[128:256, 0:128] = LEVEL_MIN; l[128:256, 128:256] = LEVEL_MAX
        if q in (10, 23):
            add(f"q{q}_wrap_luma_level2", "wrap", q, build(q, l, zc, zc, *_ll_pattern("max")))
        u = zc.copy(); u[70, 10] = CHROMA_TAG_MAX; u[10, 70] = CHROMA_TAG_MAX; u[100, 100] = CHROMA_TAG_MAX - 3
        v = zc.copy(); v[64:128, 0:64] = CHROMA_TAG_MAX - 1; v[0:64, 64:128] = CHROMA_TAG_MAX - 2
        add(f"q{q}_wrap_chroma_tags", "wrap", q, build(q, z, u, v, ll, cu, cv))
        l = z.copy(); l[256:, :] = LUMA_TAG_MAX - 1; l[300:400, 256:] = LUMA_TAG_MAX
        if q in (16, 20):
            add(f"q{q}_wrap_luma_tags", "wrap", q, build(q, l, zc, zc, ll, cu, cv))
        if q > 12:                                                  # the first direction of level 1 wraps only behind a residual list (section 7.1b),
            # and a cell above 10000 meets the value test of the mark list
            add(f"q{q}_marks_values", "marks", q, build(q, z, zc, zc, ll, cu, cv, lists=_marks_values(q)))
            add(f"q{q}_marks_plateau", "marks", q, build(q, z, zc, zc, ll, cu, cv, lists=_marks_plateau(q, True, q < 18)))
            if q == 20:
                add("q20_marks_edge_low", "marks", q, build(q, z, zc, zc, _flat(q, 125)[0], cu, cv, lists=_marks_edges(True)))
            if q == 23:
                add("q23_marks_edge_high", "marks", q, build(q, z, zc, zc, _flat(q, 126)[0], cu, cv, lists=_marks_edges(False)))
            if q == 20:
                add(f"q{q}_marks_low", "marks", q, build(q, z, zc, zc, ll, cu, cv, lists=_marks_plateau(q, False, True)))
    # q23: repeated corrections
    ll, cu, cv = _flat(23)
    z, zc = np.zeros((512, 512), np.int64), np.zeros((256, 256), np.int64)
    for many in (40, 700):
        qs3, char = _corrections(many)
        l, u, v = _details("checker", 21)
        add(f"q23_corrections_x{many}", "corrections" if many < 600 else "wrap", 23, build(23, l, u, v, ll, cu, cv, qs3=qs3, char=char))
    # the + 32 of the second direction itself: T[10][20] = 4088 and T[266][20] = -24 put the even sample of pixel (20, 20) at 32752 in front of it
    A, B = 10 * 512 + 20, 266 * 512 + 20
    res6 = bytes([127] * 20 + [10] + [0x80] * 43 + [127] * 512 + [10])          # 87 entries on cell A, one on cell B, all + 32
    add("q23_wrap_plus32", "wrap", 23, build(23, z, zc, zc, ll, cu, cv, qs3=[A << 1] * 5 + [(B << 1) | 1],
                                              lists=dict(res6=res6, res6_bit=bytes(12), res6_word=bytes(12))))
    # what the oracle's own encoder makes of adversarial pictures
    for pname, img in _pictures().items():
        for q in {"checkerboard": (20, 10), "saturated": (17,), "impulses": (23,), "blocks8": (16,)}[pname]:
            add(f"q{q}_encoded_{pname}", "encoded", q, oracle.encode(img, q))
    return out


_CACHE = []


def cases(oracle=None):
    """[(name, family, quality, bytes)], a fixed list in a fixed order; the first call needs the oracle (for the encoded pictures)"""
    if not _CACHE:
        if oracle is None:
            from oracle.oraclepy import Oracle
            subprocess.check_call(["make", "-s", "-C", os.path.join(S.ROOT, "oracle")])
            oracle = Oracle(os.path.join(S.ROOT, "oracle", "liboracle.so"))
        out = _cases(oracle)
        assert len({n for n, *_ in out}) == len(out) and len({d for *_, d in out}) == len(out)
        _CACHE.extend(out)
    return list(_CACHE)


FAMILIES = {"all_maximal": QUALITIES, "filter_signs": QUALITIES, "ll2_extremes": QUALITIES, "one_sided": QUALITIES, "lone_groups": QUALITIES,
            "wrap": QUALITIES, "marks": (16, 17, 20, 23), "corrections": (23,), "encoded": QUALITIES}


# ---------------------------------------------------------------------------------------------- classification and the record
def classify_all(exe, tmpdir, cs, workers=8):
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda kc: S.classify_one(exe, kc[1][3], tmpdir, f"v{kc[0]}"), enumerate(cs)))


def conditions(cs, classes):
    """the two conditions on the classification -> the list of those missed: every family keeps a defined case at every quality it is built for, and
    at most one case in ten is undefined"""
    missed = []
    for fam, qs in FAMILIES.items():
        for q in qs:
            if not any(f == fam and cq == q and c == "defined" for (_, f, cq, _), c in zip(cs, classes)):
                missed.append(f"family {fam} has no defined case at q{q}")
    if 10 * sum(c == "undefined" for c in classes) > len(cs):
        missed.append(f"{sum(c == 'undefined' for c in classes)} of {len(cs)} cases are undefined")
    return missed


def load_record():
    with open(RECORD) as f:
        return json.load(f)


sha = lambda b: hashlib.sha256(b).hexdigest()


def main():
    import tempfile
    exe = S.build_asan()
    assert exe, "no sanitizer build"
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        res = classify_all(exe, tmp, cs)
    rec = {}
    for (name, fam, q, data), (cls, gq, px) in zip(cs, res):
        r = {"family": fam, "quality": q, "bytes": len(data), "nhw_sha256": sha(data), "class": cls}
        if cls == "defined":
            assert gq == q, name
            r["pixels_sha256"] = sha(px)
        if cls == "undefined":
            print(name, px)
        rec[name] = r
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(rec), "cases", {c: sum(r["class"] == c for r in rec.values()) for c in ("defined", "refused", "undefined")})
    print(conditions(cs, [r[0] for r in res]) or "both conditions met")


if __name__ == "__main__":
    main()
