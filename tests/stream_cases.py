"""Crafted symbol streams for the stream stage (tests/test_stream_stage.py): the list format of the device, and the case families.

A case is (name, luma, chroma): the luma part of the stream as the serpentine gather leaves it (uint8[262144]) and the chroma part as the
chroma quantisers leave it (uint8[131072], U and V interleaved).  128 is the zero symbol.  Only symbols the quantisers can write appear
(LUMA_ALPHABET, CHROMA_ALPHABET): the reference looks a symbol's rank up in the table that held its count, so a symbol that cannot enter
the code book would index the code table with a count.

The alphabets, from nhwo_quantise_luma / nhwo_quantise_chroma (oracle/nhwo_quant.c; image_processing.c:186-519, 108-183):
  luma    the multiples of 8 ((a + 128) & 248 for |a| < 128: 0 .. 248, 128 being the zero symbol), the marks 121, 122, 125, 126, 127, 129,
          and the 38 escape codes of |a| > 127 (k_big_pos, k_big_neg): 75 symbols that are not zero;
  chroma  the multiples of 8, the marks 122, 124, 126, 130 and the same escape codes: 73 symbols that are not zero.
The rewrites add 132 .. 135, 123 and 124 to the luma part's book symbols (153 .. 159 and 201 never enter a book).  A luma book can
therefore hold at most 76 + 6 symbols and the 252 run lengths 4 .. 255 = 334 entries, a chroma book 74 symbols and the 253 run lengths
3 .. 255 = 327: the `select++` loop (more than 354 entries, compress_pixel.c:128-236) cannot be reached by an admissible stream, and no
case tries to.
"""
import numpy as np

Q = 65536
NL, NC = 4 * Q, 2 * Q
Z = 128
BIG = (10, 12, 14, 18, 20, 22, 26, 28, 30, 34, 36, 38, 42, 44, 46, 50, 52, 54, 58,
       60, 62, 66, 68, 70, 74, 76, 78, 82, 84, 86, 90, 92, 94, 98, 100, 102, 106, 108)
MULT8 = tuple(v for v in range(0, 256, 8) if v != Z)
LUMA_ALPHABET = tuple(sorted(set(MULT8 + (121, 122, 125, 126, 127, 129) + BIG)))
CHROMA_ALPHABET = tuple(sorted(set(MULT8 + (122, 124, 126, 130) + BIG)))
LUMA_REWRITTEN = (123, 124, 132, 133, 134, 135)               # book symbols only the rewrites make
MAX_LUMA_ENTRIES = len(LUMA_ALPHABET) + 1 + len(LUMA_REWRITTEN) + len(range(4, 256))
MAX_CHROMA_ENTRIES = len(CHROMA_ALPHABET) + 1 + len(range(3, 256))
P8, M8 = 136, 120                                             # +8, -8
X = 144                                                       # a symbol no rewrite looks for
PLAIN_LUMA = tuple(v for v in LUMA_ALPHABET if v not in (P8, M8))   # what the luma cases use where they want no rewrite to fire


# ------------------------------------------------------------------------------------------------ the device's list format
def _luma_order(a):
    """[4096 slices in stream order, ...] -> the quantiser's order [flush][strip]: slice g = strip * 32 + flush"""
    return a.reshape((128, 32) + a.shape[1:]).swapaxes(0, 1).reshape(a.shape)


def _chroma_perm():
    """stream slice of entry F * 128 + 2 * lane + half of the chroma map (pack_chroma_order)"""
    S = np.arange(2048)
    strip, rem = S >> 6, S & 63
    F = 4 * (rem >> 4) + ((rem >> 2) & 3)
    lane = 2 * strip + ((rem >> 1) & 1)
    perm = np.empty(2048, np.int64)
    perm[F * 128 + 2 * lane + (rem & 1)] = S
    return perm


CHROMA_PERM = _chroma_perm()


def _maps(nz):
    return np.packbits(nz.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()


def lists_from_streams(luma, chroma):
    """The production list format from dense streams (the inverse of the decoding in test_symbol_list_equals_the_byte_stream).
    -> nzq:   uint8[32768 + 132]: the luma map, a uint64 per slice at [flush * 128 + strip] (slice g = strip * 32 + flush), then fbase (33 uint32)
       vals:  the luma symbols that are not zero, flush after flush, strip after strip, stream order inside a slice
       cnzq:  uint8[16384 + 80]: the chroma map at [F * 128 + 2 * lane + half], then cfbase (16 flush starts, 4 wavefront totals)
       cvals: uint8[131072]: a wavefront's values from 32768 * wavefront on"""
    luma = np.asarray(luma, np.uint8); chroma = np.asarray(chroma, np.uint8)
    assert luma.size == NL and chroma.size == NC
    sl = _luma_order(luma.reshape(4096, 64))
    nz = sl != Z
    fbase = np.zeros(33, np.uint32)
    fbase[1:] = np.cumsum(nz.reshape(32, -1).sum(1))
    nzq = np.concatenate([_maps(nz).view(np.uint8), fbase.view(np.uint8)])
    vals = sl[nz]
    cs = chroma.reshape(2048, 64)[CHROMA_PERM]
    cnz = cs != Z
    per_flush = cnz.reshape(16, -1).sum(1)
    cfbase = np.zeros(20, np.uint32)
    cvals = np.zeros(NC, np.uint8)
    for wv in range(4):
        at = 0
        for t in range(4):
            cfbase[4 * wv + t] = 32768 * wv + at
            at += int(per_flush[4 * wv + t])
        cfbase[16 + wv] = at
        cvals[32768 * wv:32768 * wv + at] = cs[512 * wv:512 * wv + 512][cnz[512 * wv:512 * wv + 512]]
    cnzq = np.concatenate([_maps(cnz).view(np.uint8), cfbase.view(np.uint8)])
    return dict(nzq=nzq, vals=vals, cnzq=cnzq, cvals=cvals)


def lists_from_rewritten(luma):
    """B_NZS / B_VOFF / B_VALS as scan_rewrite_list_par leaves them, from a luma stream behind the three rewrites: the map and the value
    offsets in stream order, the values in the quantiser's order, and in the top three bits of a slice's offset word how many symbols at its
    head a 132 .. 135 code of the slice before covers (a code at slice offset 60 .. 63: offset - 59)."""
    luma = np.asarray(luma, np.uint8)
    sl = luma.reshape(4096, 64)
    nz = sl != Z
    cnt = _luma_order(nz.sum(1))                                 # [flush][strip]
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32)
    voff = start.reshape(32, 128).swapaxes(0, 1).reshape(-1).copy()   # back to stream order
    codes = np.flatnonzero((luma >= 132) & (luma <= 135))
    codes = codes[(codes & 63) >= 60]
    voff[(codes >> 6) + 1] |= ((codes & 63) - 59).astype(np.uint32) << 29
    o = _luma_order(sl)
    return dict(nzs=_maps(nz), voff=voff, vals=o[o != Z])


def dense_from_lists(nzs, voff, vals):
    """the dense luma stream of B_NZS / B_VOFF / B_VALS"""
    bits = np.unpackbits(np.asarray(nzs, np.uint64).view(np.uint8), bitorder="little").astype(bool)
    cnt = bits.reshape(-1, 64).sum(1)
    off = (np.asarray(voff, np.uint32) & 0x1FFFFFFF).astype(np.int64)
    out = np.full(NL, Z, np.uint8)
    if cnt.sum():
        idx = np.repeat(off - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())
        out[bits] = np.asarray(vals, np.uint8)[idx]
    return out


# ------------------------------------------------------------------------------------------------ builders
def zl():
    return np.full(NL, Z, np.uint8)


def zc():
    return np.full(NC, Z, np.uint8)


def pm(k):
    return P8 if k else M8


def _put(s, at, v):
    if 0 <= at < s.size:
        s[at] = v


def chain(s, head, m, sa, sb):
    """m candidates four apart from `head`: m + 1 symbols +-8, signs alternating (sa, sb)"""
    for k in range(m + 1):
        _put(s, head + 4 * k, pm(sa if k % 2 == 0 else sb))


# ------------------------------------------------------------------------------------------------ rewrite 1
def rewrite1_cases():
    cases = []
    for sa in (0, 1):
        for sb in (0, 1):
            s = zl()                                             # chains of 1 .. 9 candidates, every chain head at slice offsets 52 .. 63
            at = 640
            for m in range(1, 10):
                for o in range(52, 64):
                    chain(s, at + o, m, sa, sb)
                    s[at + o + 4 * m + 7] = X                        # keeps the zero runs between the chains short
                    at += 128
            cases.append((f"r1 chains sign{sa}{sb}", s, zc()))
    s = zl()                                                     # across a 2048-symbol strip edge (the flush changes), every split of the five symbols
    for k, m in enumerate((1, 1, 1, 1, 2, 3, 4, 9)):
        chain(s, 2048 * (3 + 5 * k) - 1 - (k % 4), m, k & 1, (k >> 1) & 1)
    cases.append(("r1 strip edges", s, zc()))
    for m in (1, 2, 3):                                          # inside a slice of more than 16 values, the chain behind the sixteenth
        s = zl()
        for g in (9, 40, 4095 - 7):
            s[64 * g:64 * g + 18] = PLAIN_LUMA[:18]
            chain(s, 64 * g + 18, m, g & 1, 1)
            s[64 * g + 19 + 4 * m + 4:64 * g + 59] = X
            chain(s, 64 * g + 60, m, 1, g & 1)                      # and one that leaves such a slice
        cases.append((f"r1 full slice m{m}", s, zc()))
    for head in range(4):                                        # at positions 0 .. 3, which are cleared afterwards
        for m in (1, 2):
            s = zl()
            chain(s, head, m, head & 1, 1)
            s[40] = X
            cases.append((f"r1 head{head} m{m}", s, zc()))
    for end in (NL - 5, NL - 4):                                 # ending at n - 5 and at n - 4
        for m in (1, 2, 3):
            s = zl()
            chain(s, end - 4 * m, m, 1, m & 1)
            cases.append((f"r1 end{NL - end} m{m}", s, zc()))
    for behind in ((X, X, X), (Z, X, 16), (X, Z, P8), (P8, Z, Z)):  # a selected code at slice offsets 59 .. 63, symbols right behind its five
        s = zl()
        at = 64 * 5
        for o in range(59, 64):
            for sa in (0, 1):
                chain(s, at + o, 1, sa, o & 1)
                s[at + o + 5:at + o + 8] = behind
                at += 64 * 3
                chain(s, at + o, 3, sa, 1)                           # two selected pairs eight apart
                s[at + o + 13:at + o + 16] = behind
                at += 64 * 3
        cases.append((f"r1 skip bits {behind}", s, zc()))
    return cases


# ------------------------------------------------------------------------------------------------ rewrite 2
def _r2_pattern(s, kind, i, a, b):
    """the second rewrite's rules at anchor i (nhw_encoder.c:2178-2220)"""
    if kind == "lone before4":                                   # four zeros before, one behind
        _put(s, i - 5, X); _put(s, i, pm(a)); _put(s, i + 2, X)
    elif kind == "lone after4":                                  # one zero before, four behind
        _put(s, i - 2, X); _put(s, i, pm(a)); _put(s, i + 5, X)
    elif kind == "pair before4":                                 # pair rule 1: four zeros before the first, one behind the second
        _put(s, i - 5, X); _put(s, i, pm(a)); _put(s, i + 1, pm(b)); _put(s, i + 3, X)
    elif kind == "pair after4":                                  # pair rule 2: one zero before, four behind
        _put(s, i - 2, X); _put(s, i, pm(a)); _put(s, i + 1, pm(b)); _put(s, i + 6, X)
    elif kind == "taken before4":                                # the anchor is the second of a pair: taken by its left neighbour
        _put(s, i - 6, X); _put(s, i - 1, pm(a)); _put(s, i, pm(b)); _put(s, i + 2, X)
    elif kind == "taken after4":
        _put(s, i - 3, X); _put(s, i - 1, pm(a)); _put(s, i, pm(b)); _put(s, i + 5, X)
    elif kind == "pair then lone":                               # the second of a pair, then a zero and a third +-8 that stays alone
        _put(s, i - 5, X); _put(s, i, pm(a)); _put(s, i + 1, pm(b)); _put(s, i + 3, pm(a)); _put(s, i + 8, X)
    elif kind == "no rule":                                      # three zeros before, three behind: nothing fires
        _put(s, i - 4, X); _put(s, i, pm(a)); _put(s, i + 4, X)


R2_KINDS = ("lone before4", "lone after4", "pair before4", "pair after4", "taken before4", "taken after4", "pair then lone", "no rule")


def rewrite2_cases():
    cases = []
    for a in (0, 1):
        for b in (0, 1):
            s = zl()
            at = 64 * 4
            for kind in R2_KINDS:
                for o in (0, 1, 2, 3, 4, 59, 60, 61, 62, 63):
                    _r2_pattern(s, kind, at + o, a, b)
                    s[at + 128] = X
                    at += 192
            cases.append((f"r2 slice offsets sign{a}{b}", s, zc()))
    for k, kind in enumerate(R2_KINDS):                          # at i = 4 and at i = n - 5: the ends of the rewrite's range
        for i in (4, 5, NL - 5, NL - 6):
            s = zl()
            _r2_pattern(s, kind, i, k & 1, (k >> 1) & 1)
            s[1000] = X
            cases.append((f"r2 {kind} at {i if i < 100 else i - NL}", s, zc()))
    return cases


# ------------------------------------------------------------------------------------------------ rewrite 3
R3_RUNS = tuple(range(250, 259)) + tuple(range(254 * 2 - 1, 254 * 2 + 3)) + tuple(range(254 * 3 - 1, 254 * 3 + 3)) + (2048,)


def rewrite3_cases():
    cases = []
    for d in (1, 2, 3, 4):                                       # the lone +-8 at +1 .. +4 behind the run
        for a in (0, 1):
            s = zl()
            at = 8
            for o in (0, 1, 15, 16, 17, 60, 63):                 # where the run starts, in its slice and in a group of sixteen
                for L in R3_RUNS:
                    st = (at + 63 - o) // 64 * 64 + o + 64
                    s[at:st] = X                                 # non-zero up to the run
                    p = st + L                                   # the first symbol behind the run
                    if d > 1:
                        s[p] = X
                    s[p + d - 1] = pm(a ^ (L & 1))
                    s[p + d + 4] = X                             # four zeros behind the +-8
                    at = p + d + 5
            assert at < NL - 8
            s[at:at + 40] = X
            cases.append((f"r3 runs +{d} sign{a}", s, zc()))
    cases.append(("r3 all zero", zl(), zc()))
    for name, at in (("first", 0), ("fifth", 4), ("last", NL - 1), ("fifth from the end", NL - 5)):
        for v in (X, P8):
            s = zl(); s[at] = v
            cases.append((f"r3 zero but for the {name} symbol ({v})", s, zc()))
    return cases


# ------------------------------------------------------------------------------------------------ run tokens (both parts)
def _run_stream(n, lengths, seps, phase=0):
    """runs of the given lengths, a symbol of `seps` (cycled) between them; `phase` symbols first; the rest of the stream is not zero"""
    s = np.full(n, seps[0], np.uint8)
    at = phase
    for k, L in enumerate(lengths):
        if at + L + 2 > n:
            break
        s[at:at + L] = Z
        s[at + L] = seps[k % len(seps)]
        at += L + 1
    return s


def _aligned_runs(n, lengths, seps):
    """every length at every start offset mod 64"""
    s = np.full(n, seps[0], np.uint8)
    at, k, done = 1, 0, []
    for L in lengths:
        for o in range(64):
            st = at + ((o - at) % 64)
            if st + L + 2 > n:
                return s, done
            s[st:st + L] = Z
            s[st + L] = seps[k % len(seps)]; k += 1
            at = st + L + 1
        done.append(L)
    return s, done


def _both(name, fl, fc):
    """a luma case beside a quiet chroma part, and the same for the chroma part"""
    quiet_l, quiet_c = np.full(NL, X, np.uint8), np.full(NC, X, np.uint8)
    return [(name + " luma", fl, quiet_c), (name + " chroma", quiet_l, fc)]


def run_cases():
    cases = []
    for ph in (0, 21, 42):                                       # every run length 1 .. 260; the start offsets sweep the residues
        ln = [L for _ in range(8) for L in range(1, 261)]
        cases += _both(f"runs 1..260 phase {ph}", _run_stream(NL, ln, (X, 16), ph), _run_stream(NC, ln, (X, 16, 130), ph))
    lens = list(range(250, 261))                                 # the lengths around the pieces of 254, at every start offset mod 64
    s, done = _aligned_runs(NL, lens, (X, 8))
    assert done == lens
    cases.append(("runs 250..260 aligned luma", s, np.full(NC, X, np.uint8)))
    while lens:
        s, done = _aligned_runs(NC, lens, (X, 8))
        cases.append((f"runs {done[0]}..{done[-1]} aligned chroma", np.full(NL, X, np.uint8), s))
        lens = lens[len(done):]
    s, done = _aligned_runs(NL, (508, 509, 510, 762, 763, 1016), (X, 8))
    cases.append(("runs of several pieces aligned luma", s, np.full(NC, X, np.uint8)))
    s, done = _aligned_runs(NC, (508, 509, 510), (X, 8))
    cases.append(("runs of several pieces aligned chroma", np.full(NL, X, np.uint8), s))
    short = [2, 3, 2, 2, 3, 1, 4, 3, 3, 2, 5] * 3000             # runs of 2 and 3: below `select`
    cases += _both("runs of 2 and 3", _run_stream(NL, short, (X, 16, 24)), _run_stream(NC, short, (X, 16, 24)))
    return cases


def tail_cases():
    """runs that end at N - 1 and at N - 2, the last symbol zero and not: the last symbol is never walked (a run can end in it), and the chroma
    part's is a copy of the one before it (compress_pixel.c:464-465)"""
    cases = []
    for L in (1, 3, 64, 254, 255, 256):
        for tail in ((Z, Z), (Z, X), (X, Z), (X, 16), (16, 16)):
            fl, fc = np.full(NL, X, np.uint8), np.full(NC, X, np.uint8)
            for f in (fl, fc):
                f[5000:5007] = Z                                 # (a run elsewhere)
                f[f.size - 2 - L:f.size - 2] = Z
                f[f.size - 2:] = tail
            cases += _both(f"run of {L} before the tail {tail}", fl, fc)
    return cases


# ------------------------------------------------------------------------------------------------ slice load
LOADS = (0, 1, 15, 16, 17, 32, 33, 48, 49, 64)


def load_cases():
    cases = []
    rng = np.random.default_rng(41)
    for name, spread in (("leading", False), ("spread", True)):
        def make(n, alpha):
            s = np.full(n, Z, np.uint8).reshape(-1, 64)
            for g in range(s.shape[0]):
                k = LOADS[(g + g // 32) % len(LOADS)]
                pos = np.sort(rng.choice(64, k, replace=False)) if spread else np.arange(k)
                s[g, pos] = rng.choice(alpha, k)
            return s.ravel()
        cases.append((f"slice loads {name}", make(NL, PLAIN_LUMA[:12]), make(NC, CHROMA_ALPHABET[:12])))
        fl = make(NL, (P8, M8, X, 16))
        fl[:8] = Z                                               # no chain head at 0 .. 3 (orphans below)
        cases.append((f"slice loads {name}, with +-8", fl, make(NC, (P8, M8, X, 16))))
    cases.append(("every symbol non-zero", rng.choice(LUMA_ALPHABET, NL).astype(np.uint8), rng.choice(CHROMA_ALPHABET, NC).astype(np.uint8)))
    cases.append(("every symbol non-zero, two symbols", rng.choice((X, 16), NL).astype(np.uint8), rng.choice((X, 16), NC).astype(np.uint8)))
    return cases


# ------------------------------------------------------------------------------------------------ bit budget of a slice
def _budget(n, r0, r1, step, extra=None):
    """r0 everywhere (rank 0: two bits a symbol, 128 bits a slice: the last value of the fast path); every `step`-th slice holds one r1 (rank 1:
    three bits, 129 bits a slice), so that the slices behind it start one bit later: every alignment in a word"""
    s = np.full(n, r0, np.uint8).reshape(-1, 64)
    for g in range(0, s.shape[0], step):
        s[g, (7 * g) % 64] = r1
    if extra:
        for g in range(5, s.shape[0], 97):
            s[g, 3:3 + len(extra)] = extra
    return s.ravel()


def budget_cases():
    cases = []
    for step in (2, 3, 5):
        cases.append((f"128 / 129 bits, every {step}", _budget(NL, X, 112, step), _budget(NC, X, 112, step)))
    cases.append(("128 / 129 / 130 / 131 bits", _budget(NL, X, 112, 3, (112, 112)), _budget(NC, X, 112, 3, (112, 112))))
    cases.append(("128 / 129 bits and a zero", _budget(NL, X, 112, 3, (Z,)), _budget(NC, X, 112, 3, (Z,))))
    cases.append(("128 / 129 bits and a run of five", _budget(NL, X, 112, 4, (Z,) * 5), _budget(NC, X, 112, 4, (Z,) * 5)))
    return cases


# ------------------------------------------------------------------------------------------------ code books
def book_stream(part, k, zero):
    """A stream whose book has exactly k entries: run lengths from `select` up, one run each, and symbols between them.
    zero: "top" -- isolated zeros outnumber everything (the zero symbol has rank 0); "low" -- one isolated zero; "none" -- no zero entry.
    The rest of the stream holds the book's symbols in turn ("top": (zero, symbol) pairs)."""
    n, select = (NC, 3) if part else (NL, 4)
    alpha = CHROMA_ALPHABET if part else PLAIN_LUMA
    nruns = min(k - 8, 256 - select)
    nsym = k - nruns - (zero != "none")
    assert 1 <= nsym <= len(alpha)
    syms = alpha[:nsym]
    s = np.empty(n, np.uint8)
    at = 5                                                       # (the luma part's first and last four symbols are cleared: two runs of four)
    s[:at] = syms[0]
    k_ = 0
    lengths = list(range(select, select + nruns))
    if not part:                                                 # the cleared head and tail of the luma part are runs of four themselves
        lengths = lengths[1:]
    for L in lengths:
        s[at:at + L] = Z
        s[at + L] = syms[k_ % nsym]; k_ += 1
        at += L + 1
    if zero == "low":
        s[at] = Z; s[at + 1] = syms[0]; at += 2
    if zero == "top":
        rest = np.empty(n - at, np.uint8)
        rest[0::2] = Z
        rest[1::2] = np.resize(np.array(syms, np.uint8), rest[1::2].size)
        s[at:] = rest
        s[-8:] = syms[0]
    else:
        s[at:] = np.resize(np.array(syms, np.uint8), n - at)
    return s


def book_cases():
    cases = []
    for k in (100, 150, 200, 289, 290, 291):                     # ranks below 110, in the zone 110 .. 173, behind it; the 290-entry limit
        for zero in ("top", "low", "none"):
            for part in (0, 1):
                s = book_stream(part, k, zero)
                quiet = np.full(NC if not part else NL, X, np.uint8)
                cases.append((f"book {'chroma' if part else 'luma'} k{k} zero {zero}", quiet if part else s, s if part else quiet))
    return cases


def stale_streams(luma_long):
    """The chroma book's collapse reads on into the bytes the luma book left (compress_pixel.c:58, :442-456) when the chroma table ends in a
    run of 128s.  luma: filler X (rank 0, one byte), then the run lengths 4, 5, 6 ... once each: de-interleaved, [X, 4, 5, ..., 128, ...]
    and then the 3s, so byte 125 is the length 128.  chroma: s symbols in front (an odd count: the run entries' 128s fall on odd bytes and
    close the de-interleaved table), r run lengths once each, s + 2 r bytes.  With s + 2 r = 125 the run of 128s reads on into that byte."""
    out = []
    for s_ in (25, 27, 1, 41):
        for e2 in (123, 125, 127):
            r = (e2 - s_) // 2
            if luma_long:
                fl = np.full(NL, X, np.uint8)
                at = 8
                for L in range(5, 140):
                    fl[at:at + L] = Z; at += L + 1
            else:
                fl = np.full(NL, X, np.uint8)
                fl[100:228] = Z                                  # a short book that holds the run length 128 all the same
            syms = CHROMA_ALPHABET[:s_]
            fc = np.full(NC, syms[0], np.uint8)
            at = 8
            for k in range(4 * s_):                              # every symbol four times: in front of the runs, by weight
                fc[at] = syms[k % s_]; at += 1
            for L in range(3, 3 + r):
                fc[at:at + L] = Z; at += L + 1
            out.append((f"stale bytes, luma book {'long' if luma_long else 'short'}, chroma {s_} symbols {r} runs", fl, fc))
    return out


def stale_cases():
    return stale_streams(True) + stale_streams(False)


# ------------------------------------------------------------------------------------------------ capacity
def dense_pair(seed):
    rng = np.random.default_rng(seed)
    return rng.choice(LUMA_ALPHABET, NL).astype(np.uint8), rng.choice(CHROMA_ALPHABET, NC).astype(np.uint8)


def trim_chroma(chroma, m):
    """the first m symbols of a dense chroma part, zeros behind them"""
    c = chroma.copy()
    c[m:] = Z
    return c


def capacity_cases(oracle, targets=(79997, 79998, 79999, 80000, 80001, 80002, 80003, 80010)):
    """Dense streams (every symbol non-zero, the whole alphabet) whose chroma part is cut short until luma + chroma take `target` packet
    words, by the oracle's count.  -> [(name, luma, chroma, words)]; a target no cut reaches exactly is left out."""
    luma, chroma = dense_pair(77)
    words = lambda m: oracle.stream_stage(luma, trim_chroma(chroma, m), 1)["words"]
    lo, hi = 0, NC
    assert words(lo) < min(targets) and words(hi) > max(targets)
    while hi - lo > 1:                                           # the last cut below the first target
        mid = (lo + hi) // 2
        if words(mid) < min(targets):
            lo = mid
        else:
            hi = mid
    found, m = {}, lo
    while len(found) < len(targets) and m < NC:
        w = words(m)
        if w in targets and w not in found:
            found[w] = m
        if w > max(targets) + 50:
            break
        m += 1
    return [(f"capacity {w} words", luma, trim_chroma(chroma, found[w]), w) for w in sorted(found)]


# ------------------------------------------------------------------------------------------------ random sweep
def sweep_cases(n=64, seed=2024):
    cases = []
    dens = [2.0 ** -k for k in range(9)]                         # 1/256 .. 1
    for i in range(n):
        rng = np.random.default_rng(seed + i)
        d = dens[i % 9]
        kind = (i // 9) % 3
        la = (P8, M8) if kind == 0 else (P8, M8, X, 16, 121, 127, 58, 108) if kind == 1 else LUMA_ALPHABET
        ca = (P8, M8) if kind == 0 else (P8, M8, X, 16, 122, 130, 58, 108) if kind == 1 else CHROMA_ALPHABET
        w = np.where(np.isin(la, (P8, M8)), 1.0 + 3 * (i % 2), 1.0)   # every other stream: +-8 four times as likely (the rewrites' food)
        fl = np.where(rng.random(NL) < d, rng.choice(la, NL, p=w / w.sum()), Z).astype(np.uint8)
        fc = np.where(rng.random(NC) < d, rng.choice(ca, NC), Z).astype(np.uint8)
        if i % 4 == 3:                                           # long zero runs in between
            for at in rng.integers(0, NL - 3000, 12):
                fl[at:at + int(rng.integers(200, 2600))] = Z
            for at in rng.integers(0, NC - 3000, 8):
                fc[at:at + int(rng.integers(200, 2600))] = Z
        fl[:8] = Z                                               # no chain head at 0 .. 3 (orphans below)
        cases.append((f"sweep {i} density 1/{int(1 / d)} alphabet {len(la)}", fl, fc))
    return cases


FAMILIES = {
    "rewrite1": rewrite1_cases, "rewrite2": rewrite2_cases, "rewrite3": rewrite3_cases, "runs": run_cases, "tails": tail_cases,
    "load": load_cases, "budget": budget_cases, "book": book_cases, "stale": stale_cases, "sweep": sweep_cases,
}
# the batches of the GPU tests: 32 to 64 streams a hook call
BATCHES = {"rewrites 1 and 3, runs": ("rewrite1", "rewrite3", "runs"), "rewrite 2, loads, budgets": ("rewrite2", "load", "budget"),
           "books": ("book", "stale"), "tails": ("tails",), "sweep": ("sweep",)}


def family(name):
    return [(f"{name}: {n}", l, c) for n, l, c in FAMILIES[name]()]


def batch(name):
    return [c for f in BATCHES[name] for c in family(f)]


def orphans(rewritten):
    """(201s whose 132 .. 135 code is gone, all 201s) of a luma part behind the rewrites.  A chain head at positions 0 .. 3 is cleared and
    leaves its partner, a 201, to be walked: the reference then takes the COUNT of all 201s for its rank (201 enters no book), and reads
    past its code table from a count of 290 on.  A picture cannot do this (the stream's first symbols are cells of the LL2 band, which
    holds zero symbols); the cases that do it on purpose keep the count at one or two, every other case keeps the head of the stream zero."""
    at = np.flatnonzero(rewritten == 201)
    code = rewritten[np.maximum(at - 4, 0)]
    return int(((code < 132) | (code > 135)).sum()), at.size


def admissible(name, luma, chroma):
    bad_l = np.setdiff1d(np.unique(luma), np.array(LUMA_ALPHABET + (Z,)))
    bad_c = np.setdiff1d(np.unique(chroma), np.array(CHROMA_ALPHABET + (Z,)))
    assert bad_l.size == 0 and bad_c.size == 0, f"{name}: symbols no quantiser writes: luma {bad_l.tolist()} chroma {bad_c.tolist()}"


# ------------------------------------------------------------------------------------------------ the record
SCALARS = ("status", "select1_pre", "select2_pre", "select1", "select2", "size_data1", "size_data2", "size_book1", "size_book2", "tree_end",
           "wavelet_type", "words")
ARRAYS = ("luma", "packet", "book1", "book2", "sel_word1", "sel_word2")


def digest(r):
    """a short hash of everything Oracle.stream_stage returns (the packet: its first min(words, 80000) words)"""
    import hashlib
    h = hashlib.sha256()
    h.update(np.array([r[k] for k in SCALARS], np.int64).tobytes())
    for k in ARRAYS:
        a = np.ascontiguousarray(r[k])
        h.update(np.int64(a.nbytes).tobytes()); h.update(a.tobytes())
    return h.hexdigest()[:24]


def all_cases(oracle):
    """every case of the record, in its order: the families, then the capacity cases"""
    out = [c for f in FAMILIES for c in family(f)]
    return out + [(n, l, c) for n, l, c, _ in capacity_cases(oracle)]
