"""The table of hand-assembled DEFLATE streams (TEST INFRASTRUCTURE: test_deflate_craft.py, test_wavesim_deflate_craft.py,
test_gpu_deflate_craft.py).  Family A (valid()): what the format allows and libz never writes; every case decodes to the token
model's bytes with status 0.  Family B (invalid()): every way the reference refuses a stream, each with nothing, with 64 zero bytes
and with 64 bytes of 0xFF behind the fault, and the status stated by hand with the line of the reference's src/flate.rs it comes from
(oracle/o_flate.c carries those line numbers).  The sizes are the kernels' constants: k_inflate3.hip's MCAP 64 (matches up to here ride
in a batch), LCAP 32 (literals per run), 64 descriptors, INF3_LITCAP 320, INF3_H 768 / INF3_TCAP 1024 (LDS window), CB 1024 (staged
bytes), 128-bit segments in 8192-bit tiles; k_inflate2.hip's F2_NEAR 112."""
import struct
import zlib

import numpy as np

import deflate_craft as D
from deflate_craft import Stream

(E_EOF, E_TOO_SMALL, E_MALFORMED, E_TREE_TOO_LARGE, E_BLOCK_CODE, E_HEADER_SYMBOL, E_TREE, E_TREE_HEADER, E_CODE, E_STATIC_SIZE,
 E_NOT_ENOUGH_BITS) = 1, 2, 3, 10, 11, 12, 13, 14, 15, 16, 17
E_ZLIB_CHECKSUM, E_GZIP_CRC, E_GZIP_ISIZE = 24, 53, 54
ST_FALLBACK = 0x7ff00001                       # k_inflate3.hip: the first pass hands the stream back
MCAP, LCAP, NDESC, LITCAP, WIN_H, WIN_T, CB, F2_NEAR = 64, 32, 64, 320, 768, 1024, 1024, 112
TAILS = (("", b""), (" +00", b"\0" * 64), (" +ff", b"\xff" * 64))


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def lits(data):
    return [(0, b) for b in data]


def ladder(symbols, size):
    """lengths 1, 2, .., 14, 15, 15 for the sixteen symbols, in their order"""
    assert len(symbols) == 16
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, 15)
    return lens


# ------------------------------------------------------------------------------------------------------------------ family A: valid
_valid = None


def valid():
    """[dict(name, stream, want, flags, libz (True, the reason libz refuses what the reference takes, or None: not asked))]"""
    global _valid
    if _valid is not None:
        return _valid
    cs = []

    def add(name, s, libz=True, want=None):
        want = s.expected() if want is None else want
        assert want is not None, name
        cs.append({"name": name, "stream": s.bytes(), "want": want, "flags": s.flags(), "libz": libz})

    # ---- long codes: lit/len lengths 1 .. 14, 15, 15 (most literals lie beyond the 9-bit table), the same for the distances; a
    # match of 15 + 5 + 15 + 13 = 48 bits (length symbol 284, distance symbol 28: from position 16385 on, which 64 matches of 258
    # bytes with short codes reach); the end of block as one of the 15-bit codes, or as the 1-bit one
    L16 = [0x41 + i for i in range(13)]
    ll_lit = ladder(L16 + [285, 256, 0xFF], 286)                  # the end of block has 15 bits
    ll_eob1 = ladder([256] + L16 + [285, 0xFF], 286)              # ... one bit
    d16 = ladder([0, 1, 2, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 28, 29], 30)
    text = bytes(L16) + bytes(L16[::-1]) + b"\xff" + bytes(L16[6:])
    add("long ll codes", Stream().dynamic(lits(text), ll_lit, [0], final=True))
    add("long ll codes, eob 1 bit", Stream().dynamic(lits(text), ll_eob1, [0], final=True))
    toks = lits(text) + [(258, d) for d in (1, 3, 8, 13, 30, 100, 200, 500, 1000)] + lits(text[:5]) + [(258, 2000), (258, 4)]
    add("long distance codes", Stream().dynamic(toks, ll_lit, d16, final=True))
    add("long codes, repeats in the header", Stream().dynamic(lits(text[:16]) + [(258, 1), (258, 13), (0, 0xFF)], ll_lit, d16, final=True, rle=D.greedy_rle))
    ll48 = ladder([285, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x6b, 0x6c, 0x6d, 284, 256], 286)
    ll48e = ladder([285, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x6b, 0x6c, 256, 284, 0x6d], 286)
    fill = lits(b"abcdefghijklm") + [(258, 13)] * 64              # 16525 bytes
    m48 = [(227 + 7, 16385 + 77, 284, 7), (0, 0x62), (227 + 30, 16385 + 300, 284, 30), (227, 16385, 284, 0)]
    add("match of 48 bits", Stream().dynamic(fill + m48, ll48, d16, final=True))
    add("match of 48 bits, eob 15 bits", Stream().dynamic(fill + m48 + [(0, 0x6d)], ll48e, d16, final=True))

    # ---- lengths
    add("every length", Stream().fixed(lits(b"xyz") + [(n, 3) for n in range(3, 259)] + lits(b"!"), final=True))
    add("258 as 285 and as 284+31", Stream().fixed(lits(b"pq") + [(258, 2), (258, 1, 284, 31), (0, 7), (258, 2, 284, 31), (258, 258)], final=True))
    pre = rand(80, 20)
    for n in (MCAP - 1, MCAP, MCAP + 1, MCAP + 2):                # batch or wave-wide copy
        for d in (1, 2, 3, 4, 15, 16, 17, n + 5):
            add("length %d distance %d" % (n, d), Stream().fixed(lits(pre) + [(n, d), (0, 1), (n, d), (5, n + 3)], final=True))
    # ... and with the length symbol (276: 59 .. 66) as a 15-bit code, which the general one-symbol path decodes
    ll276 = ladder(L16 + [256, 276, 0xFF], 286)
    pre = bytes(L16[(i * i + i // 3) % 13] for i in range(80))
    for n in (MCAP - 1, MCAP, MCAP + 1, MCAP + 2):
        toks = lits(pre) + [t for d in (1, 2, 3, 4, 15, 16, 17, n + 5) for t in ((n, d), (0, 0x41 + d % 13))]
        add("length %d by a 15-bit code" % n, Stream().dynamic(toks, ll276, D.lens_for(toks)[1], final=True, rle=D.greedy_rle))

    # ---- distances
    r32 = rand(32768, 21)
    alld = [(3 + k % 7, D.DBASE[k] + x) for k in range(30) for x in (0, (1 << D.DEXTRA[k]) - 1)]
    add("every distance symbol", Stream().stored(r32).fixed(alld, final=True))
    for n in (1, 5, 300):
        add("distance = output so far %d" % n, Stream().fixed(lits(rand(n, 22)) + [(9, n)], final=True))
    add("32768 at 32768", Stream().stored(r32).fixed([(10, 32768), (0, 3), (70, 32768)], final=True))
    for d in (WIN_H - 1, WIN_H, WIN_H + 1, WIN_T - 1, WIN_T, WIN_T + 1):        # around the LDS window
        add("window distance %d" % d, Stream().fixed(lits(rand(d, 23)) + [(20, d), (0, 9), (100, d), (3, d)], final=True))
    add("window distances behind a stored block", Stream().stored(rand(1100, 24)).fixed(
        [t for d in (767, 768, 769, 1023, 1024, 1025) for t in ((20, d), (0, d & 255), (70, d))], final=True))
    for d in (F2_NEAR - 1, F2_NEAR, F2_NEAR + 1):                 # the lane kernels' gathers, at every alignment of the match's start
        for a in range(16):
            add("near %d at %d" % (d, a), Stream().fixed(lits(rand(128 + a, 25 + a)) + [(40, d), (0, 2), (17, d)], final=True))

    # ---- batch limits
    four = lits(b"wxyz")
    for n in (LCAP - 1, LCAP, LCAP + 1, 2 * LCAP - 1, 2 * LCAP, 2 * LCAP + 1):
        add("%d literals between matches" % n, Stream().fixed(four + [(4, 4)] + lits(rand(n, 40 + n)) + [(5, 3), (0, 0)], final=True))
    for n in (NDESC - 1, NDESC, NDESC + 1, 2 * NDESC + 1):
        add("%d matches in a row" % n, Stream().fixed(four + [(3 + k % 3, 1 + k % 4) for k in range(n)] + [(0, 1)], final=True))
    for n in (LITCAP - 1, LITCAP, LITCAP + 1, 700):
        add("%d literals" % n, Stream().fixed(lits(rand(n, 50 + n)), final=True))
    add("long match after %d literals" % LITCAP, Stream().fixed(lits(rand(LITCAP, 60)) + [(100, 7), (0, 5)], final=True))
    add("long match after %d matches" % NDESC, Stream().fixed(four + [(3, 2)] * NDESC + [(200, 5), (0, 5)], final=True))
    add("stored after %d literals" % LITCAP, Stream().fixed(lits(rand(LITCAP, 61))).stored(rand(50, 62)).fixed(lits(b"z"), final=True))
    add("stored after %d matches" % NDESC, Stream().fixed(four + [(3, 2)] * NDESC).stored(rand(50, 63), final=True))

    # ---- block structure: a block of each type at each of the eight bit positions (k one-bit literals in front)
    tk = lits(b"hello ") + [(6, 6), (3, 1)]
    dyn_ll, dyn_d = D.lens_for(tk)
    for k in range(8):
        add("stored at shift %d" % k, D.shifted(k, lambda s: s.stored(b"stored!", final=True)))
        add("fixed at shift %d" % k, D.shifted(k, lambda s: s.fixed(tk, final=True)))
        add("dynamic at shift %d" % k, D.shifted(k, lambda s: s.dynamic(tk, dyn_ll, dyn_d, final=True)))
    empties = {"fixed": lambda s, f: s.fixed([], final=f), "dynamic": lambda s, f: s.dynamic([], final=f),
               "stored": lambda s, f: s.stored(b"", final=f)}
    for kind, put in empties.items():
        add("empty %s block mid-stream" % kind, put(Stream().fixed(lits(b"ab")), False).fixed(lits(b"cd"), final=True))
        add("empty %s block last" % kind, put(Stream().fixed(lits(b"ab")), True))
        add("empty %s block alone" % kind, put(Stream(), True))
        add("empty %s block first" % kind, put(Stream(), False).fixed(lits(b"cd"), final=True))
    add("stored 1", Stream().stored(b"A").fixed(lits(b"b"), final=True))
    add("stored 65535", Stream().stored(rand(65535, 64)).fixed(lits(b"b") + [(4, 65535 - 40000)], final=True))
    add("stored last", Stream().fixed(lits(b"abc")).stored(rand(100, 65), final=True))          # (its data ends on the input's last byte)
    s = Stream()
    for i in range(300):
        last = i == 299
        s.fixed([(0, i & 255)], final=last) if i % 2 == 0 else s.dynamic([(0, i & 255)], final=last)
    add("300 blocks", s)

    # ---- dynamic headers
    # HCLEN 4 gives lengths to 16, 17, 18 and 0 alone, so every code it can describe is empty: that case is in family B.  5 is the
    # least that can name a length (8): 256 eight-bit codes
    l8 = [0] + [8] * 256
    add("hclen 5", Stream().dynamic(lits(b"\x01\x80\xff"), l8, [0], final=True, rle=D.greedy_rle, cl_lens=[2 if v in (0, 8, 16, 18) else 0 for v in range(19)],
                                    hclen=5))
    assert D.ORDER[4] == 8
    assert D.ORDER[18] == 15
    add("hclen 19", Stream().dynamic(lits(text), ll_lit, [0], final=True, hclen=19))
    a, _ = D.lens_for(lits(b"abc"), nll=257)
    add("hlit 257", Stream().dynamic(lits(b"abc"), a, [0], final=True))
    a = D.complete_lens([0x61, 0x62, 256, 285], 286)
    add("hlit 286", Stream().dynamic(lits(b"ab") + [(258, 1)], a, [1, 1], final=True, rle=D.greedy_rle))
    add("hdist 1", Stream().dynamic(lits(b"ab") + [(5, 1)], None, [1], final=True))
    d30 = D.complete_lens([0, 29], 30)
    add("hdist 30", Stream().stored(r32).dynamic([(5, 1), (5, 32768), (0, 1)], None, d30, final=True, rle=D.greedy_rle))
    # a code-length code of lengths 1 .. 7, 7: an 18 and its extra bits are 14 bits
    ll = [6] * 10 + [7] * 30 + [8] * 100 + [9] * 111 + [0] * 5 + [9]
    assert D.kraft(ll) == 32768 and len(ll) == 257
    cl = [0] * 19
    for sym, v in ((8, 1), (9, 2), (7, 3), (6, 4), (16, 5), (17, 6), (1, 7), (18, 7)):
        cl[sym] = v
    add("code-length code 1..7,7", Stream().dynamic(lits(bytes(range(0, 250, 7))), ll, [1] + [0] * 28 + [1], final=True, rle=D.greedy_rle, cl_lens=cl))
    # a 16 behind a plain length, behind another 16, behind a 17 and behind an 18 (a zero in the last two); an 18 of 138
    rle = [(17, 0), (16, 0), (3, 0), (16, 0), (16, 0), (18, 127), (16, 3), (18, 88), (3, 0), (0, 0)]
    ll = D.expand_rle(rle)[:-1]
    assert len(ll) == 257 and D.kraft(ll) == 32768 and [i for i, v in enumerate(ll) if v] == list(range(6, 13)) + [256]
    add("16 after length, 16, 17, 18", Stream().dynamic(lits(bytes(range(6, 13)) * 2), ll, [0], final=True, rle=rle))
    # ... and with 10-bit codes alone, which are read from the sorted symbol table, not from the 9-bit one: a 16 behind an 18 that
    # repeated anything but a zero would put symbols 268 .. 273 into that table.  (Three codes of 10 bits: incomplete.)
    rle = [(18, 86), (10, 0), (10, 0), (18, 127), (18, 8), (10, 0), (18, 0), (16, 3), (0, 0)]
    ll = D.expand_rle(rle)[:-1]
    assert len(ll) == 274 and [i for i, v in enumerate(ll) if v] == [0x61, 0x62, 256]
    add("16 after 18, 10-bit codes", Stream().dynamic(lits(b"abba"), ll, [0], final=True, rle=rle), libz="libz refuses an incomplete literal/length code")
    # a 16 that is the first symbol of a 64-bit window of the code-length pass: 2-bit codes, m plain lengths in front of the 16
    # (m = 32 puts it at bit 64); every length is 6, so a repeat that took its value from anywhere else stands out
    ll = [6] * 63 + [0] * 193 + [6]
    cl2 = [2 if v in (0, 6, 16, 18) else 0 for v in range(19)]
    for m in list(range(1, 58)):
        rest = 63 - m
        reps = []
        while rest:
            k = rest if rest <= 6 else (6 if rest - 6 >= 3 else rest - 3)
            reps.append((16, k - 3)); rest -= k
        rle = [(6, 0)] * m + reps + [(18, 127), (18, 44), (6, 0), (0, 0)]
        assert D.expand_rle(rle) == ll + [0], m
        s = Stream().dynamic(lits(bytes(range(0, 63, 5))), ll, [0], final=True, rle=rle, cl_lens=cl2)
        assert m != 32 or (rle[32][0] == 16 and s.rle_at[32] - s.clens_at == 64)      # the second window's first bit
        add("16 behind %d lengths" % m, s)
    for k in range(0, 64):                                        # ... and the header at every bit offset of such a window
        rle = [(6, 0)] * 32 + [(16, 3)] * 5 + [(6, 0)] + [(18, 127), (18, 44), (6, 0), (0, 0)]
        add("16 at bit 64, header shifted %d" % k, D.shifted(k, lambda s: s.dynamic(lits(b"\x00\x3e\x1f"), ll, [0], final=True, rle=rle, cl_lens=cl2)))
    # a 16 and an 18 that cross the boundary between the lit/len and the distance lengths; a repeat that ends on HLIT + HDIST
    ll = [0] * 254 + [2, 2, 2, 2]                                 # 254, 255, 256, 257 (length 3): a complete code of four
    rle = [(18, 127), (18, 105), (2, 0), (2, 0), (16, 2)]         # 254 255; 256 257 + distance 0 1 2: the 16 crosses the boundary
    full = D.expand_rle(rle)
    assert full[:258] == ll and full[258:] == [2, 2, 2] and len(full) == 261
    add("16 across hlit", Stream().dynamic([(0, 254), (0, 255), (3, 1), (3, 2), (3, 3)], ll, [2, 2, 2], final=True, rle=rle),
        libz="the distance code 2, 2, 2 is incomplete")
    rle = [(18, 127), (18, 105), (2, 0), (2, 0), (16, 3)]         # ... onto a fourth distance length: complete, and the repeat ends the list
    assert len(D.expand_rle(rle)) == 262
    add("16 across hlit, ends the list", Stream().dynamic([(0, 254), (0, 255), (3, 1), (3, 2), (3, 4)], ll, [2, 2, 2, 2], final=True, rle=rle))
    ll = [0] * 254 + [2, 2, 2, 2, 0, 0, 0]                        # HLIT 261, then distance lengths 0 x 9, 1, 1
    rle = [(18, 127), (18, 105), (2, 0), (16, 0), (18, 1), (1, 0), (1, 0)]      # the 18 of 12 covers 258 .. 260 and distances 0 .. 8
    full = D.expand_rle(rle)
    assert full[:261] == ll and full[261:] == [0] * 9 + [1, 1]
    add("18 across hlit", Stream().stored(r32[:60]).dynamic([(0, 254), (3, 33), (3, 25)], ll, [0] * 9 + [1, 1], final=True, rle=rle))
    rle = [(18, 127), (18, 105), (2, 0), (16, 0), (1, 0), (18, 0)]              # distances 1, then eleven zeros: the 18 ends the list
    add("18 ends the list", Stream().dynamic([(0, 254), (0, 255), (3, 1)], ll[:258], [1] + [0] * 11, final=True, rle=rle))
    # no distance code at all, HDIST 1 and 30; one 1-bit distance code that is used
    add("no distance code, hdist 1", Stream().dynamic(lits(b"only literals"), None, [0], final=True))
    add("no distance code, hdist 30", Stream().dynamic(lits(b"only literals"), None, [0] * 30, final=True, rle=D.greedy_rle))
    add("one distance code of 1 bit", Stream().dynamic(lits(b"ab") + [(10, 1), (0, 0x62), (4, 1)], None, [1], final=True))
    add("one distance code of 1 bit, symbol 5", Stream().dynamic(lits(b"abcdefgh") + [(10, 8), (4, 7)], None, [0, 0, 0, 0, 0, 1], final=True))
    # incomplete lit/len codes whose missing codes never occur: libz refuses them, the reference's construct (:98-103) only refuses
    # over-subscription
    ll = [0] * 257
    ll[0x61] = ll[0x62] = ll[256] = 2
    add("incomplete ll code", Stream().dynamic(lits(b"abba"), ll, [0], final=True), libz="libz refuses an incomplete literal/length code")
    ll = [0] * 257
    ll[256] = 1
    # (libz None: its versions differ on a code of one 1-bit end of block, so it is not asked)
    add("only a 1-bit end of block", Stream().dynamic([], ll, [0], final=True), libz=None)
    add("only a 1-bit end of block, mid-stream", Stream().fixed(lits(b"a")).dynamic([], ll, [0]).fixed(lits(b"b"), final=True), libz=None)

    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    _valid = cs
    return cs


# The valid cases k_inflate3 hands back to the second pass by design: {name: the line of k_inflate3.hip that does it}.  No other
# valid case may be handed back; the set does not grow to make a failure pass.  It is empty: the one hand-back by design that is
# no error, `r == 2` in P_BUILD (an empty lit/len or code-length code), has no end-of-block code, so the reference refuses what
# follows it too (family B: "hclen 4", "ll code all zero", "code-length code all zero"); an incomplete code is not handed back.
FIRST_PASS_HANDS_BACK = {}


# ---- the position sweep: one stream of ~3 KiB -- more than two 8192-bit tiles, more than two stagings of CB bytes -- of 2-bit
# literals and 48-bit matches, behind k one-bit literals: a symbol lies across every bit of a 128-bit segment, across the tiles' edges
# and across the staged buffer's end
_sweep_body = None


def _sweep_tokens():
    ll = ladder([285, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x6b, 0x6c, 0x6d, 281, 256], 286)
    d = ladder([12, 0, 1, 2, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 28, 29], 30)
    toks = lits(b"abcdefghijklm" * 6) + [(258, 78)] * 64          # 16590 bytes, none of them reaching in front of the block
    out = 78 + 64 * 258
    for i in range(440):
        toks += [(0, 0x61)] * (1 + i % 4)
        out += 1 + i % 4
        ln = 131 + (i * 7) % 32
        dist = 16385 + (i * 2731) % min(8192, out - 16384) if out < 24577 or i % 3 else 24577 + (i * 1237) % min(8192, out - 24576)
        assert dist <= out
        toks.append((ln, dist, 281, ln - 131))
        out += ln
    return toks, ll, d


def sweep(k):
    """the sweep's stream behind k one-bit literals -> a case as valid()'s"""
    global _sweep_body
    toks, ll, d = _sweep_tokens()
    s = D.shifted(k, lambda s: s.dynamic(toks, ll, d, final=True))
    if _sweep_body is None:
        _sweep_body = D.shifted(0, lambda s: s.dynamic(toks, ll, d, final=True)).expected()
    # (no distance of the body reaches in front of it, so the k literals in front change nothing in it)
    return {"name": "sweep %d" % k, "stream": s.bytes(), "want": b"a" * k + _sweep_body, "flags": 1 if k == 0 else 0, "libz": True}


SWEEP_ALL = tuple(range(128))
SWEEP_SIM = tuple(range(0, 128, 9))


# ---------------------------------------------------------------------------------------------------------------- family B: invalid
_invalid = None


def invalid():
    """[dict(name, stream, cap, status, line)]: status is the hand-stated one for this tail (None where the bytes behind a cut decide:
    the prefixes with a tail), line the place in src/flate.rs"""
    global _invalid
    if _invalid is not None:
        return _invalid
    cs = []

    def add(name, stream, status, line, cap=4096):
        """status: one for all three tails, or (nothing, zeros, ones)"""
        if isinstance(stream, Stream):
            stream = stream.bytes()
        for k, (tag, tail) in enumerate(TAILS):
            cs.append({"name": name + tag, "stream": stream + tail, "cap": cap, "status": status[k] if isinstance(status, tuple) else status, "line": line})

    RUNS_OUT = (E_EOF, E_NOT_ENOUGH_BITS, E_NOT_ENOUGH_BITS)      # a walk that finds no code: 15 bits, if the input has them (:129-146, :252)
    add("block type 3", b"\x07", E_BLOCK_CODE, ":203")
    s = Stream().fixed(lits(b"ab"))
    s.put(0, 1); s.put(3, 2)
    add("block type 3 behind a block", s, E_BLOCK_CODE, ":203")
    add("stored, nlen wrong", Stream().fixed(lits(b"ab")).stored(b"hello", final=True, nlen=0xfffb), E_STATIC_SIZE, ":240")
    add("stored, longer than the input", Stream().stored(b"0123456789", final=True, length=100), E_EOF, ":241 push_exactly")
    add("stored, longer than the slot", Stream().fixed(lits(b"ab")).stored(rand(100, 70), final=True), E_TOO_SMALL, ":241 push_exactly", cap=101)
    # HLIT / HDIST too large: the reference reads HCLEN before it checks
    for hl, hd in ((287, 1), (288, 1), (257, 31), (257, 32), (288, 32)):
        s = Stream().dynamic([], [0] * 257, [0], final=True, hlit=hl, hdist=hd, header_only=True)
        add("hlit %d hdist %d" % (hl, hd), s, E_TREE_TOO_LARGE, ":401")
        add("hlit %d hdist %d, cut in hclen" % (hl, hd), s.bytes()[:2], (E_EOF, E_TREE_TOO_LARGE, E_TREE_TOO_LARGE), ":400, :401")
    add("hclen 4", Stream().dynamic([], [0] * 257, [0], final=True, cl_lens=[2 if v in (0, 16, 17, 18) else 0 for v in range(19)], hclen=4,
                                    rle=[(18, 127), (18, 109)], header_only=True), RUNS_OUT, ":287 (an empty lit/len code)")
    over = [1, 1, 1] + [0] * 16
    add("code-length code over-subscribed", Stream().dynamic([], [0] * 257, [0], final=True, cl_lens=over, rle=[], header_only=True), E_TREE, ":415")
    add("code-length code all zero", Stream().dynamic([], [0] * 257, [0], final=True, cl_lens=[0] * 19, hclen=19, rle=[], header_only=True),
        RUNS_OUT, ":423")
    cl = [2 if v in (0, 2, 16, 18) else 0 for v in range(19)]
    add("16 first", Stream().dynamic([], None, None, final=True, cl_lens=cl, rle=[(16, 0), (2, 0)], header_only=True), E_HEADER_SYMBOL, ":428")
    inc = [0] * 19
    inc[0], inc[8] = 1, 2                                          # codes 0 and 10: no code begins 11
    add("code-length pattern without a code", Stream().dynamic([], None, None, final=True, cl_lens=inc, rle=[(8, 0), (0, 0), ("bits", (3, 2))],
                                                               header_only=True), RUNS_OUT, ":423")
    # a 16 that runs past the 316 entries the reference has (its index panic), against one past HLIT + HDIST only
    z316 = [(2, 0)] + [(16, 3)] * 52 + [(2, 0), (2, 0)]           # 315 entries
    assert len(D.expand_rle(z316)) == 315
    add("16 past entry 316", Stream().dynamic([], None, None, final=True, hlit=286, hdist=30, cl_lens=cl, rle=z316 + [(16, 0)], header_only=True),
        E_MALFORMED, ":432 index panic")
    add("16 past hlit+hdist", Stream().dynamic([], None, None, final=True, hlit=280, hdist=30, cl_lens=cl, rle=z316[:52] + [(2, 0), (16, 1)],
                                               header_only=True), E_TREE_HEADER, ":442")
    assert len(D.expand_rle(z316[:52] + [(2, 0), (16, 1)])) == 312                 # 308 entries, then four more: past 310, short of 316
    add("17 overshoots", Stream().dynamic([], None, None, final=True, hlit=257, hdist=1, cl_lens=[2 if v in (0, 2, 17, 18) else 0 for v in range(19)],
                                          rle=[(18, 127), (18, 106), (17, 1)], header_only=True), E_TREE_HEADER, ":442")
    add("18 overshoots", Stream().dynamic([], None, None, final=True, hlit=257, hdist=1, cl_lens=cl, rle=[(2, 0), (18, 127), (18, 109)], header_only=True),
        E_TREE_HEADER, ":442")
    ll = [0] * 257
    ll[0x61] = ll[0x62] = ll[256] = 1
    add("ll code over-subscribed", Stream().dynamic([], ll, [0], final=True, rle=D.greedy_rle, header_only=True), E_TREE, ":445-446")
    add("ll code all zero", Stream().dynamic([], [0] * 257, [1, 1], final=True, rle=D.greedy_rle, header_only=True), RUNS_OUT, ":287")
    ll = D.complete_lens([0x61, 0x62, 256, 257], 258)
    add("distance code over-subscribed", Stream().dynamic([], ll, [1, 1, 1], final=True, rle=D.greedy_rle, header_only=True), E_TREE, ":447-448")
    # no end-of-block code: two 1-bit literals, so zeros and ones behind the stream go on as literals until the input or the slot ends
    ll = [0] * 257
    ll[0x61] = ll[0x62] = 1
    add("no end of block", Stream().dynamic(lits(b"abba"), ll, [0], final=True, rle=D.greedy_rle, eob=False), E_EOF, ":252 (read_u8)", cap=4096)
    add("no end of block, small slot", Stream().dynamic(lits(b"abba"), ll, [0], final=True, rle=D.greedy_rle, eob=False),
        (E_EOF, E_TOO_SMALL, E_TOO_SMALL), ":252 / the slot", cap=100)
    ll = [0] * 257
    ll[0x61] = ll[0x62] = ll[256] = 2                              # codes 00 01 10: nothing begins 11
    add("ll pattern without a code", Stream().dynamic(lits(b"ab") + [("bits", 3, 2)], ll, [0], final=True, rle=D.greedy_rle, eob=False), RUNS_OUT, ":287")
    ll = D.complete_lens([0x61, 0x62, 256, 257], 258)
    add("length with an empty distance code", Stream().dynamic(lits(b"ab") + [("sym", 257)], ll, [0], final=True, rle=D.greedy_rle, eob=False),
        RUNS_OUT, ":302")
    add("fixed 286", Stream().fixed(lits(b"a") + [("sym", 286)], final=True, eob=False), E_MALFORMED, ":297 index panic")
    add("fixed 287", Stream().fixed(lits(b"a") + [("sym", 287)], final=True, eob=False), E_CODE, ":294")
    for dsy in (30, 31):
        add("fixed distance %d" % dsy, Stream().fixed(lits(b"a") + [("sym", 257), ("dsym", dsy)], final=True, eob=False), RUNS_OUT, ":302")
    add("distance = output so far + 1", Stream().fixed(lits(b"abcde") + [(4, 6)], final=True), E_CODE, ":314")
    add("distance at position 0", Stream().fixed([(4, 1)], final=True), E_CODE, ":314")
    add("32768 at 32767", Stream().stored(rand(32767, 71)).fixed([(4, 32768)], final=True), E_CODE, ":314", cap=40000)
    # the slot
    add("literal at the capacity", Stream().fixed(lits(b"abcdef"), final=True), E_TOO_SMALL, ":289 the slot", cap=5)
    add("match across the capacity", Stream().fixed(lits(b"abc") + [(20, 3), (0, 1)], final=True), E_TOO_SMALL, ":320 the slot", cap=22)
    add("long match across the capacity", Stream().fixed(lits(b"abc") + [(200, 3), (0, 1)], final=True), E_TOO_SMALL, ":320 the slot", cap=150)
    add("stored across the capacity", Stream().fixed(lits(b"abc")).stored(rand(30, 72), final=True), E_TOO_SMALL, ":241 the slot", cap=32)
    add("capacity 0", Stream().fixed(lits(b"a"), final=True), E_TOO_SMALL, ":289 the slot", cap=0)
    add("capacity 0, stored", Stream().stored(b"a", final=True), E_TOO_SMALL, ":241 the slot", cap=0)
    # every byte prefix of twelve small valid streams: the input runs out (:252 read_u8); with a tail the bytes behind the cut decide,
    # and the oracle alone says what
    by = {c["name"]: c for c in valid()}
    for name in PREFIXED:
        st = by[name]["stream"]
        assert len(st) <= 120, (name, len(st))
        for n in range(len(st)):
            for k, (tag, tail) in enumerate(TAILS):
                cs.append({"name": "%s [:%d]%s" % (name, n, tag), "stream": st[:n] + tail, "cap": len(by[name]["want"]) + 700,
                           "status": E_EOF if k == 0 else None, "line": ":252"})
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    _invalid = cs
    return cs


PREFIXED = ("stored at shift 3", "stored last", "fixed at shift 0", "fixed at shift 5", "dynamic at shift 2", "long codes, repeats in the header",
            "16 after length, 16, 17, 18", "16 behind 32 lengths", "code-length code 1..7,7", "18 across hlit", "hdist 1",
            "empty dynamic block mid-stream")
FRAMED = ("dynamic at shift 2", "long distance codes", "stored last")


def framed():
    """[dict(name, kind ("zlib" | "gzip"), stream, want, status)]: three valid streams in zlib and gzip framing, right and wrong"""
    by = {c["name"]: c for c in valid()}
    out = []
    for name in FRAMED:
        c = by[name]
        raw, want = c["stream"], c["want"]
        ad = zlib.adler32(want)
        out.append({"name": name + " zlib", "kind": "zlib", "stream": b"\x78\x9c" + raw + struct.pack(">I", ad), "want": want, "status": 0})
        out.append({"name": name + " zlib, wrong adler", "kind": "zlib", "stream": b"\x78\x9c" + raw + struct.pack(">I", ad ^ 0x10000), "want": want,
                    "status": E_ZLIB_CHECKSUM})
        hdr = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"
        crc, n = zlib.crc32(want), len(want)
        out.append({"name": name + " gzip", "kind": "gzip", "stream": hdr + raw + struct.pack("<II", crc, n), "want": want, "status": 0})
        out.append({"name": name + " gzip, wrong crc", "kind": "gzip", "stream": hdr + raw + struct.pack("<II", crc ^ 1, n), "want": want, "status": E_GZIP_CRC})
        out.append({"name": name + " gzip, wrong isize", "kind": "gzip", "stream": hdr + raw + struct.pack("<II", crc, n + 1), "want": want,
                    "status": E_GZIP_ISIZE})
    return out


# ------------------------------------------------------------------------------------------------------------- the table as one batch
_tables = {}


def table(oracle, sweeps=SWEEP_ALL, prefix_step=1):
    """[dict(name, stream, cap, valid, ref = the oracle's (status, bytes, in_used, flags))] of both families and the sweep's shifts.
    A valid case's slot is exactly its output.  prefix_step: every how-manieth prefix (the simulator's share)."""
    key = (tuple(sweeps), prefix_step)
    if key in _tables:
        return _tables[key]
    rows = [{"name": c["name"], "stream": c["stream"], "cap": len(c["want"]), "valid": True, "want": c["want"]}
            for c in valid() + [sweep(k) for k in sweeps]]
    npre = 0
    for c in invalid():
        if " [:" in c["name"]:
            npre += 1
            if (npre // 3) % prefix_step:
                continue
        rows.append({"name": c["name"], "stream": c["stream"], "cap": c["cap"], "valid": False})
    for r in rows:
        out, used, flags, st = oracle.inflate(r["stream"], cap=r["cap"], raise_on_error=False)
        r["ref"] = (st, out, used, flags)
        assert not r["valid"] or (st, out, used) == (0, r["want"], len(r["stream"])), r["name"]
    _tables[key] = rows
    return rows


def mismatches(rows, st, out_len, in_used, flags, outs, ref=None):
    """the names of the rows whose results differ from the reference (ref[i], default the rows' own): status, out_len, the bytes (so
    far, where the stream fails), in_used and flags"""
    bad = []
    for i, r in enumerate(rows):
        es, eo, eu, ef = ref[i] if ref is not None else r["ref"]
        got = (int(st[i]), int(out_len[i]), outs[i], int(in_used[i]), int(flags[i]))
        if got != (es, len(eo), eo, eu, ef):
            bad.append((r["name"], got[0], got[1], got[3], got[4], "want", es, len(eo), eu, ef))
    return bad


def check_first_pass(rows, st, out_len, in_used, flags, outs):
    """k_inflate3 alone (variants 12 and 10): every status is 0 or the hand-back; 0 only with the reference's results; what the
    reference refuses is handed back; what it takes is accepted, FIRST_PASS_HANDS_BACK apart -- so the simulator's accepted set and
    the device's are the same set, or one of the two fails here"""
    other = [(r["name"], int(s)) for r, s in zip(rows, st) if int(s) not in (0, ST_FALLBACK)]
    assert not other, other[:6]
    acc = [i for i, s in enumerate(st) if int(s) == 0]
    pick = lambda a: [a[i] for i in acc]
    bad = mismatches(pick(rows), pick(st), pick(out_len), pick(in_used), pick(flags), pick(outs))
    assert not bad, (len(bad), bad[:6])
    handed = {r["name"] for r, s in zip(rows, st) if int(s) != 0 and r["ref"][0] == 0}
    assert handed == set(FIRST_PASS_HANDS_BACK), sorted(handed ^ set(FIRST_PASS_HANDS_BACK))[:8]


GZIP_HEAD = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def behind_history(oracle, rows, hist):
    """the reference for every row's stream behind `hist`: the oracle on non-final stored blocks holding hist (they end on a byte
    boundary), then the stream -- less the history in out_len and the bytes, less the stored blocks in in_used"""
    front = b"".join(Stream().stored(hist[a:a + 65535]).bytes() for a in range(0, len(hist), 65535))
    ref = []
    for r in rows:
        out, used, flags, st = oracle.inflate(front + r["stream"], cap=len(hist) + r["cap"], raise_on_error=False)
        assert len(out) >= len(hist) and used >= len(front)
        ref.append((st, out[len(hist):], used - len(front), flags))
    return ref


def into_history(hist):
    """[(name, stream, cap, the token model's bytes behind hist)]: the distances that point in front of the stream, which a history
    makes valid"""
    out = []
    for name, s in (("distance = output so far + 1", Stream().fixed(lits(b"abcde") + [(4, 6)], final=True)),
                    ("distance at position 0", Stream().fixed([(4, 1)], final=True)),
                    ("distance %d at position 2" % len(hist), Stream().fixed(lits(b"ab") + [(9, len(hist)), (0, 1), (70, len(hist))], final=True))):
        want = s.expected(hist)
        out.append((name, s.bytes(), len(want), want))
    return out
