"""Stage access and plain references for the two high-compression encoders (TEST INFRASTRUCTURE, shared by
test_wavesim_deflate_stages.py, test_wavesim_lz4hc_stages.py and test_gpu_hc_stages.py).  The stage arrays (chains, candidates, prices, arrivals, parses, match lists) live in the encoders' scratch;
their offsets come from the kernels' own carve functions through tests/sim_*_run.layout.  The references are tests/hc_ref/hc_ref.cpp
(serial C++, built here with g++) and the plain Python below, written from the definitions in the kernels' header comments."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(HERE, "hc_ref", "build", "libhc_ref.so")
SEG = 65536
DE_WIN, HC_WIN = 32768, 65535
DH_RING, HC_RING = 512, 2048
HC_MAXM = HC_RING - 64
HC_TOKCAP = 16384
ELEN = SEG + 64                         # entries of a segment's arrival record, both encoders
# chain depth per level, restated (a changed table in the kernels is noticed: the search would differ from the reference)
DH_DEPTH = {2: 4, 3: 8, 4: 16, 5: 32, 6: 64, 7: 96, 8: 160, 9: 256}
HC_DEPTH = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 8, 7: 12, 8: 16, 9: 24, 10: 64, 11: 128, 12: 256}
_ref = None


def ref():
    global _ref
    if _ref is None:
        src = os.path.join(HERE, "hc_ref", "hc_ref.cpp")
        if not (os.path.exists(REF_OUT) and os.path.getmtime(REF_OUT) >= os.path.getmtime(src)):
            os.makedirs(os.path.dirname(REF_OUT), exist_ok=True)
            tmp = REF_OUT + ".%d" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-o", tmp, src])
            os.replace(tmp, REF_OUT)
        _ref = C.CDLL(REF_OUT)
        _ref.ref_deflate_min_cost.restype = C.c_uint64
        _ref.ref_lz4_min_cost.restype = C.c_uint64
        _ref.ref_lz4_greedy_size.restype = C.c_uint64
    return _ref


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _bytes(raw):
    return np.frombuffer(bytes(raw) + b"\0" * 8, np.uint8)      # (the references read in[0..n) only)


def ref_links(raw, win):
    link, inb = np.zeros(max(len(raw), 1), np.uint16), _bytes(raw)
    ref().ref_links(_p(inb), C.c_uint64(len(raw)), C.c_uint32(win), _p(link))
    return link[:len(raw)]


def ref_search(raw, link, win, depth, lz4):
    cand, inb = np.zeros(max(len(raw), 1), np.uint32), _bytes(raw)
    link = np.ascontiguousarray(link, np.uint16)
    ref().ref_search(_p(inb), C.c_uint64(len(raw)), _p(link), C.c_uint32(win), C.c_uint32(depth), int(lz4),
                     C.c_uint32(HC_MAXM if lz4 else 258), _p(cand))
    return cand[:len(raw)]


def ref_deflate_min_cost(seg, cand, price):
    cand = np.ascontiguousarray(cand, np.uint32)
    price, inb = np.ascontiguousarray(price, np.uint8), _bytes(seg)
    return int(ref().ref_deflate_min_cost(_p(inb), C.c_uint32(len(seg)), _p(cand), _p(price)))


def ref_lz4_min_cost(L, cand):
    cand = np.ascontiguousarray(cand, np.uint32)
    return int(ref().ref_lz4_min_cost(C.c_uint32(L), _p(cand)))


def ref_lz4_greedy_size(n, cand):
    cand = np.ascontiguousarray(np.concatenate([cand, [0]]), np.uint32)
    return int(ref().ref_lz4_greedy_size(C.c_uint64(n), _p(cand)))


# ------------------------------------------------------------------------------------------------------------ views of a scratch

def _arr(scratch, off, dtype, count):
    return np.frombuffer(scratch, dtype, count, off) if count else np.zeros(0, dtype)


def deflate_views(raws, scratch, lay, copy=False):
    """Per stream: the stage arrays of a DEFLATE level scratch (a uint8 array, lay = sim_deflate_hc_run.layout of it).  link, cand
    and pos per position of the stream; elen [segments][ELEN]; price [segments][320]; seg_type, seg_bits [segments]."""
    n = len(raws)
    first = _arr(scratch, lay["seg_first"], np.uint32, n + 1)
    views = []
    for b, r in enumerate(raws):
        f0, ns, ln = int(first[b]), (len(r) + SEG - 1) // SEG, len(r)
        assert int(first[b + 1]) - f0 == ns and f0 + ns <= lay["cap"]
        v = {"link": _arr(scratch, lay["link"] + 2 * f0 * SEG, np.uint16, ln),
             "cand": _arr(scratch, lay["cand"] + 4 * f0 * SEG, np.uint32, ln),
             "pos": _arr(scratch, lay["pos"] + 4 * f0 * SEG, np.uint32, ln),
             "elen": _arr(scratch, lay["elen"] + 4 * f0 * ELEN, np.uint32, ns * ELEN).reshape(ns, ELEN),
             "price": _arr(scratch, lay["price"] + 320 * f0, np.uint8, ns * 320).reshape(ns, 320),
             "seg_type": _arr(scratch, lay["seg_type"] + 4 * f0, np.uint32, ns),
             "seg_bits": _arr(scratch, lay["seg_bits"] + 4 * f0, np.uint32, ns)}
        views.append({k: a.copy() for k, a in v.items()} if copy else v)
    return views


def lz4_views(raws, scratch, lay, copy=False):
    """Per block: the stage arrays of an LZ4 HC scratch.  link and cand per position of the block (cand: as k_hc_search left it, valid
    only before k_hc_parse ran); elen [segments][ELEN]; toks: per segment the match list k_hc_parse wrote over cand, as (start in the
    segment, length, distance) rows (valid only after it ran); seg_nm, seg_fm, seg_le [segments]."""
    n = len(raws)
    first = _arr(scratch, lay["seg_first"], np.uint32, n + 1)
    views = []
    for b, r in enumerate(raws):
        f0, ns, ln = int(first[b]), (len(r) + SEG - 1) // SEG, len(r)
        assert int(first[b + 1]) - f0 == ns and f0 + ns <= lay["cap"]
        v = {"link": _arr(scratch, lay["link"] + 2 * f0 * SEG, np.uint16, ln),
             "cand": _arr(scratch, lay["cand"] + 4 * f0 * SEG, np.uint32, ln),
             "elen": _arr(scratch, lay["elen"] + 4 * f0 * ELEN, np.uint32, ns * ELEN).reshape(ns, ELEN),
             "seg_nm": _arr(scratch, lay["seg_nm"] + 4 * f0, np.uint32, ns),
             "seg_fm": _arr(scratch, lay["seg_fm"] + 4 * f0, np.uint32, ns),
             "seg_le": _arr(scratch, lay["seg_le"] + 4 * f0, np.uint32, ns)}
        toks = []
        for s in range(ns):
            nm = min(int(v["seg_nm"][s]), HC_TOKCAP)
            t = _arr(scratch, lay["cand"] + 4 * (f0 + s) * SEG + 8 * (HC_TOKCAP - nm), np.uint64, nm)
            toks.append(np.stack([t & 0xFFFF, (t >> 16) & 0xFFFF, t >> 32], 1).astype(np.int64) if nm else np.zeros((0, 3), np.int64))
        v = {k: a.copy() for k, a in v.items()} if copy else v
        v["toks"] = toks
        views.append(v)
    return views


def deflate_reduce(raws, res):
    """what a simulator worker sends back of sim_deflate_hc_run.stages: (rc, outputs, status, views)"""
    rc, outs, st, scratch, lay = res
    return rc, outs, st, deflate_views(raws, scratch, lay, copy=True) if rc == 0 else None


def lz4_reduce(raws, res):
    rc, outs, st, scratch, lay = res
    return rc, outs, st, lz4_views(raws, scratch, lay, copy=True) if rc == 0 else None


# ------------------------------------------------------------------------------------------------------------ RFC 1951, in Python

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_SYM = [0] * 259                     # length -> index into LBASE (symbol 257 + index)
for _i, _b in enumerate(LBASE):
    for _l in range(_b, 259):
        LEN_SYM[_l] = _i
DIST_SYM = np.zeros(32769, np.int64)    # distance -> symbol
for _i, _b in enumerate(DBASE):
    DIST_SYM[_b:] = _i
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.p = 0
        self.n = 8 * len(data)

    def get(self, k):
        assert self.p + k <= self.n, "the stream ends inside a block"
        x = (self.v >> self.p) & ((1 << k) - 1)
        self.p += k
        return x


def _decoder(lengths):
    """canonical Huffman code of RFC 1951 3.2.2 -> {(length, code): symbol}"""
    code, table = 0, {}
    for ln in range(1, 16):
        for sym, l in enumerate(lengths):
            if l == ln:
                table[(ln, code)] = sym
                code += 1
        code <<= 1
    return table


def _sym(bits, table):
    code = 0
    for ln in range(1, 16):
        code = code << 1 | bits.get(1)              # (Huffman codes are packed from their most significant bit)
        if (ln, code) in table:
            return table[(ln, code)]
    raise AssertionError("no such code")


def inflate_tokens(data):
    """A token-level inflate of a raw DEFLATE stream.  -> a list of blocks, each a dict: final, type, bits (the block's length in bits,
    header and end-of-block symbol included, for a stored block the padding and LEN/NLEN too), tokens ((0, byte) literals and
    (length, distance) matches; a stored block's bytes as literals), and for type 2 the code lengths ll, dl."""
    bits, blocks = _Bits(data), []
    while True:
        start = bits.p
        final, typ = bits.get(1), bits.get(2)
        blk = {"final": final, "type": typ, "tokens": []}
        assert typ != 3
        if typ == 0:
            bits.p = (bits.p + 7) & ~7
            ln, nln = bits.get(16), bits.get(16)
            assert ln == nln ^ 0xFFFF
            blk["tokens"] = [(0, bits.get(8)) for _ in range(ln)]
        else:
            if typ == 1:
                ll, dl = FIXED_LL, [5] * 30
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.get(3)
                ct, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _sym(bits, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                blk["ll"], blk["dl"] = ll, dl
            lt, dt = _decoder(ll), _decoder(dl)
            while True:
                s = _sym(bits, lt)
                if s < 256:
                    blk["tokens"].append((0, s))
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    ln = LBASE[s - 257] + bits.get(LEXTRA[s - 257])
                    ds = _sym(bits, dt)
                    assert ds <= 29
                    blk["tokens"].append((ln, DBASE[ds] + bits.get(DEXTRA[ds])))
        blk["bits"] = bits.p - start
        blocks.append(blk)
        if final:
            assert bits.n - bits.p < 8, "bytes after the final block"
            return blocks


def fixed_cost(tokens):
    """the exact bits of a fixed-Huffman block (type 1) of these tokens: header, tokens, end-of-block symbol"""
    c = 3 + FIXED_LL[256]
    for ln, x in tokens:
        if ln == 0:
            c += FIXED_LL[x]
        else:
            c += FIXED_LL[257 + LEN_SYM[ln]] + LEXTRA[LEN_SYM[ln]] + 5 + DEXTRA[int(DIST_SYM[x])]
    return c


def walk(pos, L):
    """the parse p += max(1, pos[p] >> 16) from 0 -> the token starts (it must land on L exactly)"""
    starts, p = [], 0
    while p < L:
        starts.append(p)
        p += max(1, int(pos[p]) >> 16)
    assert p == L, "the parse ends at %d, the segment at %d" % (p, L)
    return starts


def parse_tokens(seg, pos):
    """the walk of pos over the segment's bytes as inflate_tokens lists them"""
    return [(int(pos[p]) >> 16, (int(pos[p]) & 0xFFFF) + 1) if pos[p] else (0, seg[p]) for p in walk(pos, len(seg))]


def parse_cost(seg, pos, price):
    """bits of the walk of pos under price[320] (the end-of-block symbol aside, as the parse counts)"""
    c = 0
    for p in walk(pos, len(seg)):
        m = int(pos[p])
        if m:
            ls, ds = LEN_SYM[m >> 16], int(DIST_SYM[(m & 0xFFFF) + 1])
            c += int(price[257 + ls]) + LEXTRA[ls] + int(price[288 + ds]) + DEXTRA[ds]
        else:
            c += int(price[seg[p]])
    return c


def histogram(seg, src):
    """literal/length [288] and distance [32] counts of the walk of src (cand or pos) over the segment, the end-of-block symbol once"""
    f = np.zeros(320, np.int64)
    for p in walk(src, len(seg)):
        m = int(src[p])
        if m:
            f[257 + LEN_SYM[m >> 16]] += 1
            f[288 + int(DIST_SYM[(m & 0xFFFF) + 1])] += 1
        else:
            f[seg[p]] += 1
    f[256] += 1
    return f


def check_prices(price, freq, where):
    """the price table k_dh_price derives from a parse's histogram: every symbol 0..285 and distance 0..29 priced 1..15, the others 0,
    both codes complete (Kraft with equality), and no symbol seen more often than another priced higher"""
    for lo, n, tot in ((0, 286, 288), (288, 30, 32)):
        ln = price[lo:lo + n].astype(np.int64)
        assert ln.min() >= 1 and ln.max() <= 15, where
        assert not price[lo + n:lo + tot].any(), where
        assert int((1 << (15 - ln)).sum()) == 1 << 15, (where, "Kraft")
        f = freq[lo:lo + n]
        order = np.lexsort((ln, f))                 # by frequency, then by length
        # across strictly increasing frequency the length never increases: the longest length of a frequency class is at most the
        # shortest of every rarer class
        fs, ls = f[order], ln[order]
        cls = np.flatnonzero(np.diff(fs)) + 1
        mins = np.minimum.reduceat(ls, np.concatenate([[0], cls]))
        maxs = np.maximum.reduceat(ls, np.concatenate([[0], cls]))
        assert (maxs[1:] <= np.minimum.accumulate(mins)[:-1]).all(), (where, "a more frequent symbol is priced higher")


def check_deflate_parse(seg, cand, pos, price, where):
    """(a) pos walks from 0 to the segment's end exactly and every match token is a prefix (3 bytes at least) of the candidate at its
    start, at the candidate's distance; (b) its cost equals the minimum over all such parses.  -> (cost, minimum)"""
    L = len(seg)
    for p in walk(pos, L):
        m = int(pos[p])
        if m:
            c = int(cand[p])
            assert c and 3 <= (m >> 16) <= (c >> 16) and (m & 0xFFFF) == (c & 0xFFFF), (where, p, hex(m), hex(c))
    got, want = parse_cost(seg, pos, price), ref_deflate_min_cost(seg, cand, price)
    assert got == want, (where, "parse costs %d bits, the minimum is %d" % (got, want))
    return got, want


# ------------------------------------------------------------------------------------------------------------ LZ4

def mext(l):
    """length bytes of a match of l bytes"""
    return 1 + (l - 19) // 255 if l >= 19 else 0


def lext(r):
    """length bytes of a run of r literals"""
    return 1 + (r - 15) // 255 if r >= 15 else 0


def lz4_block_tokens(blk):
    """the sequences of an LZ4 block as (literals, match start, match length, distance) rows; the final one (literals, end, 0, 0)"""
    p, out, toks = 0, 0, []
    while True:
        tok = blk[p]
        p += 1
        r = tok >> 4
        if r == 15:
            while True:
                b = blk[p]
                p += 1
                r += b
                if b != 255:
                    break
        p += r
        out += r
        if p == len(blk):
            toks.append((r, out, 0, 0))
            return toks
        off = blk[p] | blk[p + 1] << 8
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = blk[p]
                p += 1
                ml += b
                if b != 255:
                    break
        toks.append((r, out, ml + 4, off))
        out += ml + 4


def lz4_pieces(elen, L):
    """the parse of a segment before adjacent pieces are joined, read from the arrival record: elen[q] = the length of the edge that
    arrives at q | its distance << 16 (1: a literal) -> (start, length, distance) rows in order"""
    q, pieces = L, []
    while q > 0:
        e = int(elen[q])
        el = e & 0xFFFF
        assert 1 <= el <= q, (q, hex(e))
        if el > 1:
            pieces.append((q - el, el, e >> 16))
        q -= el
    return pieces[::-1]


def check_lz4_parse(L, cand, elen, toks, where):
    """(a) Validity of a segment's match list (toks rows: start, length, distance) against the search's candidates: the arrivals walk
    from the segment's end to 0; every piece is a prefix (4 bytes at least) of the candidate at its start, at its distance, inside the
    segment; the list is the pieces in order with adjacent pieces of one distance joined while the sum stays below 2^16.
    -> (pieces, bytes the joins save)"""
    pieces = lz4_pieces(elen, L)
    for st, el, d in pieces:
        c = int(cand[st])
        assert 4 <= el <= min(c >> 16, L - st, HC_MAXM) and d == c & 0xFFFF and 1 <= d, (where, st, el, d, hex(c))
    # join from the end, as the kernel's header says: a match that ends where the next starts, at the same distance
    joined, saved = [], 0
    for st, el, d in pieces[::-1]:
        if joined and st + el == joined[-1][0] and d == joined[-1][2] and joined[-1][1] + el <= 0xFFFF:
            nl = joined[-1][1]
            saved += 3 + mext(el) + mext(nl) - mext(nl + el)
            joined[-1] = (st, nl + el, d)
        else:
            joined.append((st, el, d))
    joined = joined[::-1]
    assert len(joined) <= HC_TOKCAP and [tuple(int(x) for x in t) for t in toks] == joined, (where, len(toks), len(joined))
    for (s0, l0, _), (s1, _, _) in zip(joined, joined[1:]):
        assert s0 + l0 <= s1, where
    assert all(l < 1 << 16 for _, l, _ in joined), where
    return pieces, saved


def pack(raws, lead):
    """the input buffer the simulator drivers' stages() build: `lead` bytes of padding before every stream -> (bytes, offsets)"""
    buf, offs = bytearray(), []
    for r in raws:
        buf += b"\xC3" * lead
        offs.append(len(buf))
        buf += r
    return bytes(buf) + b"\0" * 16, offs
