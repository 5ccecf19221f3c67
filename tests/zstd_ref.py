"""A plain-Python Zstandard decoder, written from the format (RFC 8878): the oracle that travels with the tests, because neither this
Python nor the GPU machine need have a Zstandard module.  Where libzstd is found (tests/test_zstd_ref.py) it is checked against
libzstd 1.4.8, whose accept / reject it follows where that differs from the RFC; DESIGN.md 3.22 lists those places and the three where
this decoder and the kernel are stricter than libzstd.

decode(blob, dictionary=b"", cap=None) -> (bytes, in_used) for one whole file (concatenated frames, skippable frames skipped, trailing
bytes that are no magic left alone), or raises ZstdRefError with .status, the name of the rcx status.  Slow and simple on purpose: a
bitstream is one Python integer.  Also xxh64().

decode(trace=[]) appends what the file reaches: ("frame", ...), ("block", type, size), ("lit", ...), ("nseq", ...), ("modes", ...) and
one-word entries for the paths the kernel has a branch for -- lithdr{1,2,3}_{raw,rle}, hufhdr{3,4,5}, lit_full, rep{1,2,3} and
rep{1,2,3}_ll0 (offset_value 1, 2, 3 behind literals and behind none; rep3_ll0 is rep0 - 1), zero_as_1, ll_bits>=8, ml_bits>=14,
of_code>=20, far, overlap, dict, dict_straddle, frame2_compressed, weights_end_state{1,2}.  tests/zstd_cases.props turns a trace into a
set of words."""

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 * 1024
M64 = (1 << 64) - 1

STATUS = {"OK": 0, "E_EOF": 1, "E_OUTPUT_TOO_SMALL": 2, "E_ZSTD_MAGIC": 80, "E_ZSTD_HEADER": 81, "E_ZSTD_DATA": 82, "E_ZSTD_CHECKSUM": 83,
          "E_ZSTD_DICT": 84}


class ZstdRefError(Exception):
    def __init__(self, status, why=""):
        Exception.__init__(self, "%s %s" % (status, why))
        self.status = status
        self.code = STATUS[status]


def _data(why):
    return ZstdRefError("E_ZSTD_DATA", why)


# ---- XXH64 ---------------------------------------------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, w):
    return (_rotl((acc + w * _P2) & M64, 31) * _P1) & M64


def xxh64(data, seed=0):
    data = bytes(data)
    n, i = len(data), 0
    if n >= 32:
        a = [(seed + _P1 + _P2) & M64, (seed + _P2) & M64, seed & M64, (seed - _P1) & M64]
        while i + 32 <= n:
            for j in range(4):
                a[j] = _round(a[j], int.from_bytes(data[i + 8 * j:i + 8 * j + 8], "little"))
            i += 32
        h = (_rotl(a[0], 1) + _rotl(a[1], 7) + _rotl(a[2], 12) + _rotl(a[3], 18)) & M64
        for j in range(4):
            h = ((h ^ _round(0, a[j])) * _P1 + _P4) & M64
    else:
        h = (seed + _P5) & M64
    h = (h + n) & M64
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[i:i + 8], "little")), 27) * _P1 + _P4) & M64
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * _P1 & M64), 23) * _P2 + _P3) & M64
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * _P5 & M64), 11) * _P1) & M64
        i += 1
    h ^= h >> 33
    h = h * _P2 & M64
    h ^= h >> 29
    h = h * _P3 & M64
    h ^= h >> 32
    return h


# ---- bitstreams ----------------------------------------------------------------------------------------------------------------------
class Backward:
    """read from the last byte's highest set bit downward; `over` once a read went past the first bit (zeros come back)"""

    def __init__(self, data):
        if not data or not data[-1]:
            raise _data("bitstream without an end mark")
        self.v = int.from_bytes(data, "little")
        self.left = self.v.bit_length() - 1
        self.over = False

    def read(self, n):
        if n > self.left:
            r = (self.v & ((1 << self.left) - 1)) << (n - self.left)
            self.over = self.over or n > 0
            self.left = 0
            return r
        self.left -= n
        return (self.v >> self.left) & ((1 << n) - 1)

    def peek(self, n):
        if n > self.left:
            return (self.v & ((1 << self.left) - 1)) << (n - self.left)
        return (self.v >> (self.left - n)) & ((1 << n) - 1)

    def skip(self, n):
        if n > self.left:
            self.over, self.left = True, 0
        else:
            self.left -= n

    def done(self):
        return not self.over and self.left == 0


# ---- FSE -----------------------------------------------------------------------------------------------------------------------------
def read_ncount(data, max_sym, max_log):
    """the normalised counts of a table description -> (counts, accuracy log, bytes consumed); zeros are read behind the description's
    end and the description fails if it used any"""
    v = int.from_bytes(data, "little")
    log = (v & 15) + 5
    if log > max_log:
        raise _data("accuracy log %d over %d" % (log, max_log))
    at, remaining, threshold, nbits = 4, (1 << log) + 1, 1 << log, log + 1
    counts, prev0 = [], False
    while remaining > 1 and len(counts) <= max_sym:
        if prev0:
            n0 = len(counts)
            while (v >> at) & 0xFFFF == 0xFFFF:
                n0, at = n0 + 24, at + 16
            while (v >> at) & 3 == 3:
                n0, at = n0 + 3, at + 2
            n0, at = n0 + ((v >> at) & 3), at + 2
            if n0 > max_sym:
                raise _data("zero run past the last symbol")
            counts += [0] * (n0 - len(counts))
        mx = 2 * threshold - 1 - remaining
        w = (v >> at) & (2 * threshold - 1)
        if w & (threshold - 1) < mx:
            c, at = w & (threshold - 1), at + nbits - 1
        else:
            c, at = (w - mx if w >= threshold else w), at + nbits
        c -= 1
        remaining -= abs(c)
        counts.append(c)
        prev0 = c == 0
        while remaining < threshold:
            nbits, threshold = nbits - 1, threshold >> 1
    if remaining != 1:
        raise _data("distribution does not add up")
    if at > 8 * len(data):
        raise _data("table description runs past its end")
    return counts, log, (at + 7) // 8


def build_fse(counts, log):
    """-> cells of (symbol, bits, baseline)"""
    size = 1 << log
    cell = [0] * size
    high = size - 1
    nxt = []
    for s, c in enumerate(counts):
        if c == -1:
            cell[high] = s
            high -= 1
            nxt.append(1)
        else:
            nxt.append(c)
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(counts):
        for _ in range(max(c, 0)):
            cell[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    tab = []
    for u in range(size):
        s = cell[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        tab.append((s, nb, (ns << nb) - size))
    return tab


LL_CODE = [(i, 0) for i in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3), (48, 4), (64, 6), (128, 7),
                                         (256, 8), (512, 9), (1024, 10), (2048, 11), (4096, 12), (8192, 13), (16384, 14), (32768, 15), (65536, 16)]
ML_CODE = [(i + 3, 0) for i in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3), (67, 4), (83, 4), (99, 5),
                                             (131, 7), (259, 8), (515, 9), (1027, 10), (2051, 11), (4099, 12), (8195, 13), (16387, 14),
                                             (32771, 15), (65539, 16)]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
PRE = {"ll": (build_fse(LL_DEF, 6), 6), "ml": (build_fse(ML_DEF, 6), 6), "of": (build_fse(OF_DEF, 5), 5)}
LIMITS = {"ll": (35, 9), "of": (31, 8), "ml": (52, 9)}


# ---- Huffman -------------------------------------------------------------------------------------------------------------------------
HUF_LOG = 11


def read_huffman(data, trace=None):
    """the table description at the head of `data` -> (table of (symbol, length) indexed by the next `log` bits, log, bytes consumed);
    trace: gets which of the two interleaved states ran off an FSE weight stream"""
    trace = [] if trace is None else trace
    if not data:
        raise _data("no huffman description")
    hb = data[0]
    if hb >= 128:
        nw = hb - 127
        used = 1 + (nw + 1) // 2
        if used > len(data):
            raise _data("huffman weights run past the literals")
        w = [(data[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(nw)]
    else:
        used = 1 + hb
        if used > len(data) or hb < 2:
            raise _data("huffman weights run past the literals")
        counts, log, hdr = read_ncount(data[1:used], 255, 6)
        if hdr >= hb:
            raise _data("no weight bitstream")
        tab = build_fse(counts, log)
        b = Backward(data[1 + hdr:used])
        s1, s2 = b.read(log), b.read(log)
        if b.over:
            raise _data("weight bitstream shorter than its two states")
        w = []
        while True:
            if len(w) > 253:
                raise _data("more than 255 weights")
            sym, nb, base = tab[s1]
            w.append(sym)
            s1 = base + b.read(nb)
            if b.over:
                w.append(tab[s2][0])
                trace.append(("weights_end_state1",))
                break
            if len(w) > 253:
                raise _data("more than 255 weights")
            sym, nb, base = tab[s2]
            w.append(sym)
            s2 = base + b.read(nb)
            if b.over:
                w.append(tab[s1][0])
                trace.append(("weights_end_state2",))
                break
    if any(x > HUF_LOG for x in w):
        raise _data("huffman weight over 11")
    tot = sum((1 << x) >> 1 for x in w)
    if not tot:
        raise _data("huffman weights are all zero")
    log = tot.bit_length()
    if log > HUF_LOG:
        raise _data("huffman codes longer than 11 bits")
    rest = (1 << log) - tot
    if rest & (rest - 1):
        raise _data("huffman weights do not complete a power of two")
    w.append(rest.bit_length())
    ones = sum(1 for x in w if x == 1)
    if ones < 2 or ones & 1:
        raise _data("odd number of the longest huffman codes")
    table, at = [None] * (1 << log), 0
    for wt in range(1, log + 1):
        for s, x in enumerate(w):
            if x == wt:
                for u in range(at, at + (1 << (wt - 1))):
                    table[u] = (s, log + 1 - wt)
                at += 1 << (wt - 1)
    return table, log, used


def huffman_stream(data, table, log, count):
    b = Backward(data)
    out = bytearray()
    for _ in range(count):
        if b.over:
            break
        s, n = table[b.peek(log)]
        b.skip(n)
        out.append(s)
    if not b.done() or len(out) != count:
        raise _data("huffman stream does not end with its last symbol")
    return bytes(out)


# ---- frames --------------------------------------------------------------------------------------------------------------------------
class _Frame:
    def __init__(self, dictionary, trace=None, index=0):
        self.dict = dictionary
        self.index = index                                       # which of the file's Zstandard frames this is
        self.trace = trace if trace is not None else []
        self.out = bytearray()
        self.huf = None
        self.tabs = None
        self.rep = [1, 4, 8]

    def literals(self, blk):
        b0 = blk[0]
        kind, sf = b0 & 3, (b0 >> 2) & 3
        if kind < 2:
            if not sf & 1:
                hs, size = 1, b0 >> 3
            elif sf == 1:
                hs, size = 2, int.from_bytes(blk[:2], "little") >> 4
            else:
                hs, size = 3, int.from_bytes(blk[:3], "little") >> 4
            if hs > len(blk) or size > BLOCK_MAX:
                raise _data("literals header")
            self.trace.append(("lit", ("raw", "rle")[kind], 0, ""))
            self.trace.append(("lithdr%d_%s" % (hs, ("raw", "rle")[kind]),))
            if kind == 0:
                if hs + size > len(blk):
                    raise _data("raw literals run past the block")
                return blk[hs:hs + size], hs + size
            if hs + 1 > len(blk):
                raise _data("RLE literals run past the block")
            return blk[hs:hs + 1] * size, hs + 1
        if len(blk) < 5:
            raise _data("block too short for compressed literals")
        h = int.from_bytes(blk[:4], "little")
        streams = 4
        if sf < 2:
            hs, size, csize = 3, (h >> 4) & 0x3FF, (h >> 14) & 0x3FF
            streams = 4 if sf else 1
        elif sf == 2:
            hs, size, csize = 4, (h >> 4) & 0x3FFF, h >> 18
        else:
            hs, size, csize = 5, (h >> 4) & 0x3FFFF, (h >> 22) + (blk[4] << 10)
        if size > BLOCK_MAX or hs + csize > len(blk) or not size:
            raise _data("compressed literals header")
        body = blk[hs:hs + csize]
        self.trace.append(("hufhdr%d" % hs,))
        if size == BLOCK_MAX:
            self.trace.append(("lit_full",))                    # the literals fill the kernel's buffer
        self.trace.append(("lit", ("huffman", "treeless")[kind - 2], streams, ("direct" if body and body[0] >= 128 else "fse") if kind == 2 else ""))
        if kind == 2:
            table, log, used = read_huffman(body, self.trace)
            self.huf = (table, log)
            body = body[used:]
        elif self.huf is None:
            raise _data("treeless literals with no table before them")
        table, log = self.huf
        if streams == 1:
            return huffman_stream(body, table, log, size), hs + csize
        if len(body) < 10:
            raise _data("four streams in fewer than 10 bytes")
        l1, l2, l3 = (int.from_bytes(body[i:i + 2], "little") for i in (0, 2, 4))
        seg = (size + 3) // 4
        if 6 + l1 + l2 + l3 > len(body) or 3 * seg > size:
            raise _data("jump table")
        cuts = [6, 6 + l1, 6 + l1 + l2, 6 + l1 + l2 + l3, len(body)]
        return b"".join(huffman_stream(body[cuts[i]:cuts[i + 1]], table, log, seg if i < 3 else size - 3 * seg) for i in range(4)), hs + csize

    def seq_table(self, name, mode, data, idx):
        max_sym, max_log = LIMITS[name]
        if mode == 0:
            return PRE[name], 0
        if mode == 1:
            if not data or data[0] > max_sym:
                raise _data("RLE symbol")
            return ([(data[0], 0, 0)], 0), 1
        if mode == 3:
            if self.tabs is None:
                raise _data("repeat mode with no table before it")
            return self.tabs[idx], 0
        counts, log, used = read_ncount(data, max_sym, max_log)
        return (build_fse(counts, log), log), used

    def block(self, blk):
        if len(blk) < 3 or len(blk) >= BLOCK_MAX:
            raise _data("compressed block of %d bytes" % len(blk))
        if self.index:
            self.trace.append(("frame2_compressed",))
        lits, used = self.literals(blk)
        rest = blk[used:]
        if not rest:
            raise _data("no sequences section")
        nseq, at = rest[0], 1
        none = nseq == 0                                         # (libzstd: the one-byte 0 alone ends the section; 80 00 goes on to the modes)
        if nseq >= 128:
            if nseq == 255:
                if len(rest) < 3:
                    raise _data("sequence count")
                nseq, at = rest[1] + (rest[2] << 8) + 0x7F00, 3
            else:
                if len(rest) < 2:
                    raise _data("sequence count")
                nseq, at = ((nseq - 128) << 8) + rest[1], 2
        self.trace.append(("nseq", nseq, at))
        if none:
            if at != len(rest):
                raise _data("bytes behind a count of 0 sequences")
            self.out += lits
            return
        if at >= len(rest):
            raise _data("no symbol modes")
        modes = rest[at]
        at += 1
        self.trace.append(("modes", modes >> 6, (modes >> 4) & 3, (modes >> 2) & 3))
        tabs = []
        for idx, (name, mode) in enumerate((("ll", modes >> 6), ("of", (modes >> 4) & 3), ("ml", (modes >> 2) & 3))):
            t, u = self.seq_table(name, mode, rest[at:], idx)
            tabs.append(t)
            at += u
        if not nseq:                                             # a count of 0 in two or three bytes: the tables are read, what follows is not
            self.out += lits
            return
        self.tabs = tabs
        (t_ll, g_ll), (t_of, g_of), (t_ml, g_ml) = tabs
        b = Backward(rest[at:])
        s_ll, s_of, s_ml = b.read(g_ll), b.read(g_of), b.read(g_ml)
        if b.over:
            raise _data("sequence bitstream shorter than its states")
        rep, out, lp = self.rep, self.out, 0
        for i in range(nseq):
            (c_ll, n_ll, b_ll), (c_ml, n_ml, b_ml), (oc, n_of, b_of) = t_ll[s_ll], t_ml[s_ml], t_of[s_of]
            ov = b.read(oc)
            mlen = ML_CODE[c_ml][0] + b.read(ML_CODE[c_ml][1])
            llen = LL_CODE[c_ll][0] + b.read(LL_CODE[c_ll][1])
            if LL_CODE[c_ll][1] >= 8:
                self.trace.append(("ll_bits>=8",))
            if ML_CODE[c_ml][1] >= 14:
                self.trace.append(("ml_bits>=14",))
            if oc >= 20:
                self.trace.append(("of_code>=20",))
            if oc <= 1:                                          # offset_value 1, 2, 3: the repeat offsets
                self.trace.append(("rep%d%s" % (1 + oc + ov, "" if llen else "_ll0"),))
            if oc > 1:
                off = (1 << oc) + ov - 3
                rep[:] = [off, rep[0], rep[1]]
            elif oc == 0:
                if llen:
                    off = rep[0]
                else:
                    off = rep[1]
                    rep[:] = [off, rep[0], rep[2]]
            else:
                idx = 1 + (0 if llen else 1) + ov
                off = rep[0] - 1 if idx == 3 else rep[idx]
                if not off:
                    self.trace.append(("zero_as_1",))
                    off = 1                                      # (libzstd reads a zero as 1)
                rep[:] = [off, rep[0], rep[1]] if idx != 1 else [off, rep[0], rep[2]]
            if llen > len(lits) - lp:
                raise _data("literal length past the literals")
            if off > len(out) + llen + len(self.dict):
                raise _data("offset beyond history")
            out += lits[lp:lp + llen]
            lp += llen
            if off > BLOCK_MAX:
                self.trace.append(("far",))
            if off < mlen:
                self.trace.append(("overlap",))
            if off > len(out):                                   # the match starts in the dictionary
                self.trace.append(("dict",))
                d = off - len(out)
                take = min(d, mlen)
                if take < mlen:
                    self.trace.append(("dict_straddle",))       # ... and ends in the frame's output
                out += self.dict[len(self.dict) - d:len(self.dict) - d + take]
                mlen -= take
            if mlen:
                if off >= mlen:
                    out += out[len(out) - off:len(out) - off + mlen]
                else:
                    pat = bytes(out[len(out) - off:])
                    out += (pat * (mlen // off + 1))[:mlen]
            if i + 1 < nseq:
                s_ll = b_ll + b.read(n_ll)
                s_ml = b_ml + b.read(n_ml)
                s_of = b_of + b.read(n_of)
            if b.over:
                raise _data("sequence bitstream read past its first bit")
        if not b.done():
            raise _data("bits left over in the sequence bitstream")
        out += lits[lp:]


def decode(blob, dictionary=b"", cap=None, trace=None):
    """-> (bytes, in_used).  cap: the slot's capacity; a result longer than it raises E_OUTPUT_TOO_SMALL with .size, after every other
    check but the content checksums of frames that end beyond it."""
    blob, dictionary = bytes(blob), bytes(dictionary or b"")
    pos, frames, zframes, total = 0, 0, 0, bytearray()
    while True:
        if len(blob) - pos < 4:
            if frames:
                break
            raise ZstdRefError("E_EOF", "file shorter than 4 bytes")
        magic = int.from_bytes(blob[pos:pos + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if len(blob) - pos < 8:
                raise ZstdRefError("E_EOF", "skippable frame header")
            size = int.from_bytes(blob[pos + 4:pos + 8], "little")
            if size > len(blob) - pos - 8:
                raise ZstdRefError("E_EOF", "skippable frame")
            pos += 8 + size
            frames += 1
            continue
        if magic != MAGIC:
            if frames:
                break
            raise ZstdRefError("E_ZSTD_MAGIC")
        if len(blob) - pos < 5:
            raise ZstdRefError("E_EOF", "frame header")
        fhd = blob[pos + 4]
        fcsf, single, didf = fhd >> 6, (fhd >> 5) & 1, fhd & 3
        dids = 4 if didf == 3 else didf
        fcss = single if fcsf == 0 else (2, 4, 8)[fcsf - 1]
        hsize = 5 + (0 if single else 1) + dids + fcss
        if len(blob) - pos < hsize:
            raise ZstdRefError("E_EOF", "frame header")
        if fhd & 8:
            raise ZstdRefError("E_ZSTD_HEADER", "reserved bit")
        q = pos + 5
        if not single:
            if (blob[q] >> 3) + 10 > 31:
                raise ZstdRefError("E_ZSTD_HEADER", "window")
            q += 1
        if int.from_bytes(blob[q:q + dids], "little"):
            raise ZstdRefError("E_ZSTD_DICT")
        q += dids
        fcs = int.from_bytes(blob[q:q + fcss], "little") + (256 if fcss == 2 else 0)
        pos += hsize
        f = _Frame(dictionary, trace, zframes)
        zframes += 1
        f.trace.append(("frame", fcss, 0 if single else 1, (fhd >> 2) & 1))
        while True:
            if len(blob) - pos < 3:
                raise ZstdRefError("E_EOF", "block header")
            bh = int.from_bytes(blob[pos:pos + 3], "little")
            kind, bsize = (bh >> 1) & 3, bh >> 3
            pos += 3
            f.trace.append(("block", kind, bsize))
            if kind == 3:
                raise _data("block type 3")
            csz = 1 if kind == 1 else bsize
            if csz > len(blob) - pos:
                raise ZstdRefError("E_EOF", "block")
            if kind == 0:
                f.out += blob[pos:pos + bsize]
            elif kind == 1:
                f.out += blob[pos:pos + 1] * bsize
            else:
                f.block(blob[pos:pos + bsize])
            pos += csz
            if bh & 1:
                break
        if fcss and len(f.out) != fcs:
            raise _data("decoded size is not the declared one")
        if fhd & 4:
            if len(blob) - pos < 4:
                raise ZstdRefError("E_EOF", "checksum")
            fits = cap is None or len(total) + len(f.out) <= cap
            if fits and xxh64(f.out) & 0xFFFFFFFF != int.from_bytes(blob[pos:pos + 4], "little"):
                raise ZstdRefError("E_ZSTD_CHECKSUM")
            pos += 4
        total += f.out
        frames += 1
    if cap is not None and len(total) > cap:
        e = ZstdRefError("E_OUTPUT_TOO_SMALL")
        e.size, e.used = len(total), pos
        raise e
    return bytes(total), pos


def outcome(blob, dictionary=b"", cap=None):
    """-> (status name, bytes or None, out_len, in_used) as the batch call reports a file"""
    try:
        data, used = decode(blob, dictionary, cap)
        return "OK", data, len(data), used
    except ZstdRefError as e:
        if e.status == "E_OUTPUT_TOO_SMALL":
            return e.status, None, e.size, e.used
        return e.status, None, 0, 0
