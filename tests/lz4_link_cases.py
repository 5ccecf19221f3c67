"""Hand-built LZ4 blocks for the segment-link repair of the parser wave (k_lz4_decode_v8.hip, run_parser8 step 2), shared by
tests/test_wavesim_lz4_link.py and tests/test_gpu_lz4_link.py.

PHASE-LOCKED streams: after one long literal run the block is thousands of copies of one p-byte sequence whose bytes are all the
same value b -- the token b, its literals b.., the offset b | b << 8.  A walk started at ANY byte of it reads the same token, so walks
in different phases never meet: a guessing lane lands in its segment in the phase of its own start, the true walk in the phase
the literal run left it in, and every link between two segments fails unless the two happen to agree.  The literal run is as
long as the offset needs (b = 0x10: 4112 bytes back) and its length sets the true phase.

Every builder returns compressed bytes only; the tests decode them with the oracle first and require status OK."""
import numpy as np

CH, SEG = 4096, 64

# period -> the byte: 3: token 0x01 (L 0, M 5, offset 257), 4: 0x10 (L 1, M 4, offset 4112), 5: 0x20 (L 2, offset 8224), 7: 0x40 (L 4, offset 16448)
LOCK = {3: 0x01, 4: 0x10, 5: 0x20, 7: 0x40}


def _ext(v):
    """length-extension bytes for the part of a length above the nibble's 15"""
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def seq(lits, off=None, mlen=None):
    """one LZ4 sequence: `lits` literal bytes, then a match of mlen (>= 4) bytes `off` back; off None: the block's last token"""
    L = len(lits)
    m = 0 if off is None else mlen - 4
    out = bytearray([(min(L, 15) << 4) | min(m, 15)])
    if L >= 15:
        out += _ext(L - 15)
    out += lits
    if off is not None:
        out += bytes([off & 255, off >> 8])
        if m >= 15:
            out += _ext(m - 15)
    return bytes(out)


def unit(period):
    return bytes([LOCK[period]]) * period


def min_run(period):
    b = LOCK[period]
    return b | (b << 8)


def _head(b, run):
    """the opening literal run (bytes b: a guess that starts inside it is in lock step at once); the first match of the locked stretch
    rides on the run's token (M nibble = b & 15, offset b | b << 8)"""
    assert run >= (b | (b << 8))
    out = bytearray([0xF0 | (b & 15)]) + _ext(run - 15) + bytes([b]) * run + bytes([b, b])
    return bytes(out)


TAIL = seq(b"tail-end", None, None)              # 9 bytes: the closing literals


def locked(period, nseq, run=None, lead=0, inserts=(), tail=TAIL):
    """head(run + lead) + nseq locked sequences + tail; inserts: {index: bytes} placed in front of sequence `index`"""
    run = (min_run(period) + 90 if run is None else run) + lead
    ins = dict(inserts)
    out = bytearray(_head(LOCK[period], run))
    u = unit(period)
    for i in range(nseq):
        if i in ins:
            out += ins[i]
        out += u
    if nseq in ins:
        out += ins[nseq]
    return bytes(out + tail)


def locked_len(period, n, lead=0):
    """a locked block of exactly n compressed bytes (n large enough for the run), true phase shifted by `lead`"""
    base = min_run(period) + 3 + lead
    hl = len(_head(LOCK[period], base))
    k, r = divmod(n - hl - len(TAIL), period)
    assert k >= 1, n
    b = locked(period, k, run=base - lead + r, lead=lead)
    if len(b) != n:                                  # (the run's extension grew by a byte)
        b = locked(period, k, run=base - lead + r - 1, lead=lead) if r else locked(period, k - 1, run=base - lead + period - 1, lead=lead)
    assert len(b) == n, (len(b), n)
    return b


# ---- tokens that next_tok_c does not decide from the staged bytes alone (and two it does), to be placed inside a locked stretch
def special(kind, period=4):
    b = LOCK[period]
    off = b | (b << 8)
    lit = bytes([b])
    if kind.startswith("lit"):                       # a literal run of that many bytes, then a 4-byte match
        return seq(lit * int(kind[3:]), off, 4)
    if kind == "mext1":                              # match-length nibble 15 and ONE extension byte: stays on the hop table
        return seq(lit, off, 4 + 15 + 5)
    if kind == "mextff":                             # ... and several 0xff bytes: the general path
        return seq(lit, off, 4 + 15 + 255 + 255 + 7)
    raise ValueError(kind)


SPECIALS = ("lit15", "lit16", "lit270", "lit600", "mext1", "mextff")


def placed(kind, target, period=4, after=80):
    """a locked block whose special token starts at compressed byte `target` exactly, `after` locked sequences behind it"""
    base = min_run(period) + 88
    hl = len(_head(LOCK[period], base))
    k, r = divmod(target - hl, period)
    assert k >= 1
    blob = locked(period, k + after, run=base + r, inserts={k: special(kind, period)})
    assert blob[target:target + len(special(kind, period))] == special(kind, period)
    return blob


def placements(kind, edge, period=4):
    """starts of the special token around `edge` (a chunk edge: a segment edge too): the token ends on, before and behind the edge, spans it,
    starts in the last and the first segment, and jumps over whole segments on either side"""
    tl = len(special(kind, period))
    ds = {-(tl + 66), -(tl + 1), -tl, -(tl - 1), -(tl // 2), -129, -65, -64, -63, -17, -5, -4, -3, -2, -1, 0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129}
    return [edge + d for d in sorted(ds)]


def short_streams():
    """compressed lengths below what a locked stream needs: 4-byte sequences `10 61 01 00` (a literal, a match one byte back) and a literal tail"""
    out = {1: bytes([0x00])}
    for n in (19, 20, 21, 63, 64, 65):
        k, r = divmod(n - 1, 4)
        k -= 2
        r += 8
        out[n] = b"\x10a\x01\x00" * k + seq(b"z" * r, None, None)
        assert len(out[n]) == n
    return out


EDGE_LENGTHS = (4095, 4096, 4097, 4096 + 63, 4096 + 64, 4096 + 65, 8191, 8192, 8193)


def edge_blocks():
    """the lengths the parser's chunks and segments turn on, each in all three phases of the period-3 stream and the four of the period-4 one where it fits"""
    blobs = list(short_streams().values())
    for n in EDGE_LENGTHS:
        for lead in (0, 1, 2):
            blobs.append(locked_len(3, n, lead))
        if n > 4400:
            for lead in (0, 1, 2, 3):
                blobs.append(locked_len(4, n, lead))
    # ragged last segments: every length of the last one, links failing up to it (period 3, short blocks: segment 0 holds the true
    # cursor, the run jumps over 1..4, every later link fails)
    for n in range(600, 600 + 67):
        blobs.append(locked_len(3, n, n % 3))
    return blobs


def giant_blocks():
    """a chunk that is one token: a 4200-byte literal run whose token is the first of the third chunk (the true walk enters the chunk on it), and near misses"""
    return [placed("lit4200", 2 * CH + d, 4, after=40) for d in (-3, -2, -1, 0, 1, 2, 3, 17, 64)] + \
           [placed("lit9000", 2 * CH + d, 4, after=40) for d in (0, 1, 2)]


def phase_blocks():
    """every link fails: the four periods, every true phase; the period-4 stream long enough for three chunks behind the run"""
    blobs = []
    for lead in (0, 1, 2, 3):
        blobs.append(locked(4, 3100, run=4200, lead=lead))
    for period, nseq in ((3, 3000), (5, 1800), (7, 1300)):
        for lead in range(period):
            blobs.append(locked(period, nseq, lead=lead))
    return blobs


def general_blocks():
    blobs = []
    for kind in SPECIALS:
        for t in placements(kind, 2 * CH):
            blobs.append(placed(kind, t))
    for kind in ("lit270", "mextff", "lit16"):       # the same around a plain segment edge, period 3 and 5
        for period, edge in ((3, 1024 + 9 * SEG), (5, 3 * CH + 5 * SEG)):
            for d in (-66, -64, -3, -1, 0, 1, 62, 64):
                blobs.append(placed(kind, edge + d, period))
    return blobs


def malformed(blobs, count, seed):
    """`count` truncations and `count` single-byte mutations of `blobs`, in turn"""
    rng = np.random.default_rng(seed)
    cut, mut = [], []
    for i in range(count):
        b = blobs[i % len(blobs)]
        cut.append(b[: int(rng.integers(0, len(b)))])
        m = bytearray(b)
        # half of the mutations in the locked stretch or the special tokens (the run's literals are most of a block)
        lo = 0 if i % 2 else max(0, len(b) - min(len(b), 2000))
        m[int(rng.integers(lo, len(b)))] = int(rng.integers(0, 256))
        mut.append(bytes(m))
    return cut, mut
