"""Hand-built LZ4 blocks for the parser's token WALK (k_lz4_decode_v8.hip: walk_steps2, RCX_WALK_READ).

A step of the walk reads sixteen bytes from the token's LDS address rounded down to 8, picks the three dwords from (address & ~3) on,
and decides from the eight bytes at the token where the next token starts; a match-length extension byte beyond those eight is read
on its own (ds_read_u8).  What a step sees therefore turns on the token's length fields, on how far the match-length extension lies
from the token, and on where the token stands: in its segment of 64 input bytes (a lane each), in the chunk of 4096 (the reads of
its last token reach into the slack staged behind the chunk) and in front of the block's last 20 bytes, which the portable loop takes.

The blocks are built from sequence lists.  Positions are the block's own: with an input that starts 16-byte aligned a chunk is
[4096 k, 4096 (k + 1)) and a segment 64 bytes of it; tests/test_gpu_lz4_walk.py moves every block through all sixteen input
misalignments, which moves every token through all eight read phases and the segment grid across the tokens.

    build(tail_kind, tail_at) -> Case(blob, raw, tokens, named)   the builder asserts that every case of NAMES is in the block
    CASES                                                          the (tail_kind, tail_at) pairs the suites run
    tokens(blob)                                                   an independent walk of a block: one Tok per token"""
import collections
import random

SEG, CHUNK = 64, 4096
Tok = collections.namedtuple("Tok", "pos L M lit_ext match_ext hop nxt last")    # hop: distance token -> where a match-length extension is / would be
Case = collections.namedtuple("Case", "blob raw tokens named")

LITS = [0, 1, 2, 3, 4, 5, 6, 7, 14, 15, 15 + 254, 15 + 255]                    # 0..7, 14, 15 + ext 0, 15 + ext 254, 15 + 255 + 0
MATCHES = [4 + 4, 4 + 14, 4 + 15, 4 + 15 + 254, 4 + 15 + 255]                  # nibble 4, 14, 15 + ext 0, 15 + 254, 15 + 255 + 0
MEXT = [4 + 15, 4 + 15 + 254, 4 + 15 + 255]
DISTS = list(range(3, 15)) + [16, 17, 19]                                      # token -> match-length extension: 3..14, and beyond sixteen bytes
TAILS = {"l1m19": (1, 4 + 15), "l3m273": (3, 4 + 15 + 254), "l7m274": (7, 4 + 15 + 255)}
CASES = [(k, at) for k in sorted(TAILS) for at in (20, 19)]

NAMES = (["lit_%d" % L for L in LITS] + ["match_%d" % M for M in MATCHES] + ["lit_%d_match_%d" % (L, M) for L in LITS for M in MATCHES] +
         ["mext_at_%d_M%d" % (d, M) for d in DISTS for M in MEXT] +
         ["seg_first", "seg_last", "seg_last_straddles", "chunk_last", "chunk_last_at_4095", "tail_at_n_minus_20_or_19"])


def _len_bytes(v):
    """extension bytes of a length field whose nibble is 15 (v = length - 15)"""
    out = bytearray()
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)
    return bytes(out)


def tokens(blob):
    """walk a block as the format says (no checks beyond the buffer's end): one Tok per token"""
    n, p, out = len(blob), 0, []
    while p < n:
        t = blob[p]; q = p + 1
        L, le = t >> 4, 0
        if L == 15:
            while True:
                x = blob[q]; q += 1; le += 1; L += x
                if x != 255:
                    break
        q += L
        if q >= n:
            out.append(Tok(p, L, 0, le, 0, q - p + 2, n, True))
            break
        hop = q + 2 - p
        q += 2
        M, me = (t & 15) + 4, 0
        if (t & 15) == 15:
            while True:
                x = blob[q]; q += 1; me += 1; M += x
                if x != 255:
                    break
        out.append(Tok(p, L, M, le, me, hop, q, False))
        p = q
    return out


class _B:
    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.blob, self.raw, self.k = bytearray(), bytearray(), 0

    @property
    def pos(self):
        return len(self.blob)

    @staticmethod
    def size(L, M):
        return 1 + (len(_len_bytes(L - 15)) if L >= 15 else 0) + L + 2 + (len(_len_bytes(M - 19)) if M >= 19 else 0)

    def seq(self, L, M):
        lits = bytes(self.rnd.randrange(256) for _ in range(L))
        self.blob.append((min(L, 15) << 4) | (min(M - 4, 15) if M else 0))
        if L >= 15:
            self.blob += _len_bytes(L - 15)
        self.blob += lits; self.raw += lits
        if not M:
            return
        self.k += 1
        off = 16 + (self.k * 7) % 48 if self.k % 5 else 1 + self.k % 15          # mostly behind the match, one in five a run
        assert off <= len(self.raw)
        self.blob += bytes((off & 255, off >> 8))
        if M >= 19:
            self.blob += _len_bytes(M - 19)
        for _ in range(M):
            self.raw.append(self.raw[-off])

    def pad_to(self, target):
        """filler tokens (a literal or a few, a match of 4) up to block position `target`"""
        g = target - self.pos
        assert g == 0 or g >= 3, (self.pos, target)
        while g > 8:
            self.seq(1, 4); g -= 4
        if g:
            self.seq(g - 3, 4)
        assert self.pos == target

    def place(self, L, M, at_mod, mod=SEG):
        """the sequence (L, M) with its token at the next block position that is at_mod (mod `mod`), filler in front"""
        t = self.pos + (at_mod - self.pos) % mod
        if 0 < t - self.pos < 3:
            t += mod
        self.pad_to(t)
        self.seq(L, M)
        return t


def build(tail_kind="l1m19", tail_at=20, seed=0x57A1C):
    """One block with every case of NAMES.  Its last token but one -- TAILS[tail_kind] -- starts `tail_at` bytes in front of the block's end:
    20 is the last token the hand-written loop walks, 19 the first one left to the portable loop."""
    b = _B(seed + 31 * sorted(TAILS).index(tail_kind) + tail_at)
    b.seq(70, 4)                                            # history for every offset used below
    # 1. every literal length with every match length, wherever they fall (3.4 KB: inside the first chunk)
    for L in LITS:
        for M in MATCHES:
            b.seq(L, M)
    assert b.pos < CHUNK - 300, b.pos
    # 2. the chunk's last token: its reads reach into the slack behind the chunk
    b.place(2, 4 + 15 + 254, CHUNK - 6, CHUNK)              # starts at 4090, its extension byte at 4095
    assert b.pos == CHUNK
    # 3. the match-length extension at every distance from its token: as a segment's first token, as its last (the fields straddle the
    # boundary), and at a free place
    how = 0
    for d in DISTS:
        L = {16: 13, 17: 14, 19: 15}.get(d, d - 3)
        assert _B.size(L, 19) - 1 == d
        for M in MEXT:
            how += 1
            if how % 3 == 0:
                b.place(L, M, 0)
            elif how % 3 == 1:
                b.place(L, M, SEG - 1 - (how // 3) % 3)     # token at 63, 62, 61 of its segment
            else:
                b.seq(L, M)
    assert b.pos < 2 * CHUNK - 80, b.pos
    b.place(15, 4 + 15, 2 * CHUNK - 1, 2 * CHUNK)           # token at 8191: chunk_last_at_4095 of the second chunk
    b.seq(5, 4 + 15 + 255)
    for _ in range(12):
        b.seq(2, 6)
    # 4. the tail: TAILS[tail_kind] at n - tail_at, then the last token's literals
    tL, tM = TAILS[tail_kind]
    fin = tail_at - _B.size(tL, tM) - 1
    assert 5 <= fin <= 14, fin
    b.seq(tL, tM)
    b.seq(fin, 0)
    blob, raw = bytes(b.blob), bytes(b.raw)
    toks = tokens(blob)
    n = len(blob)
    assert toks[-1].last and toks[-2].pos == n - tail_at and (toks[-2].L, toks[-2].M) == (tL, tM)
    named = _named(toks, n)
    missing = [k for k in NAMES if not named.get(k)]
    assert not missing, missing
    return Case(blob, raw, toks, named)


def _named(toks, n):
    """case name -> the tokens (positions) that are that case"""
    named = collections.defaultdict(list)
    for t in toks:
        if t.last:
            continue
        ext = t.lit_ext or t.match_ext
        if t.L in LITS:
            named["lit_%d" % t.L].append(t.pos)
        if t.M in MATCHES:
            named["match_%d" % t.M].append(t.pos)
        if t.L in LITS and t.M in MATCHES:
            named["lit_%d_match_%d" % (t.L, t.M)].append(t.pos)
        if t.match_ext and t.hop in DISTS and t.M in MEXT:
            named["mext_at_%d_M%d" % (t.hop, t.M)].append(t.pos)
        if ext and t.pos % SEG == 0:
            named["seg_first"].append(t.pos)
        if ext and t.pos // SEG != t.nxt // SEG:
            named["seg_last"].append(t.pos)
            if (t.nxt - 1) // SEG != t.pos // SEG:
                named["seg_last_straddles"].append(t.pos)
        if ext and t.pos // CHUNK != t.nxt // CHUNK:
            named["chunk_last"].append(t.pos)
            if t.pos % CHUNK == CHUNK - 1:
                named["chunk_last_at_4095"].append(t.pos)
        if ext and t.pos in (n - 20, n - 19):
            named["tail_at_n_minus_20_or_19"].append(t.pos)
    return named


def cuts(case):
    """block lengths that end the block INSIDE a token with a length extension: behind its token byte, in front of its match-length
    extension (or where one would be), and in front of its last byte"""
    out = set()
    for t in case.tokens:
        if t.last or not (t.lit_ext or t.match_ext):
            continue
        for c in (t.pos + 1, t.pos + t.hop, t.nxt - 1):
            if t.pos < c < t.nxt:
                out.add(c)
    return sorted(out)
