"""CPU suite: emit6's HISTORY-ONLY window matches (k_lz4_emit6.hip, RCX_X6_EARLY) on the wave64 simulator.

A window match whose source ends at or below the batch's first output byte is loaded before the copy rounds and stored
with the gathered matches; it enters the rounds with nothing to copy.  The blocks here are hand-built, sequence by
sequence, so that this path can go wrong: every source x destination misalignment, every length on both sides of a
frame (16) and of an entry (32), sources that end exactly at the batch's first byte and one byte past it, sources around
the window's oldest byte (window match <-> gathered match), a block's first batches (nothing gathered yet), batches with
gathered lanes and no early ones, chains that redirection re-points into history, dependents whose only producer is an
early lane, a batch without a single round, a run next to early lanes.

How the parser cuts batches (k_lz4_decode_v8.hip): 64 tokens each, fewer where the entries -- two for a match above 32
bytes -- would pass 64; the batch holding the block's first token and the one holding its last tokens go through emit5,
every other batch built here is plain and must go through emit6 (statistics slot 8 counts those, slot 9 emit5's, slot 14
the copy rounds, slot 15 the early lanes).  `Blk` follows the same rule, so a case knows where each batch begins."""
import ctypes as C

import numpy as np
import pytest

from rust_compress_amd import synth

LZ4_DECODE = 0
MIS = ((0, 0), (1, 1), (2, 7), (3, 14), (13, 3))           # input / output buffer misalignments: those of the emit6 test in test_wavesim_lz4.py
H = 768                                                     # the window's history: between H and H + 15 bytes stand below a batch's first byte


def lz4_block(seqs, tail):
    """an LZ4 block from (literal bytes, match length, offset) triples and the last sequence's literals"""
    out = bytearray()

    def ext(v):
        while v >= 255:
            out.append(255); v -= 255
        out.append(v)
    for lit, m, off in seqs:
        L, M = len(lit), m - 4
        assert m >= 4 and 1 <= off <= 65535
        out.append((min(L, 15) << 4) | min(M, 15))
        if L >= 15: ext(L - 15)
        out += lit
        out += bytes((off & 255, off >> 8))
        if M >= 15: ext(M - 15)
    L = len(tail)
    out.append(min(L, 15) << 4)
    if L >= 15: ext(L - 15)
    out += tail
    return bytes(out)


class Blk:
    """A block under construction: the sequences, the output position, and the batch each token falls into."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.seqs, self.pos = [], 0
        self.b0, self.bt, self.be = 0, 0, 0                 # the open batch: its first output byte, tokens, entries
        self.starts = [0]
        self.sure_early = 0                                 # entries that are early whatever the buffers' alignment
        self.pairs = set()                                  # (source - destination misalignment, destination misalignment) of those

    def _open(self, M):
        """the batch the next token (match length M) falls into"""
        ne = 2 if M > 32 else 1
        if self.bt == 64 or self.be + ne > 64:
            assert self.pos - self.b0 <= 1024, "a batch above the executor's cap would fall back to emit5"
            self.b0, self.bt, self.be = self.pos, 0, 0
            self.starts.append(self.pos)
        return ne

    def tok(self, L, M, off):
        assert L <= 32 and 4 <= M <= 64 and (off >= 16 or M <= 32)
        ne = self._open(M)
        mdst = self.pos + L
        assert off <= mdst
        slo = mdst - off
        if off >= M and slo + M <= self.b0 and slo >= max(0, self.b0 - H + 16):
            self.sure_early += ne
            self.pairs.add((off & 3, mdst & 3))
        self.seqs.append((self.rng.integers(0, 256, L, dtype=np.uint8).tobytes(), M, off))
        self.pos = mdst + M
        self.bt += 1; self.be += ne
        return mdst

    def new_batch(self):
        """fill the open batch up to its 64 tokens (history-only matches of four bytes)"""
        while self.bt < 64 and self.be < 64:
            self.hist(1, 4)

    def hist(self, L, M, below=0, spread=96):
        """a match whose source ends `below` bytes below the open batch's first byte, or -- spread -- up to that many more"""
        self._open(M)
        mdst = self.pos + L
        room = min(spread, self.b0 - M - below)
        extra = int(self.rng.integers(0, room + 1)) if room > 0 else 0
        return self.tok(L, M, mdst - self.b0 + M + below + extra)

    def at(self, L, M, slo):
        self._open(M)
        return self.tok(L, M, self.pos + L - slo)

    def first_batch(self, per_token=8):
        """the batch with the block's first token (emit5): 64 tokens of per_token bytes"""
        for _ in range(64):
            self.tok(per_token - 4, 4, 4)

    def finish(self):
        """the last tokens (emit5: within 40 bytes of the block's end) in a batch of their own, >= 64 bytes behind the last plain batch"""
        self.new_batch()
        for _ in range(4):
            self.tok(12, 4, 7)
        tail = self.rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
        self.n_batches = len(self.starts)
        return lz4_block(self.seqs, tail)


# ------------------------------------------------------------------------------------------------------------ the blocks
def blk_misalign_lengths():
    """history-only matches alone, from the block's first plain batch on (nothing gathered yet): lengths 4 / 15 / 16 / 17 / 31 / 32 at
    every source x destination misalignment, then 33..64 (two entries each) -- not one copy round in the whole block"""
    b = Blk(101)
    b.first_batch()
    k = 0
    for rep in range(4):                                    # 4 batches x 64 tokens
        for i in range(64):
            M = (4, 15, 4, 16, 4, 17, 4, 31, 4, 32, 4, 4)[k % 12] if i % 2 else 4 + (k % 3)
            b.hist(k % 4 if i else 1, M, below=(k // 4) % 4, spread=0 if i % 3 == 0 else 96)
            k += 1
    for M in range(33, 65):
        if b.be + 2 > 30:
            b.new_batch()
        b.hist(M % 4, M, below=M % 5)
        b.hist(1 + M % 3, 4)
    blob = b.finish()
    assert b.pairs == {(s, d) for s in range(4) for d in range(4)}
    return blob, b, dict(rounds=0)


def blk_batch_edge():
    """sources that end exactly at the batch's first byte (early) and one, two ... bytes past it (they wait for the batch's first
    entry), for lengths on both sides of a frame and at every destination misalignment"""
    b = Blk(102)
    b.first_batch()
    for rep in range(3):
        b.new_batch()
        b.tok(3, 6, 300 + rep)                                # the batch's first entry: literals, then a match from history
        for i in range(63):
            M = (4, 16, 17, 32, 5, 15, 31, 8)[(i // 2) % 8] if i % 2 == 0 else 4
            past = (0, 1, 0, 2, 0, 1, 4, 9)[(i // 3) % 8]
            mdst = b.pos + i % 4
            b.tok(i % 4, M, mdst - b.b0 + M - past)           # source end = batch start + past
    return b.finish(), b, {}


def blk_window_floor():
    """sources that start around the window's oldest byte -- H .. H + 15 bytes below the batch's first byte, by the buffer's
    alignment: every start from 40 bytes above to 40 bytes below it, so that the last window match and the first gathered one
    are both there at every alignment; then a batch of gathered matches and dependents with no early lane at all"""
    b = Blk(103)
    b.first_batch(16)
    for rep in range(2):
        b.new_batch()
        for i in range(64):
            b.hist(3, 8)
    b.new_batch()
    b0 = b.pos
    for i in range(64):
        M = (4, 16, 17, 32, 7, 20)[i % 6] if i % 3 == 0 else 4
        b.at(i % 4, M, b0 - (H - 24) - i - (i // 16))       # starts b0 - 744 ... b0 - 810
    b.new_batch()
    b0 = b.pos
    early0 = b.sure_early
    for i in range(64):
        if i % 2 == 0:
            b.at(2, (6, 16, 18, 32)[i // 2 % 4], b0 - 1000 - 3 * i)     # gathered
        else:
            b.tok(1, 5, 6 + i % 3)                                       # from the entry in front: dependent
    assert b.sure_early == early0
    return b.finish(), b, {}


def blk_chains():
    """dependents of early lanes: chains in which every match lies inside the match in front (redirection re-points one, two and
    three links into history; the fourth and fifth wait), and matches that begin in an early lane's literals (not redirected: they
    are ready in the first round, their only producer stands already)"""
    b = Blk(104)
    b.first_batch()
    for rep in range(3):
        b.new_batch()
        b.hist(2, 4)
        for chain in range(5):
            head = b.hist(chain % 4, 24 + chain, below=chain % 3)         # early, up to 30 bytes
            prev, plen = head, 24 + chain
            for depth in range(5):
                M = plen - 2
                L = depth % 3
                b.at(L, M, prev + 1 + depth % 2)                           # inside the match in front
                prev, plen = b.pos - M, M
            m2 = b.hist(3, 12)                                             # early
            b.at(1, 10, m2 - 2)                                            # starts in its literals, runs into its match
            b.at(0, 17, m2 - 3)
    return b.finish(), b, {}


def blk_run_next_to_early():
    """runs -- at most two a plain batch -- among early lanes and lanes that wait for the run; and, first in a batch with no
    literals, a match of more than 16 bytes that overlaps itself at a distance of 16..31: its source ends where the batch begins,
    yet its second frame reads its first"""
    b = Blk(105)
    b.first_batch()
    for rep in range(4):
        b.new_batch()
        b.tok(0, 17 + 5 * rep, 16 + rep * 5 if rep < 3 else 31)            # (0, 17, 16) (0, 22, 21) (0, 27, 26) (0, 32, 31)
        for i in range(20):
            b.hist(i % 4, 4 + i, below=i % 2)
        r = b.tok(2, 20 + rep, 1 + 2 * rep)                                # a run of period 1 / 3 / 5 / 7
        b.at(1, 12, r + 3)                                                 # reads the run
        b.hist(2, 18)
        b.tok(3, 9 + rep, 2 + rep)                                         # a second run
        for i in range(19):
            b.hist(1 + i % 3, 16 + i % 3)
            b.at(0, 6, b.pos - 9)                                          # inside the match in front
    return b.finish(), b, {}


CASES = [blk_misalign_lengths, blk_batch_edge, blk_window_floor, blk_chains, blk_run_next_to_early]
ROUNDS_A_BATCH = 1.7619            # measured: copy rounds a plain batch on the two text blocks below (2.5661 with RCX_X6_EARLY 0)


def _stats():
    import simrun
    lib = simrun.lib()
    lib.sim_stats.restype = C.POINTER(C.c_ulonglong)
    return lib.sim_stats()


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[4:])
def test_early_matches_decode_as_the_oracle(oracle, case):
    import simrun
    blob, b, want = case()
    raw = oracle.lz4_decode_block(blob, cap=b.pos + 24)
    assert len(raw) == b.pos + 24
    st = _stats()
    for variant in (0, 15):
        for mis in MIS:
            for s in (8, 9, 14, 15):
                st[s] = 0
            outs, _, in_used, status, _ = simrun.run(LZ4_DECODE, variant, [blob, blob], [len(raw)] * 2, in_misalign=mis[0], out_misalign=mis[1])
            assert not status.any() and outs == [raw, raw] and list(in_used) == [len(blob)] * 2
            if variant == 0:
                # every batch but the block's first and last went through emit6, and none of those fell back to emit5
                assert (st[8], st[9]) == (2 * (b.n_batches - 2), 2 * 2), (mis, st[8], st[9], b.n_batches)
                assert st[15] >= 2 * b.sure_early > 0, (mis, st[15], b.sure_early)
                if "rounds" in want:
                    assert st[14] == want["rounds"], (mis, st[14])


def test_early_matches_cut_the_copy_rounds(oracle):
    """the two text blocks of test_plain_batches_need_few_copy_rounds: with the history-only matches out of the rounds a plain batch
    needs 1.76 of them where it needed 2.57; the inputs are seeded, the figure is exact -- 5 % of slack for a
    change elsewhere in the executor"""
    import simrun
    st = _stats()
    raws = [synth.gen("text", 65536, 21 + i).tobytes() for i in range(2)]
    blobs = [oracle.lz4_encode_block(r) for r in raws]
    for s in (8, 14, 15):
        st[s] = 0
    outs, _, in_used, status, _ = simrun.run(LZ4_DECODE, 0, blobs, [len(r) for r in raws])
    assert not status.any() and outs == raws and list(in_used) == [len(x) for x in blobs]
    assert st[8] > 100 and st[15] > 15 * st[8], (st[8], st[15])
    assert st[14] < 1.05 * ROUNDS_A_BATCH * st[8], (st[8], st[14], st[14] / st[8])
