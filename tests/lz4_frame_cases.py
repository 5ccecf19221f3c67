"""Hand-built LZ4 blocks for emit6's FRAME STORES (k_lz4_emit6.hip: store_frame, the mask table, the copy rounds' store).

A frame store writes the bytes [a, a + n) of a 4-byte aligned frame of five dwords (a = 0..3: the destination's misalignment,
n = 1..16) under the masks of table row a + n; a sequence of 17..32 bytes is two frames.  The blocks here put every row 1..19
through every kind of store -- literals, a gathered (far) match, an early (history-only) match, a match copied in a round behind
a producer of its own batch, a run -- and hold the batches the four-or-five-atomics choice turns on: no lane beyond its frame's
first 16 bytes, exactly one lane (the batch's first, last, a middle one; a block a kind of store), neighbours whose frames share a boundary dword with
rows 8 apart (one bank at a row stride of 12 dwords), and one batch that goes through emit5's frame stores.

The batch rule is tests/test_wavesim_lz4_early.py's (`Blk`): 64 tokens a batch, the block's first and last batches through emit5,
every other one plain.  A destination's misalignment is its output position's plus the output buffer's: the blocks step through
all four residues themselves, so an aligned buffer (the GPU suite) sees every row as well.

CASES: functions -> (block, Blk, expectations); tests/test_wavesim_lz4_frames.py and tests/test_gpu_lz4_frames.py run them."""
from test_wavesim_lz4_early import Blk, H

FAR = H + 200                                               # a source this far below a batch's first byte has left the window


def _fit(b, need):
    """open a new batch unless `need` more bytes and the filler tokens after them stay within a batch's 1024"""
    if b.bt >= 60 or b.be >= 60 or (b.pos - b.b0) + need + 5 * (64 - b.bt) > 1000:
        b.new_batch()
        b.hist(1, 4)                                        # (the new batch is open: b.b0 is its first byte)


def _start(seed, bytes_before=0):
    """a block whose first batch (emit5) and, if asked, enough plain batches stand in front: `bytes_before` output bytes"""
    b = Blk(seed)
    b.first_batch(16)                                       # 1024 bytes
    while b.pos < bytes_before:
        b.new_batch()
        for _ in range(64):
            b.hist(3, 9)
    b.new_batch()
    b.hist(1, 4)
    return b


def _ne(M):
    """entries of a match: two above 32 bytes"""
    return 2 if M > 32 else 1


def _new_batch_at(b, a):
    """close the open batch so that the next one begins at output residue a (mod 4): a match of 4..7 bytes in front of new_batch's
    fillers, which are an entry and 5 bytes each"""
    if b.bt >= 63 or b.be >= 63:
        b.new_batch()
        b.hist(1, 4)
    fill = 63 - max(b.bt, b.be)
    b.hist(0, 4 + (a - (b.pos + 5 * fill)) % 4)
    b.new_batch()
    assert b.pos % 4 == a and (b.bt == 64 or b.be == 64)


def _lit_for(b, a):
    """literal count (0..3) that puts the next match at misalignment a"""
    return (a - b.pos) % 4


# ------------------------------------------------------------------------------------------------ every a x n, per store kind
def blk_literals():
    """literal runs of 1..32 bytes at every misalignment (17..32: two frames), each in front of a history-only match of 4 bytes"""
    b = _start(201)
    for L in range(1, 33):
        for a in range(4):
            _fit(b, L + 16)
            pad = (a - b.pos) % 4
            if pad:
                b.hist(0, 4 + pad)                          # (no literals: brings the output position to residue a)
            assert b.pos % 4 == a
            b.hist(L, 4)
    return b.finish(), b, {}


def blk_gathered():
    """gathered matches -- the source has left the window -- of 4..64 bytes at every misalignment (above 32: two entries)"""
    b = _start(202, FAR + 1100)
    k = far = 0
    for M in list(range(4, 33)) + [33, 34, 35, 40, 47, 48, 49, 63, 64]:
        for a in range(4):
            _fit(b, M + 4)
            L = _lit_for(b, a)
            k += 1
            b.at(L, M, b.b0 - FAR - 7 * (k % 29) - M)
            far += _ne(M)
    return b.finish(), b, dict(far=far)


def blk_early():
    """history-only matches of 4..64 bytes at every misalignment, the source at every misalignment too"""
    b = _start(203, 300)
    k = 0
    for M in list(range(4, 33)) + [33, 34, 35, 40, 47, 48, 49, 63, 64]:
        for a in range(4):
            _fit(b, M + 4)
            k += 1
            b.hist(_lit_for(b, a), M, below=k % 4, spread=40)
    return b.finish(), b, dict(early=b.sure_early)


def blk_rounds():
    """matches of 4..64 bytes whose source is the literals and the match of an entry of their own batch: copied in a round, at
    every destination misalignment, the source's misalignment stepping as well"""
    b = _start(204, 300)
    k = nround = 0
    prod, pb0 = None, None
    for M in list(range(4, 33)) + [33, 34, 35, 40, 47, 48, 49, 63, 64]:
        for a in range(4):
            _fit(b, M + 4 + 80)
            if prod is None or b.b0 != pb0 or b.pos - b.b0 + M + 84 > 1000:
                if b.b0 == pb0:
                    b.new_batch()
                    b.hist(1, 4)
                prod, pb0 = b.pos, b.b0
                b.hist(32, 4)                               # the producers: 32 literals, a match of 4, 32 literals ... -- a source that
                b.hist(32, 4)                               # lay inside ONE producer's match would be re-pointed into history and
                b.hist(8, 8)                                # stored early; these begin in literals, both halves of a long one
            k += 1
            L = _lit_for(b, a)
            src = prod + 5 + k % 5
            assert src >= b.b0 and src + M <= b.pos + L      # (this batch's bytes, and the source ends where the match begins or below)
            b.at(L, M, src)
            nround += _ne(M)
    return b.finish(), b, dict(rounds=nround)


def _run_frames(mdst, M, p):
    """the frames emit6's fill_run stores for a run of M bytes and period p at output position mdst: (misalignment, bytes) a step --
    period doubling, whole periods, at most 16 bytes"""
    out, done, back = [], 0, p
    while done < M:
        c = min(back, M - done, 16)
        out.append(((mdst + done) & 3, c))
        done += c
        if 2 * back <= p + done:
            back *= 2
    return out


RUN_PERIODS = (1, 2, 3, 5, 15)
ALL_FRAMES = {(a, n) for a in range(4) for n in range(1, 17)}


def _run_plan():
    """(period, length, misalignment) of the runs: every period on both sides of a frame and at an entry's 32 bytes at every
    misalignment, then -- a step's misalignment is tied to the steps in front of it -- the runs, picked greedily, that bring every
    (a, n), n = 1..16, to fill_run's store"""
    plan = [(p, M, a) for p in RUN_PERIODS for M in sorted({max(4, p + 1), 16, 17, 32}) for a in range(4)]
    have = set()
    for p, M, a in plan:
        have.update(_run_frames(a, M, p))
    cand = [(p, M, a) for p in RUN_PERIODS for M in range(max(4, p + 1), 33) for a in range(4)]
    while have != ALL_FRAMES:
        best = max(cand, key=lambda c: len(set(_run_frames(c[2], c[1], c[0])) - have))
        assert set(_run_frames(best[2], best[1], best[0])) - have
        plan.append(best)
        have.update(_run_frames(best[2], best[1], best[0]))
    return plan


def blk_runs():
    """runs -- period 1, 2, 3, 5, 15 -- two a batch (a third would send the batch through emit5), a lane that reads the run right behind
    it; together their fill steps store every (misalignment, length) pair with 1..16 bytes: asserted here"""
    b = _start(205, 300)
    seen = set()
    for n, (p, M, a) in enumerate(_run_plan()):
        if n % 2 == 0:
            b.new_batch()
            b.hist(1, 4)
            for i in range(10):
                b.hist(i % 4, 5 + i)
        r = b.tok(_lit_for(b, a), M, p)
        assert r % 4 == a
        seen.update(_run_frames(r, M, p))
        if M >= 12:
            b.at(1, 8, r + 2)
        else:
            b.hist(1, 8)
    assert seen == ALL_FRAMES, sorted(ALL_FRAMES - seen)
    return b.finish(), b, dict(rounds=n + 1)


# ------------------------------------------------------------------------------------------------ the fifth dword
def _quiet(b, i):
    """a token no frame of which passes its first 16 bytes whatever the buffer's alignment: a + n <= 3 + 8"""
    b.hist(1 + i % 3, 4 + i % 5)


def _blk_fifth(kind, seed):
    """Batches in which no lane has a + n > 16 (kind "none"), or in which exactly one lane can have it -- the batch's first token, its
    last, one in the middle -- through one kind of store: a literal run ("lit", 15 bytes: a >= 2 reaches the fifth dword), an early
    match, a gathered match, a match copied in a round (its producer stands in front: the fifth token, not the first).  Each batch
    comes at four shifts of the output position, so that whatever the buffer's alignment some have the lane at a >= 2 and some at
    a < 2 (nobody beyond 16 at all).  -> expectations: `fifth`, where each of those frames starts in the output"""
    b = _start(seed, FAR + 1100)
    starts = []
    for where in ((1,) if kind == "none" else (4, 63, 31) if kind == "round" else (0, 63, 31)):
        for shift in range(4):
            if where == 0:
                _new_batch_at(b, shift)                     # the batch's first token is the one: the shift is in the batch's first byte
            else:
                b.new_batch()
                b.hist(shift + 1, 4)                        # token 0: moves everything behind it by `shift`
            for i in range(0 if where == 0 else 1, 64):
                if i != where or kind == "none":
                    _quiet(b, i)
                elif kind == "lit":
                    starts.append(b.pos)
                    b.hist(15, 4)
                elif kind == "early":
                    starts.append(b.hist(1, 15, below=shift))
                elif kind == "far":
                    starts.append(b.at(1, 15, b.b0 - FAR - 33 - shift))
                else:
                    starts.append(b.at(1, 15, b.b0 + 1 + shift))        # token 0's bytes and the next tokens': this batch's
                    assert b.b0 + 1 + shift + 15 <= b.pos - 15
            if where == 0:
                assert b.starts[-1] == (starts[-1] if kind == "lit" else starts[-1] - 1)
    return b.finish(), b, dict(fifth=starts)


def _fifth_case(kind, seed):
    def case():
        return _blk_fifth(kind, seed)
    case.__name__ = "blk_fifth_" + kind
    case.__doc__ = _blk_fifth.__doc__
    return case


FIFTH_CASES = [_fifth_case(k, 206 + 10 * i) for i, k in enumerate(("none", "lit", "early", "far", "round"))]


# ------------------------------------------------------------------------------------------------ shared boundary dwords
def _entry(b, n, kind, k):
    """one frame of n bytes (1..16) with no literals in front, stored with its neighbours' in one instruction: a match of n bytes, or --
    n < 4 -- the second entry of a match of 32 + n"""
    M = n if n >= 4 else 32 + n
    if kind == "early":
        b.hist(0, M, below=k % 3, spread=24)
    elif kind == "far":
        b.at(0, M, b.b0 - FAR - 11 * (k % 7) - M)
    else:
        b.at(0, M, b.b0 + 2 + k % 3)
        assert b.b0 + 2 + k % 3 + M <= b.pos - M


def _pairs():
    """(row of the left lane, row of the right lane), 8 apart, such that the two frames share a dword: the left one ends inside a
    dword (row % 4 != 0), the right one begins there (a = row % 4) and has a match's length left (row - a >= 4).  Rows e and e + 8
    with e % 4 == 0 end on a dword boundary: nothing shared, no pair."""
    out = []
    for e in range(1, 12):
        for left, right in ((e, e + 8), (e + 8, e)):
            if left % 4 and right - left % 4 >= 4:
                out.append((left, right))
    return out


def blk_shared_dwords():
    """neighbouring lanes whose frames share a boundary dword, their rows 8 apart (the rows whose masks meet in a bank at a row stride
    of 12 dwords), as early, gathered and round-copied matches; the early and gathered pairs once inside a batch and once as the
    batch's very first bytes: the window's first dwords whenever the batch begins with a slide"""
    b = _start(207, FAR + 1100)
    k = 0
    for kind in ("early", "far", "round"):
        for at_start in ((False,) if kind == "round" else (False, True)):
            for left, right in _pairs():
                k += 1
                lo, hi = max(0, left - 16), min(3, left - 1)        # the left frame: a + n = left
                a = lo + k % (hi - lo + 1)
                if at_start:
                    _new_batch_at(b, a)
                else:
                    _fit(b, 200)
                    if kind == "round":
                        while b.pos - b.b0 < 80:
                            b.hist(24, 24)                  # (a round needs its producer in the batch)
                    b.hist(0, 4 + (a - b.pos) % 4)
                assert b.pos % 4 == a and (not at_start or b.bt == 64 or b.be == 64)
                _entry(b, left - a, kind, k)
                assert b.pos % 4 == left % 4 and (not at_start or b.b0 + left - a + (32 if left - a < 4 else 0) == b.pos)
                _entry(b, right - left % 4, kind, k + 1)
                _quiet(b, k)
    return b.finish(), b, {}


# ------------------------------------------------------------------------------------------------ emit5's frame stores
def blk_emit5_frames():
    """batches with three runs -- not plain: emit5 -- and gathered matches of every length 4..32 at every misalignment: emit5 stores
    what it gathers with the same frame store and the same table"""
    b = _start(208, FAR + 1100)
    k = 0
    nb5 = 0
    for M in range(4, 33):
        for a in range(4):
            if k % 20 == 0:
                b.new_batch()
                b.hist(1, 4)
                for p in (1, 3, 7):
                    b.tok(2, 12 + p, p)
                nb5 += 1
            k += 1
            b.at(_lit_for(b, a), M, b.b0 - FAR - 5 * (k % 31) - M)
    return b.finish(), b, dict(emit5=nb5)


CASES = [blk_literals, blk_gathered, blk_early, blk_rounds, blk_runs] + FIFTH_CASES + [blk_shared_dwords, blk_emit5_frames]
