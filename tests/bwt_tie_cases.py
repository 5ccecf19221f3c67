"""Inputs whose suffixes tie deep and in groups of chosen sizes: what the suffix sorter's five paths (tests/sa_check.py: classify) get to
sort in the doubling rounds.  Deterministic, seeded; tests/test_sa_check.py proves what the table covers."""
import functools

import numpy as np

SYM0 = 48                                   # the planted texts' alphabet: ALPHA symbols from here, and one more above them for `top`
ALPHA = 60


def planted(g, wlen, seed, noise=(0, 3), top=False, short=0):
    """g copies of one random word of wlen symbols, each followed by a two-byte tag no other copy has and by noise[0]..noise[1] random
    symbols.  The suffixes that start k symbols into the copies share exactly wlen - k symbols: for every k <= wlen - 32 a group of
    exactly g suffixes that stands unchanged from depth 17 to depth 32.  top: the word starts with a symbol above every other one, so
    that the copies' own suffixes are the last g of the suffix array.  short: that many of the copies (the g + short in all) lack the
    word's first symbol: the group of k = 0 has g suffixes, the groups of k >= 1 have g + short -- both sides of a class boundary
    from one text."""
    rng = np.random.default_rng(seed)
    assert g + short <= ALPHA * ALPHA and wlen >= 32 + (1 if short else 0)
    W = rng.integers(0, ALPHA, wlen, dtype=np.uint8) + SYM0
    if top:
        W[0] = SYM0 + ALPHA
    tags = rng.permutation(ALPHA * ALPHA)[:g + short]
    lacks = set(rng.permutation(g + short)[:short].tolist())
    parts = []
    for i, t in enumerate(tags):
        parts += [W[1:] if i in lacks else W, np.array([SYM0 + t // ALPHA, SYM0 + t % ALPHA], dtype=np.uint8),
                  rng.integers(0, ALPHA, int(rng.integers(noise[0], noise[1] + 1)), dtype=np.uint8) + SYM0]
    return np.concatenate(parts).tobytes()


def periodic(p, g, tail, alpha, seed):
    """W^g + W[:tail] for a random primitive word W of p symbols: the suffixes of one phase form a group that loses a member every p
    symbols of depth, so the groups slide down through the size classes round after round, with LCPs near the text's length."""
    rng = np.random.default_rng(seed)
    while True:
        W = rng.integers(0, alpha, p, dtype=np.uint8) + 97
        if all(not np.array_equal(W, np.roll(W, s)) for s in range(1, p)):
            break
    return (W.tobytes() * g) + W.tobytes()[:tail]


def fibonacci(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def thue_morse(n):
    i = np.arange(n, dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        i ^= i >> np.uint64(s)
    return ((i & np.uint64(1)).astype(np.uint8) + 97).tobytes()


LOW = SYM0 - 1                              # a symbol below the planted alphabet: only first_key_bins() uses it


def first_key_bins(counts, seed):
    """sum(counts) copies of one prefix of nine symbols, the i-th symbol of the alphabet behind counts[i] of them, then a two-byte tag
    no other copy with that symbol has.  For the finished bins of the radix partition, which bws_new_group hands to the next round
    (nearly every other group comes out of an LDS sort's queue).  In a doubling round such a bin of exactly 256 does not exist: keys
    are the positions of group heads, a partition step's bin of more than BWS_LMAX suffixes that the last digit alone splits has its
    keys inside 256 positions, and the groups that start there and end there hold fewer than 256 suffixes between them.  In round 0
    keys are symbols: with 33..63 distinct bytes in the batch the first key holds 10 symbols of 6 bits, the copies differ in the
    last one only, and -- the prefix starts with LOW twice, so the copies are the first of k_bws_first's bins all by themselves and the
    levels below start at bit 40 -- the partition walks down to the last digit with all of them (more than BWS_LMAX) in one bin,
    where each count is a bin of equal keys."""
    rng = np.random.default_rng(seed)
    P = rng.integers(0, ALPHA, 9, dtype=np.uint8) + SYM0
    P[:2] = LOW
    follow = np.repeat(np.arange(len(counts), dtype=np.uint8) + SYM0, counts)
    tags = np.concatenate([rng.permutation(ALPHA * ALPHA)[:c] for c in counts])
    rows = np.empty((follow.size, 12), dtype=np.uint8)
    rows[:, :9] = P
    rows[:, 9] = follow
    rows[:, 10] = SYM0 + tags // ALPHA
    rows[:, 11] = SYM0 + tags % ALPHA
    return rows[rng.permutation(follow.size)].tobytes()


def filler(n, seed, alpha=ALPHA, sym0=SYM0):
    """a short block of odd length between two blocks of a batch: the blocks behind it start at another place in the sorter's windows"""
    return (np.random.default_rng(seed).integers(0, alpha, n, dtype=np.uint8) + sym0).tobytes()


def _dense(seed):
    """four planted words in one block: groups of 2, 12, 13 and 32 suffixes, 17 of each that stand from depth 17 to 32"""
    return b"".join(planted(g, 48, 10 * seed + i) for i, g in enumerate((2, 12, 13, 32)))


FIRST_KEY_BINS = (2, 12, 13, 32, 33, 256, 257, 2048, 2049)


@functools.lru_cache(maxsize=None)
def case_table():
    """-> ((name, (block, ...)), ...): the batches the simulator and the GPU sort.  Fillers of 7, 31 and 45 bytes between the blocks."""
    f = lambda n, s: filler(n, 900 + s)
    d1 = _dense(1)
    dense = (d1, f(7, 1), _dense(2), f(31, 2), d1, f(45, 3), _dense(3), f(7, 4), _dense(4), f(31, 5), _dense(5), f(45, 6),
             _dense(22), f(7, 7), planted(9, 40, 77, top=True), f(31, 8), planted(20, 40, 78, top=True))      # d1 twice; the pass ends in a group
    lds = (planted(33, 40, 81), f(7, 11), planted(256, 36, 82, short=1), f(31, 12), f(45, 13), planted(2048, 33, 84, noise=(0, 0), short=1))
    q = lambda n, s: filler(n, 950 + s, 4, 97)
    per = (periodic(37, 33, 5, 4, 1), q(7, 1), periodic(37, 66, 20, 4, 2), q(31, 2), periodic(37, 300, 11, 4, 4), q(45, 3),
           periodic(37, 370, 3, 4, 6), periodic(3, 3500, 2, 3, 7))
    special = (fibonacci(4181), q(7, 6), thue_morse(4096), q(31, 7), bytes(3001), q(45, 8), b"", b"ab" * 2000 + b"a")
    bins = (f(45, 21), first_key_bins(FIRST_KEY_BINS, 91), f(7, 22), f(31, 23))
    return (("planted_dense", dense), ("planted_lds_partition", lds), ("periodic", per), ("special", special), ("first_key_bins", bins))


def bases(blocks):
    """where each block of a batch starts in its sorting pass's array (one pass a batch): the lengths of the blocks before it"""
    out, a = [], 0
    for b in blocks:
        out.append(a)
        a += len(b)
    return out
