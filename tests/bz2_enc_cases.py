"""The inputs of the bzip2 ENCODER's tests (reference, wave simulator, GPU): (name, data, level, C or None for the real one,
100000 * level - 19): what a block holds of run-length form.  A small C changes the blocking, not the format: it
is how many-block files, the shortened chunks and the boundary cases are reached at a few kilobytes (TEST INFRASTRUCTURE)."""
import functools
import os

import numpy as np

from rust_compress_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _synth(kind, n, seed=11):
    return synth.gen(kind, n, seed).tobytes()


def _plain(n, step=7):
    """n bytes without a run"""
    return bytes((i * step + i // 251) % 251 for i in range(n))


def _with_runs4(n, k):
    """n bytes: k runs of exactly four 0xff between stretches without a run"""
    seg = (n - 4 * k) // (k + 1)
    out = b"".join(_plain(seg, 7 + 2 * i) + b"\xff" * 4 for i in range(k))
    return out + _plain(n - len(out), 5)


def _runs_between(k):
    return b"xy" + b"r" * k + b"z" + b"q" * k + b"w"


def deep_codes():
    """An input whose fit meets a code of 18 bits before the limit of 17 (tests/golden/bz2_enc/deep_codes.dat, 10 586 bytes;
    tests/gen_bz2_enc_golden.py makes it again).  How it was made: 16 MTF ranks with the counts 3, 4, 7, 11, 18, ... (each above the sum of all counts two places below it, the upper ones a tenth
    larger), spread evenly over the block so that every group of 50 looks alike and one table takes them all; with RUNA, RUNB and the end
    symbol at weight 1 that is a chain of 19 leaves.  The ranks were turned into L by the MTF's inverse, a few neighbours of L swapped until
    its LF map was a single cycle, L into the text by the inverse transform and the text through the run-length undo.  The block allows no
    40 such symbols: 20 leaves of a chain weigh 14 139 symbols at the least, and the simulator's blocks end at 12 000."""
    with open(os.path.join(HERE, "golden", "bz2_enc", "deep_codes.dat"), "rb") as fh:
        return fh.read()


def zero_runs():
    """a text whose L holds zero runs of 1, 2, 3 and 4 (among others) and runs that cross the borders of the MTF's chunks (32 bytes at the
    least): sorted contexts of unequal lengths"""
    out = bytearray()
    for i, k in enumerate((1, 2, 3, 4, 5, 2, 3, 1, 4, 40, 70, 33)):
        out += (bytes([65 + i]) + b"#") * (k + 1)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def cases():
    rnd = np.random.default_rng(5)
    out = [
        ("empty", b"", 9, None),
        ("one", b"a", 9, None),
        ("two_equal", b"zz", 1, None),
        ("all256x3", bytes(range(256)) * 3, 9, None),
        ("a1000", b"a" * 1000, 9, None),
        ("ab3000", b"ab" * 3000, 5, None),
    ]
    out += [("run%d" % k, _runs_between(k), 9, None) for k in (3, 4, 5, 254, 255, 256, 259, 260, 510, 600)]
    # C = 1000: plain bytes go in chunks of 985.  A run that straddles the border of two chunks (the border is at 996)
    out.append(("run_straddles", _plain(995) + b"R" * 30 + _plain(700, 3), 9, 1000))
    # five input bytes, four of them equal, give six: the forms' sum shortens the chunks to 820 bytes from the start
    out.append(("all_expand", b"aaaab" * 400, 9, 1000))
    # the file's average says 993 bytes a chunk, but the first chunk holds the eight runs of exactly four and its form is C + 1: the chunks
    # are shortened once more; and the same with a form of exactly C, which stays
    out.append(("over_by_one", _with_runs4(985, 8) + _plain(300 - 24, 9) + b"z" * 24, 9, 1000))
    out.append(("fits_exactly", _with_runs4(985, 8) + _plain(300 - 22, 9) + b"z" * 22, 9, 1000))
    out.append(("last_chunk_1", _plain(2 * 985 + 1, 11), 3, 1000))
    out.append(("exactly_2_chunks", _plain(2 * 985, 13), 3, 1000))
    for kind in ("text", "words", "runs", "dna4", "rand"):
        for n in (300, 3000, 12000):
            out.append(("%s%d" % (kind, n), _synth(kind, n), 9 if n != 3000 else 1, None))
    out.append(("rand64", rnd.integers(0, 256, 64, dtype=np.uint8).tobytes(), 9, None))
    out.append(("one_used_byte", b"q" * 3, 9, None))
    out.append(("deep_codes", deep_codes(), 9, None))
    # skewed, homogeneous symbols: two tables take every group, four are chosen by none
    w = 1.45 ** np.arange(40)[::-1]
    out.append(("unchosen_tables", rnd.choice(np.arange(40, 80, dtype=np.uint8), 3000, p=w / w.sum()).tobytes(), 9, None))
    out.append(("zero_runs", zero_runs(), 9, None))
    out.append(("many_blocks", _synth("text", 9000, 8), 2, 700))
    return out


def by_name(name):
    for c in cases():
        if c[0] == name:
            return c
    raise KeyError(name)


def real_c():
    return [c for c in cases() if c[3] is None]


@functools.lru_cache(maxsize=None)
def ref(name):
    """the serial reference's (stream, blocks) of a case, computed once for all tests"""
    import bz2_enc_ref
    _, data, level, c = by_name(name)
    return bz2_enc_ref.encode(data, level, c)
