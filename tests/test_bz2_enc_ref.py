"""The bzip2 encoder's SPECIFICATION, through its serial reference: libbz2, read strictly, returns the input of every
case, the sizes stay within the cap of libbz2's own, and the cases reach what they are there to reach."""
import bz2
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bz2_cases as BC                                                       # noqa: E402
import bz2_craft as K                                                        # noqa: E402
import bz2_enc_cases as EC                                                   # noqa: E402
import bz2_enc_ref as R                                                      # noqa: E402

NAMES = [c[0] for c in EC.cases()]


@pytest.mark.parametrize("name", NAMES)
def test_libbz2_reads_the_reference(name):
    _, data, level, c = EC.by_name(name)
    stream, blocks = EC.ref(name)
    assert BC.strict(stream) == (data, len(stream))
    assert stream[:4] == b"BZh" + bytes([0x30 + level])
    if c is None:                                                            # (a small chunk size changes the blocking: decoding only)
        theirs = len(bz2.compress(data, level))
        print("%s: %d bytes, libbz2 %d" % (name, len(stream), theirs))
        assert len(stream) <= theirs * 1.01 + 8


def test_degenerate_sizes():
    assert len(EC.ref("empty")[0]) == 14 and EC.ref("empty")[1] == []
    assert len(EC.ref("one")[0]) == 37


def test_chunk_rule():
    c = 1000
    assert R.chunks(b"", c) == []
    assert R.chunks(b"x" * 5, c) == [(0, 5)]
    # plain bytes: q = C, chunks of C - C // 64
    assert R.chunks(EC.by_name("exactly_2_chunks")[1], c) == [(0, 985), (985, 985)]
    assert R.chunks(EC.by_name("last_chunk_1")[1], c) == [(0, 985), (985, 985), (1970, 1)]
    d = EC.by_name("run_straddles")[1]
    assert R.chunks(d, c) == [(0, 996), (996, 729)] and d[995:1025] == b"R" * 30                # (the border at 996 is inside the run)
    # 2000 bytes whose pieces' forms are 1200 each: chunks of 820 from the start
    assert R.chunks(EC.by_name("all_expand")[1], c) == [(0, 820), (820, 820), (1640, 360)]
    # the average says 993 bytes, the first chunk's form is C + 1: shortened once more; exactly C: it stays
    d = EC.by_name("over_by_one")[1]
    assert len(K.rle1(d[:993])) == c + 1
    assert R.chunks(d, c) == [(0, 977), (977, 308)]
    d = EC.by_name("fits_exactly")[1]
    assert len(K.rle1(d[:992])) == c
    assert R.chunks(d, c) == [(0, 992), (992, 293)]
    # long runs: a chunk takes many times C input bytes, as libbz2's greedy cut does
    assert R.chunks(b"a" * 5000, c) == [(0, 5000)]
    # the real block size: 120 000 bytes of aaaab at level 1 are two chunks, as libbz2 writes two blocks; text fills its blocks
    assert R.chunks(b"aaaab" * 24000, R.chunk_size(1)) == [(0, 82017), (82017, 37983)]
    assert R.chunk_size(9) == 899981 and R.chunks(b"ab" * 450000, 899981) == [(0, 885919), (885919, 14081)]
    # every chunk fits, and the chunks tile the input
    for _, data, level, cc in EC.cases():
        cc = R.chunk_size(level) if cc is None else cc
        parts = R.chunks(data, cc)
        assert all(len(K.rle1(data[o:o + n])) <= cc for o, n in parts)
        assert [o for o, _ in parts] == [sum(n for _, n in parts[:i]) for i in range(len(parts))] and sum(n for _, n in parts) == len(data)
    assert len(EC.ref("many_blocks")[1]) >= 13


def test_equal_rotations_by_descending_start():
    l, orig = R.rotations(b"abab")
    assert (l, orig) == (b"bbaa", 1)                                         # rotations 2, 0 (equal), then 3, 1
    assert R.rotations(b"aaa") == (b"aaa", 2)
    blocks = EC.ref("ab3000")[1]
    assert blocks[0]["orig"] == 2999


def test_cases_reach_what_they_are_for():
    deep = EC.ref("deep_codes")[1][0]
    assert deep["deepest"] > R.LIMIT and max(max(t) for t in deep["tables"]) == R.LIMIT
    assert EC.ref("unchosen_tables")[1][0]["unchosen"]
    assert len(EC.ref("one_used_byte")[1][0]["tables"][0]) == 3
    assert len(EC.ref("rand64")[1][0]["tables"]) == 2
    assert len(EC.ref("text300")[1][0]["tables"]) in (2, 3) and len(EC.ref("text3000")[1][0]["tables"]) == 5
    assert len(EC.ref("rand3000")[1][0]["tables"]) == 6 and len(EC.ref("text12000")[1][0]["tables"]) == 6
    # zero runs of 1, 2, 3 and 4 in L, and one across a border of the MTF's chunks (32 bytes at the least)
    b = EC.ref("zero_runs")[1][0]
    used = b["used"]
    mtf, ranks = list(used), []
    for x in b["l"]:
        j = mtf.index(x)
        ranks.append(j)
        mtf.insert(0, mtf.pop(j))
    runs, i = [], 0
    while i < len(ranks):
        if ranks[i] == 0:
            j = i
            while j < len(ranks) and ranks[j] == 0:
                j += 1
            runs.append((i, j - i))
            i = j
        else:
            i += 1
    assert {1, 2, 3, 4} <= {n for _, n in runs}
    ch = max(32, -(-len(ranks) // 128))                                      # (k_bzip2_enc.hip: at most 128 chunks of at least 32 bytes)
    assert any(s // ch != (s + n - 1) // ch for s, n in runs)


def test_the_golden_input_is_what_its_generator_makes():
    import gen_bz2_enc_golden
    assert gen_bz2_enc_golden.make() == EC.deep_codes()


def test_code_lengths_are_complete_and_limited():
    for counts in ([0, 0, 1], [5, 0, 0, 0, 9, 1], [1 << k for k in range(25)], [0] * 258, list(range(258))):
        lens, _ = R.code_lengths(counts)
        assert max(lens) <= R.LIMIT and min(lens) >= 1
        assert sum(1 << (R.LIMIT - x) for x in lens) == 1 << R.LIMIT
