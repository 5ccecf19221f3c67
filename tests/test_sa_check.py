"""CPU: the suffix-array certificate itself (tests/sa_check.py), and what the tie-group case table (tests/bwt_tie_cases.py) makes the
suffix sorter do.  The coverage conditions are conditions on the inputs, not measurements of the sorter: the first key holds at most
16 symbols and h doubles from there, so some doubling round has 16 < h <= 32 and some round has 2048 < h <= 4096, whatever first
key the driver picks.  A group that stands unchanged from depth 17 to depth 32 is a group of that round; a group at depth 32 (4096)
whose enclosing group at depth 17 (2049) has the same size class has that class at every depth between."""
import functools

import numpy as np

import bwt_tie_cases as TC
import corpus
import sa_check as S


@functools.lru_cache(maxsize=None)
def _census():
    """Every tie group of the case table at depths 17 / 32 and 2049 / 4096, with where it lies in its sorting pass (one pass a batch)."""
    shallow, same, deep, passes = [], [], [], []
    for bi, (name, blocks) in enumerate(TC.case_table()):
        bases = TC.bases(blocks)
        N = sum(len(b) for b in blocks)
        edges = sorted({a for a, b in zip(bases, blocks) if b and a})          # where a block follows another one
        passes.append((name, N, edges))
        for T, base in zip(blocks, bases):
            sa = S.suffix_array_doubling(T)
            assert S.check_suffix_array(T, sa), name
            t = S.ties(T, sa)
            for lo, hi, out in ((17, 32, shallow), (2049, 4096, deep)):
                if len(T) <= lo:
                    continue
                s0, z0 = t.groups(lo, base)
                s1, z1 = t.groups(hi, base)
                enc = np.searchsorted(s0, s1, side="right") - 1                   # the depth-`lo` group a depth-`hi` group lies in
                assert (enc >= 0).all() and (s0[enc] + z0[enc] >= s1 + z1).all()
                for a, z, e in zip(s1.tolist(), z1.tolist(), enc.tolist()):
                    out.append((bi, a, z, int(z0[e])))
                    if lo == 17 and int(s0[e]) == a and int(z0[e]) == z:
                        same.append((bi, a, z))
    return shallow, same, deep, passes


def test_shallow_band_reaches_every_size_class():
    shallow, _, _, _ = _census()
    got = {S.classify(a, z)[0] for _, a, z, z0 in shallow if S.classify(a, z)[0] == S.classify(a, z0)[0]}
    assert got == set(S.CLASSES)


def test_shallow_band_dense_classes_in_both_window_grids():
    _, same, _, _ = _census()
    got = {S.classify(a, z) for _, a, z in same if z <= 32}
    assert got == {(c, k) for c in ("dense_rank", "dense_bitonic") for k in ("aligned", "shifted")}


def test_exact_sizes_on_both_sides_of_every_class_boundary():
    _, same, _, _ = _census()
    sizes = {z for _, _, z in same}
    assert {2, 12, 13, 32, 33, 256, 257, 2048, 2049} <= sizes


def test_window_and_array_ends():
    _, same, _, passes = _census()
    dense = [(bi, a, z) for bi, a, z in same if z <= 32]
    # the last slot of an aligned window
    assert any((a + z - 1) % 64 == 63 and S.classify(a, z)[1] == "aligned" for _, a, z in dense)
    # The last slot of a shifted window [64 w - 32, 64 w + 32) is position 31 (mod 64).  A group of at most 32 suffixes that ends there
    # starts at 64 w or later: it lies inside the ALIGNED window and the aligned pass has sorted it.  What the shifted pass can meet in
    # its last lane is such a group in a window that it works on, because a group across 64 w has flagged the window.  This is NOT a
    # sort in the last lane and no positive coverage of `nexthead`: it holds the shifted pass to leaving a group alone that this round
    # has sorted already.  (`nexthead` decides for the last group of an aligned window: the slot-63 condition above.)
    shifted = {(bi, (a + 32) >> 6) for bi, a, z in dense if S.classify(a, z)[1] == "shifted"}
    assert any((a + z - 1) % 64 == 31 and (bi, (a + z - 1 + 32) >> 6) in shifted for bi, a, z in dense)
    # the last position of the pass, in a window that the array does not fill
    assert any(a + z == passes[bi][1] and passes[bi][1] % 64 != 0 for bi, a, z in dense)


def test_two_blocks_in_one_window():
    """a window (of the grid that takes the group) with suffixes of two blocks in it and a group to sort"""
    _, same, _, passes = _census()
    def window(a, z):
        w0 = (a >> 6) << 6 if S.classify(a, z)[1] == "aligned" else (((a + 32) >> 6) << 6) - 32
        return w0, w0 + 64
    assert any(any(window(a, z)[0] < e < window(a, z)[1] for e in passes[bi][2]) for bi, a, z in same if z <= 32)


def test_deep_band_reaches_the_lds_sorts_and_the_partition():
    _, _, deep, _ = _census()
    got = {S.classify(a, z)[0] for _, a, z, z0 in deep if S.classify(a, z)[0] == S.classify(a, z0)[0]}
    assert {"lds_wave", "lds_wg", "partition"} <= got


def test_first_key_bins_are_finished_partition_bins_of_the_boundary_sizes():
    """tests/bwt_tie_cases.py, first_key_bins: more than 2048 suffixes in one group at depth 9 (the first key less its last symbol),
    inside it at depth 10 (the first key of a batch with 33..63 distinct bytes) groups of exactly every boundary size; the copies'
    first two symbols occur nowhere else in the block, so they are a first-level bin of their own."""
    blocks = dict(TC.case_table())["first_key_bins"]
    assert 33 <= len(set(b"".join(blocks))) <= 63
    T = max(blocks, key=len)
    t = S.ties(T, S.suffix_array_doubling(T))
    s2, z2 = t.groups(2)
    s9, z9 = t.groups(9)
    s10, z10 = t.groups(10)
    big = int(np.argmax(z9))
    assert z9[big] == sum(TC.FIRST_KEY_BINS) > 2048 and s9[big] == 0
    assert (int(s2[0]), int(z2[0])) == (0, int(z9[big]))                           # the depth-2 group of the prefix is the copies and nothing else
    inside = (s10 >= s9[big]) & (s10 + z10 <= s9[big] + z9[big])
    assert sorted(z10[inside].tolist()) == sorted(TC.FIRST_KEY_BINS)


def test_batches_have_what_the_table_promises():
    for name, blocks in TC.case_table():
        lens = [len(b) for b in blocks]
        assert {7, 31, 45} <= set(lens), name                                     # odd fillers: the bases of the blocks vary
        assert len({a % 64 for a in TC.bases(blocks)}) >= 4, name
    tables = dict(TC.case_table())
    assert any(tables[n].count(b) >= 2 for n in tables for b in tables[n] if len(b) > 1000)      # two identical blocks in one batch


# ---- the checker itself ------------------------------------------------------------------------------------------------------------
def test_certificate_accepts_the_oracles_suffix_arrays(oracle):
    for r in corpus.small_corpus():
        sa = oracle.bwt_suffixes(r)
        assert S.suffix_array_fault(r, sa) is None, len(r)
        assert S.bwt_from_sa(r, sa) == oracle.bwt_encode(r), len(r)
        assert np.array_equal(S.suffix_array_doubling(r), sa)


def test_certificate_rejects_mutants():
    tried = 0
    for r in corpus.small_corpus() + [TC.periodic(37, 33, 5, 4, 1), TC.planted(12, 40, 3)]:
        if len(r) < 4:
            continue
        sa = np.array(S.suffix_array_doubling(r))
        assert S.check_suffix_array(r, sa)
        # two adjacent entries swapped inside a tie group that is deeper than one symbol
        s2, z2 = S.tie_groups(r, sa, 2)
        for a in s2.tolist()[:: max(1, len(s2) // 7)]:
            m = sa.copy(); m[[a, a + 1]] = m[[a + 1, a]]
            assert not S.check_suffix_array(r, m), (len(r), a)
            tried += 1
        # two entries swapped across groups; one entry duplicated over another
        n = len(r)
        for i, j in ((0, n - 1), (n // 3, n // 2), (1, 2)):
            if r[sa[i]:] == r[sa[j]:]:
                continue
            m = sa.copy(); m[[i, j]] = m[[j, i]]
            assert not S.check_suffix_array(r, m), (len(r), i, j)
            m = sa.copy(); m[i] = m[j]
            assert not S.check_suffix_array(r, m), (len(r), i, j)
            tried += 2
        assert not S.check_suffix_array(r, sa[:-1]) and not S.check_suffix_array(r, sa + 1)
    assert tried > 100


def test_tie_groups_against_a_direct_comparison():
    rng = np.random.default_rng(4)
    for T in (b"abracadabra" * 9, bytes(70), b"ab" * 40 + b"a", bytes(rng.integers(0, 3, 400, dtype=np.uint8)), TC.fibonacci(300)):
        sa = S.suffix_array_doubling(T).tolist()
        for d in (1, 2, 3, 7, 17, 32, 33):
            want, j = [], 0
            while j < len(T):
                k = j + 1
                while k < len(T) and sa[j] + d <= len(T) and sa[k] + d <= len(T) and T[sa[j]: sa[j] + d] == T[sa[k]: sa[k] + d]:
                    k += 1
                if k - j >= 2:
                    want.append((j + 5, k - j))
                j = k
            s, z = S.tie_groups(T, sa, d, base=5)
            assert list(zip(s.tolist(), z.tolist())) == want, (len(T), d)


def test_classify_boundaries():
    assert [S.classify(0, z)[0] for z in (2, 12, 13, 32, 33, 256, 257, 2048, 2049)] == \
        ["dense_rank", "dense_rank", "dense_bitonic", "dense_bitonic", "lds_wave", "lds_wave", "lds_wg", "lds_wg", "partition"]
    assert S.classify(32, 32)[1] == "aligned" and S.classify(33, 32)[1] == "shifted" and S.classify(63, 2)[1] == "shifted"
    assert S.classify(64, 12)[1] == "aligned" and S.classify(100, 40) == ("lds_wave", None)
