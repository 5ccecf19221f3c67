"""A certificate for suffix arrays, and the tie groups a prefix-doubling sorter meets on the way to one (plain numpy, no GPU).

The oracle's suffix sorter is qsort_r over memcmp: n log n comparisons of LCP bytes each, hopeless on a text whose suffixes share
thousands of symbols.  check_suffix_array() needs no sorter: it is the Burkhardt-Kaerkkaeinen certificate, O(n) and vectorised, in
the reference's order (a proper prefix sorts first: an implicit sentinel below every byte)."""
import numpy as np


def _arrays(T, SA):
    T = np.frombuffer(bytes(T), dtype=np.uint8) if not isinstance(T, np.ndarray) else np.ascontiguousarray(T, dtype=np.uint8)
    SA = np.frombuffer(bytes(SA), dtype="<u4") if isinstance(SA, (bytes, bytearray, memoryview)) else np.asarray(SA)
    return T, SA.astype(np.int64)


def _rank(SA, n):
    rank = np.empty(n, dtype=np.int64)
    rank[SA] = np.arange(n, dtype=np.int64)
    return rank


def suffix_array_fault(T, SA):
    """None if SA is the suffix array of T, else a sentence about the first thing that is wrong.
    (a) SA is a permutation of 0..n-1; (b) with rank = SA^-1 and nx[i] = rank[SA[i] + 1] (-1 past the end),
    (T[SA[i]], nx[i]) < (T[SA[i+1]], nx[i+1]) for every i.  (b) says that every suffix is smaller than its successor GIVEN that the
    order of the suffixes one symbol shorter is the one SA states; by induction over the length of the common prefix the two are
    equivalent to "SA is sorted", and (a) makes it the suffix array."""
    T, SA = _arrays(T, SA)
    n = T.size
    if SA.size != n:
        return "%d entries for %d suffixes" % (SA.size, n)
    if n == 0:
        return None
    if SA.min() < 0 or SA.max() >= n:
        return "an entry outside 0..n-1"
    seen = np.bincount(SA, minlength=n)
    if (seen != 1).any():
        return "not a permutation: suffix %d occurs %d times" % (int(np.argmax(seen != 1)), int(seen[np.argmax(seen != 1)]))
    rank = _rank(SA, n)
    nx = np.full(n, -1, dtype=np.int64)
    inside = SA + 1 < n
    nx[inside] = rank[SA[inside] + 1]
    c = T[SA].astype(np.int64)
    ok = (c[:-1] < c[1:]) | ((c[:-1] == c[1:]) & (nx[:-1] < nx[1:]))
    if not ok.all():
        i = int(np.argmin(ok))
        return "positions %d, %d: suffix %d does not sort before suffix %d" % (i, i + 1, int(SA[i]), int(SA[i + 1]))
    return None


def check_suffix_array(T, SA):
    return suffix_array_fault(T, SA) is None


def bwt_from_sa(T, SA):
    """-> (L bytes, origin): L[i] = T[SA[i] - 1], or T[n - 1] where SA[i] == 0; origin = rank[0] (0 for the empty text)."""
    T, SA = _arrays(T, SA)
    if T.size == 0:
        return b"", 0
    return T[SA - 1].tobytes(), int(np.nonzero(SA == 0)[0][0])        # (index -1 is T[n - 1])


class _Ties:
    """same[d][j]: the suffixes at SA positions j - 1 and j share their first d symbols (j = 0: False).  A doubling over ranks:
    same[a + b][j] = same[a][j] and the suffixes `a` symbols on lie in one depth-b group -- or nothing, when either of them ends
    within its first a symbols (two different suffixes that share a + b >= a + 1 symbols are both longer than a)."""

    def __init__(self, T, SA):
        self.T, self.SA = _arrays(T, SA)
        self.n = self.T.size
        self.rank = _rank(self.SA, self.n)
        c = self.T[self.SA]
        self.same = {1: np.concatenate([[False], c[1:] == c[:-1]])}

    def at(self, d):
        if d not in self.same:
            a = 1 << (d.bit_length() - 1)
            a, b = (a, d - a) if d != a else (d // 2, d // 2)
            sa_, sb_ = self.at(a), self.at(b)
            gid = np.cumsum(~sb_)                                      # the depth-b group of every SA position
            on = self.SA + a
            g = np.where(on < self.n, gid[self.rank[np.minimum(on, self.n - 1)]], -1 - np.arange(self.n))      # (past the end: a group of its own)
            self.same[d] = sa_ & np.concatenate([[False], g[1:] == g[:-1]])
        return self.same[d]

    def groups(self, d, base=0):
        if self.n == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        s = self.at(d)
        heads = np.nonzero(~s)[0]
        sizes = np.diff(np.append(heads, self.n))
        keep = sizes >= 2
        return heads[keep] + base, sizes[keep]


def ties(T, SA):
    """The tie groups of one text at several depths share their doubling tables: ties(T, SA).groups(depth, base)."""
    return _Ties(T, SA)


def tie_groups(T, SA, depth, base=0):
    """-> (start, size): every maximal run of two or more SA positions whose suffixes share their first `depth` symbols -- the groups a
    doubling round with h = depth has to sort.  `base`: the lengths of the blocks before this one in the sorting pass (the sorter's
    windows are counted in the pass's array, so where a group lies in them depends on it)."""
    return _Ties(T, SA).groups(depth, base)


# The sorter's routing (k_bwt_sort.hip), as literals: BWS_WAVE = 32 (the largest group of the dense passes), BWS_LWAVE = 256 (of the
# one-wave LDS sort), BWS_LMAX = 2048 (of the workgroup LDS sort); inside the dense pass `maxlen <= 12u` picks the rank sort.
# With BWS_WAVE = 32 no group can fail bws_dense_ok: 32 consecutive positions that cross a multiple of 64 lie inside the window
# shifted by 32.  So nothing reaches k_bws_small.
CLASSES = ("dense_rank", "dense_bitonic", "lds_wave", "lds_wg", "partition")


def classify(start, size):
    """-> (class, None), or (class, "aligned" | "shifted") for the two dense classes: the group lies inside one 64-suffix window of the
    aligned grid, or only inside one of the grid shifted by 32."""
    start, size = int(start), int(size)
    assert size >= 2
    if size > 2048:
        return "partition", None
    if size > 256:
        return "lds_wg", None
    if size > 32:
        return "lds_wave", None
    kind = "aligned" if start >> 6 == (start + size - 1) >> 6 else "shifted"
    return ("dense_rank" if size <= 12 else "dense_bitonic"), kind


def suffix_array_doubling(T):
    """A suffix array by prefix doubling over numpy sorts (O(n log^2 n) whatever the LCPs): for the tests that need the tie groups of
    an input without a GPU.  Certify what it returns like any other sorter's."""
    T = np.frombuffer(bytes(T), dtype=np.uint8) if not isinstance(T, np.ndarray) else T
    n = T.size
    if n == 0:
        return np.zeros(0, np.int64)
    rank = T.astype(np.int64) + 1                                      # 0: past the end
    k = 1
    while True:
        nxt = np.zeros(n, np.int64)
        nxt[: n - k] = rank[k:] if k < n else 0
        key = rank * (max(n, 256) + 2) + nxt
        order = np.argsort(key, kind="stable")
        ks = key[order]
        new = np.concatenate([[1], 1 + np.cumsum(ks[1:] != ks[:-1])])
        rank = np.empty(n, np.int64)
        rank[order] = new
        if new[-1] == n or k >= n:
            return order
        k *= 2


def assert_block(T, sa_words, L, origin, tag=None):
    """What every sorter test asks of a block: the suffix array it exported (little-endian u32 words) passes the certificate, and the
    transform it wrote is the one that follows from that array."""
    fault = suffix_array_fault(T, sa_words)
    assert fault is None, (tag, len(T), fault)
    eL, eo = bwt_from_sa(T, sa_words)
    assert bytes(L) == eL, (tag, len(T), "L differs from the certified suffix array's")
    assert not len(T) or int(origin) == eo, (tag, len(T), "origin", int(origin), eo)
