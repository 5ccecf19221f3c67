"""Regenerates tests/golden/bz2_enc/deep_codes.dat: an input of 10 586 bytes whose table fit meets a code of 18 bits before the limit
of 17 (bz2_enc_cases.deep_codes has why it has 16 ranks and not 40 symbols).  python tests/gen_bz2_enc_golden.py [--check]
(TEST INFRASTRUCTURE)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import bz2_craft as K                                                        # noqa: E402
import bz2_enc_ref as R                                                      # noqa: E402

OUT = os.path.join(HERE, "golden", "bz2_enc", "deep_codes.dat")
PHASE, SCALE, BASE = 4, 1.1, 60


def text_with_l(l):
    """-> (text, L'): a text whose rotation sort gives L', which is l with a few neighbours swapped so that its LF map is one cycle"""
    l = bytearray(l)
    n = len(l)
    while True:
        order = sorted(range(n), key=lambda i: (l[i], i))
        cyc = [-1] * n
        nc = 0
        for s in range(n):
            if cyc[s] < 0:
                p = s
                while cyc[p] < 0:
                    cyc[p] = nc
                    p = order[p]
                nc += 1
        if nc == 1:
            break
        # swapping unequal neighbours of L composes the map with a transposition: two cycles become one
        for i in range(n - 1):
            if cyc[i] != cyc[i + 1] and l[i] != l[i + 1]:
                l[i], l[i + 1] = l[i + 1], l[i]
                break
        else:
            raise ValueError("cannot join the cycles")
    t, c = K.walk(bytes(l), 0)
    assert c == n
    return t, bytes(l)


def counts():
    """16 ranks: 3, 4, then each the sum of the two before -- each above the sum of all counts two places below it, so that with RUNA, RUNB
    and the end symbol at weight 1 the Huffman tree is a chain --, the counts from 100 on a tenth larger (room for what the swaps disturb)"""
    c = [3, 4]
    while len(c) < 16:
        c.append(c[-1] + c[-2])
    return [int(x * SCALE) if x >= 100 else x for x in c]


def symbols(c):
    """the ranks spread evenly over the block, the most frequent first in number: every group of 50 looks alike"""
    c = c[::-1]
    slots = []
    for s, k in enumerate(c):
        slots += [(((j + 0.5 + PHASE * s * 0.37) % k) / k, s) for j in range(k)]
    slots.sort()
    return [s + 2 for _, s in slots]                                         # (rank r >= 1 is symbol r + 1: no RUNA / RUNB)


def make():
    c = counts()
    used = list(range(BASE, BASE + len(c) + 1))
    l = K.symbols_to_l(symbols(c), used)
    t, _ = text_with_l(l)
    data = K.unrle(t)
    assert K.rle1(data) == t and len(data) <= 12000
    block = R.encode(data, 9)[1][0]
    assert block["deepest"] > R.LIMIT, block["deepest"]
    return data


if __name__ == "__main__":
    data = make()
    if "--check" in sys.argv:
        with open(OUT, "rb") as fh:
            assert fh.read() == data, "the golden file differs from what this script makes"
        print("deep_codes.dat: %d bytes, as generated" % len(data))
    else:
        with open(OUT, "wb") as fh:
            fh.write(data)
        print("wrote %s (%d bytes)" % (OUT, len(data)))
