"""CPU suite: the hand-built blocks of tests/lz4_walk_cases.py are what they say -- each decodes under the oracle to the bytes the
builder states, consuming the whole block, and holds every named case (the builder's own assertion, repeated here from an independent
walk of the block); the cut blocks of the GPU suite end inside a token."""
import pytest

import lz4_walk_cases as K


@pytest.fixture(scope="module")
def cases():
    return {c: K.build(*c) for c in K.CASES}


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "%s-n%d" % c)
def test_block_decodes_to_the_stated_bytes(oracle, cases, case):
    c = cases[case]
    raw = oracle.lz4_decode_block(c.blob, cap=len(c.raw))    # (raises unless the block is well-formed to its last byte)
    assert raw == c.raw
    assert 4 * 1024 + 64 < len(c.blob) < 12 * 1024          # two chunks and a chunk edge, and still a small block


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "%s-n%d" % c)
def test_named_cases_are_present(cases, case):
    c = cases[case]
    toks, n = K.tokens(c.blob), len(c.blob)
    assert toks == c.tokens
    by_pos = {t.pos: t for t in toks}
    for name in K.NAMES:
        assert c.named.get(name), name
    for L in K.LITS:
        assert any(t.L == L and not t.last for t in toks), L
    for M in K.MATCHES:
        assert any(t.M == M for t in toks), M
    for d in K.DISTS:
        for M in K.MEXT:
            assert any(t.hop == d and t.M == M and t.match_ext for t in toks), (d, M)
    # the placements, from the positions alone
    assert any(t.pos % K.SEG == 0 and t.match_ext for t in toks)
    assert any(t.pos % K.SEG == K.SEG - 1 and t.match_ext for t in toks)
    assert any(t.pos < K.CHUNK <= t.nxt and t.match_ext and t.pos + t.hop == K.CHUNK - 1 for t in toks)     # the extension byte is the chunk's last
    assert any(t.pos == 2 * K.CHUNK - 1 and t.lit_ext for t in toks)                                          # the token byte is
    tail = by_pos[n - case[1]]
    assert (tail.L, tail.M) == K.TAILS[case[0]] and tail.match_ext and toks[-1].last and toks[-2] == tail


def test_cuts_end_inside_a_token(cases):
    for c in cases.values():
        cuts = K.cuts(c)
        assert len(cuts) > 100
        starts = sorted(t.pos for t in c.tokens)
        for n in cuts:
            assert n not in starts and 0 < n < len(c.blob)
