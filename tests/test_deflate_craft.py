"""CPU suite: the table of hand-assembled DEFLATE streams (deflate_craft_cases.py) against three independent legs, with no kernel
involved.  Valid cases: the token model == the reference-faithful oracle == libz (Python's zlib), apart from the cases that state why
libz refuses them.  Invalid cases: the oracle's status == the status stated by hand in the case."""
import zlib

import deflate_craft as D
import deflate_craft_cases as T


def _libz(stream):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None, None
    return (out, len(stream) - len(d.unused_data)) if d.eof else (None, None)


def test_assembler_against_libz_streams():
    """the writer's own pieces: canonical codes of the fixed block are RFC 1951's, a greedy spelling expands to its list, and a
    stream re-assembled from libz's tokens decodes (by libz) to libz's input"""
    c = D.canonical(D.FIXED_LL)
    assert c[0] == (0x30, 8) and c[143] == (0xBF, 8) and c[144] == (0x190, 9) and c[255] == (0x1FF, 9) and c[256] == (0, 7) and c[287] == (0xC7, 8)
    for lens in ([0] * 300, [3] * 7 + [0] * 140 + [5] * 4 + [0, 0, 7], [1, 0, 0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0]):
        assert D.expand_rle(D.greedy_rle(lens)) == lens
    assert [D.length_symbol(n) for n in (3, 10, 11, 257, 258)] == [(257, 0), (264, 0), (265, 0), (284, 30), (285, 0)]
    assert [D.dist_symbol(d) for d in (1, 4, 5, 6, 24577, 32768)] == [(0, 0), (3, 0), (4, 0), (4, 1), (29, 0), (29, 8191)]
    toks = [(0, b) for b in b"abcabc"] + [(30, 3), (258, 6), (0, 0), (258, 1, 284, 31)]
    for s in (D.Stream().fixed(toks, final=True), D.Stream().dynamic(toks, final=True), D.Stream().dynamic(toks, final=True, rle=D.greedy_rle)):
        assert _libz(s.bytes()) == (s.expected(), len(s.bytes()))


def test_valid_cases_model_oracle_libz(oracle):
    cases = T.valid() + [T.sweep(k) for k in T.SWEEP_ALL]
    refused, unasked = [], []
    for c in cases:
        want = c["want"]
        out, used, flags, st = oracle.inflate(c["stream"], cap=len(want), raise_on_error=False)
        assert (st, out, used, flags) == (0, want, len(c["stream"]), c["flags"]), c["name"]
        got = _libz(c["stream"])
        if c["libz"] is None:
            unasked.append(c["name"])
        elif c["libz"] is True:
            assert got == (want, len(c["stream"])), c["name"]
        else:
            assert isinstance(c["libz"], str) and got == (None, None), c["name"]
            refused.append(c["name"])
    assert len(refused) <= 4 and len(unasked) <= 2, (refused, unasked)      # the incomplete codes alone


def test_the_sweep_is_long_enough():
    """longer than two 8192-bit tiles behind the 448-bit head start, and than two stagings of CB bytes"""
    sw = T.sweep(0)
    assert 8 * len(sw["stream"]) > 2 * 8192 + 448 and len(sw["stream"]) > 2 * T.CB
    names = [c["name"] for c in T.valid()]
    assert set(T.PREFIXED) <= set(names) and set(T.FRAMED) <= set(names) and set(T.FIRST_PASS_HANDS_BACK) <= set(names)


def test_invalid_cases_oracle_and_hand(oracle):
    n = 0
    for c in T.invalid():
        out, used, flags, st = oracle.inflate(c["stream"], cap=c["cap"], raise_on_error=False)
        if c["status"] is not None:                   # (None: a cut stream with a tail, which may even decode)
            assert st == c["status"], (c["name"], c["line"], st)
            n += 1
    assert n > 400


def test_framed_cases(oracle):
    for c in T.framed():
        if c["kind"] == "zlib":
            out, used, flags, st = oracle.zlib_decode(c["stream"], cap=len(c["want"]), raise_on_error=False)
            assert (st, out, used) == (c["status"], c["want"], len(c["stream"])), c["name"]
        try:
            got = zlib.decompress(c["stream"], 15 if c["kind"] == "zlib" else 31)
            assert c["status"] == 0 and got == c["want"], c["name"]
        except zlib.error:
            assert c["status"] != 0, c["name"]
