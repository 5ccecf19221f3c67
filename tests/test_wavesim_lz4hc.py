"""CPU suite: the UNMODIFIED LZ4 high-compression encoder kernels (k_lz4_hc.hip) on the wave64 simulator of tests/wavesim.  There is
no oracle for HC: every output must decode with the reference-faithful oracle to its input and pass check_block, a walk of the LZ4
block format that asserts each of its rules.  (On a GPU, tests/test_gpu_lz4_hc.py checks that the device makes the same bytes.)"""
import numpy as np
import pytest

from rust_compress_amd import synth

RCX_RC_BAD_ARG = -1


def check_block(blk, n):
    """Walks one LZ4 block that must decode to n bytes and asserts the format's rules: every match at least 4 bytes long, its
    offset 1..65535 and inside the block, the last 5 bytes literals, the last match starting 12 bytes before the end at the latest,
    the final sequence literals only, nothing after it.  -> (matches, literal bytes)."""
    p, out, matches, lits = 0, 0, 0, 0
    while True:
        assert p < len(blk), "block ends inside a sequence"
        tok = blk[p]
        p += 1
        r = tok >> 4
        if r == 15:
            while True:
                assert p < len(blk)
                b = blk[p]
                p += 1
                r += b
                if b != 255:
                    break
        assert p + r <= len(blk)
        p += r
        out += r
        lits += r
        if p == len(blk):
            assert tok & 15 == 0, "the final sequence holds literals only"
            break
        assert p + 2 <= len(blk)
        off = blk[p] | blk[p + 1] << 8
        p += 2
        assert 1 <= off <= 65535 and off <= out, "offset %d at output %d" % (off, out)
        ml = tok & 15
        if ml == 15:
            while True:
                assert p < len(blk)
                b = blk[p]
                p += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        assert n - out >= 12, "a match starts %d bytes before the end" % (n - out)
        out += ml
        assert n - out >= 5, "a match ends %d bytes before the end" % (n - out)
        matches += 1
    assert out == n
    return matches, lits


def _raws():
    raws = [synth.gen("text", n, 40 + n % 7).tobytes() for n in (0, 1, 4, 5, 11, 12, 13, 65535, 65536, 65537, 150000)]
    for i, k in enumerate(("runs", "dna4", "rand")):
        raws.append(synth.gen(k, 65536 + (i - 1), 3 + i).tobytes())
        raws.append(synth.gen(k, 13 + i, 9).tobytes())
    raws.append(b"\0" * 70000)
    raws.append((b"abcdefg" * 20000)[:131073])
    return raws


KINDS = ("text", "words", "runs", "dna4")


def _blocks(kind):
    return [synth.gen(kind, 65536, s).tobytes() for s in range(100, 102)]


@pytest.fixture(scope="module")
def runs():
    """the simulator runs the tests below share, spread over worker processes (the slowest first)"""
    import sim_lz4hc_run
    jobs = {}
    for lv in (12, 10, 9, 4, 1):
        jobs[("rt", lv)] = (_raws(), lv)
    for lv in range(12, 0, -1):
        jobs[("grow", lv)] = ([b for k in KINDS for b in _blocks(k)], lv)
    return dict(zip(jobs, sim_lz4hc_run.encode_many(list(jobs.values()))))


@pytest.mark.parametrize("level", [1, 4, 9, 10, 12])
def test_round_trip_and_block_format(oracle, runs, level):
    import sim_lz4hc_run
    raws = _raws()
    rc, outs, st, out_len, in_used, _, _ = runs[("rt", level)]
    assert rc == 0 and not st.any()
    assert [int(u) for u in in_used] == [len(r) for r in raws]
    for r, e in zip(raws, outs):
        assert oracle.lz4_decode_block(e, cap=max(len(r), 1)) == r
        check_block(e, len(r))
        assert len(e) <= sim_lz4hc_run.bound(len(r))
        assert len(e) <= 1 + len(r) + (1 + (len(r) - 15) // 255 if len(r) >= 15 else 0)    # never more than the block as literals
    # the long, compressible inputs use matches
    assert check_block(outs[-1], len(raws[-1]))[0] > 0 and check_block(outs[-2], len(raws[-2]))[0] > 0


def test_levels_do_not_grow(oracle, runs):
    """Total over two 64 KiB blocks of each kind: a level is at most 1.005 of the level below (the tolerance of the DEFLATE levels'
    test: a deeper search changes the candidates, and the parse's cost of a literal run is not exact)."""
    tot = []
    for lv in range(1, 13):
        rc, outs, st, _, _, _, _ = runs[("grow", lv)]
        assert rc == 0 and not st.any()
        tot.append(sum(map(len, outs)))
    raws = [b for k in KINDS for b in _blocks(k)]
    for r, e in zip(raws, runs[("grow", 12)][1]):
        assert oracle.lz4_decode_block(e, cap=len(r)) == r
    for k in range(11):
        assert tot[k + 1] <= 1.005 * tot[k], tot


def test_long_runs(oracle):
    """Runs longer than the longest match the search reports come out as one match per segment (the parse's pieces are joined; a
    joined match stays below 2^16 bytes): a few bytes more than the greedy encoder's single match per segment boundary crossed."""
    import sim_lz4hc_run
    raws = [b"z" * 100000, b"\0" * 70000, (b"abcdefg" * 20000)[:131073], bytes(range(7, 12)) * 30000, b"\0" * 65536 * 3]
    rc, outs, st, _, _, _, _ = sim_lz4hc_run.encode(raws, 9)
    assert rc == 0 and not st.any()
    for r, e in zip(raws, outs):
        assert oracle.lz4_decode_block(e, cap=len(r)) == r
        matches, _ = check_block(e, len(r))
        segs = (len(r) + 65535) // 65536
        assert matches <= 2 * segs
        assert len(e) <= len(oracle.lz4_encode_block(r)) + 6 * segs


def test_ratio_against_the_reference_encoder(oracle):
    import sim_lz4hc_run
    raws = [synth.gen("text", 65536, 60 + i).tobytes() for i in range(4)]
    rc, outs, st, _, _, _, _ = sim_lz4hc_run.encode(raws, 9)
    assert rc == 0 and not st.any()
    greedy = sum(len(oracle.lz4_encode_block(r)) for r in raws)
    assert sum(map(len, outs)) <= 0.85 * greedy


def test_slots_levels_and_scratch():
    import sim_lz4hc_run
    raws = [synth.gen(k, 65536, 70 + i).tobytes() for i, k in enumerate(("text", "runs", "dna4"))]
    rc, outs, st, _, _, out, off = sim_lz4hc_run.encode(raws, 1)
    assert rc == 0 and not st.any()
    caps = [sim_lz4hc_run.bound(len(r)) for r in raws]
    caps[1] -= 1
    rc2, outs2, st2, out_len2, in_used2, out2, off2 = sim_lz4hc_run.encode(raws, 1, caps)
    assert rc2 == 0 and list(st2) == [0, 2, 0] and int(out_len2[1]) == 0 and int(in_used2[1]) == 0
    assert outs2[0] == outs[0] and outs2[2] == outs[2]
    # nothing outside the written blocks changes: the too-small slot entirely, the others past out_len
    for i in range(3):
        lo, hi = int(off2[i]) + int(out_len2[i]), int(off2[i]) + caps[i]
        assert (out2[lo:hi] == 0xEE).all()
    for level in (0, 13):
        assert sim_lz4hc_run.encode(raws, level)[0] == RCX_RC_BAD_ARG
    # scratch for the first block's segment only: the others get RCX_E_MALFORMED, the covered one is right
    rc3, outs3, st3, _, _, _, _ = sim_lz4hc_run.encode(raws, 1, scratch_bytes=_scratch_for(3, 1))
    assert rc3 == 0 and list(st3) == [0, 3, 3] and outs3[0] == outs[0]


def _scratch_for(nblocks, segments):
    """hc_scratch_bytes(nblocks, segments) of k_lz4_hc.hip, written out (the kernels are not a library on the CPU)"""
    al = lambda x: (x + 255) & ~255
    base = al(4 * (nblocks + 1)) + al(4 * nblocks) + 2 * al(8 * nblocks) + 256
    seg = 4 * 4 + 8 * 4 + 2 * 65536 + 4 * 65536 + 4 * (65536 + 64)
    return base + segments * seg + 4096
