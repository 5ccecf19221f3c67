"""CPU suite: compression levels 1..9 of the DEFLATE / zlib / gzip encoder -- the UNMODIFIED kernels (k_deflate_encode.hip,
k_deflate_hc.hip) on the wave64 simulator of tests/wavesim.  Every output must decode with Python's zlib and with the
reference-faithful oracle; level 1 must be the level-1 encoder's bytes; header fields, statuses, determinism and the compression
ratio against Python's zlib at the same level.  (On a GPU, tests/test_gpu_deflate_levels.py checks that the device makes the same
bytes.)  The simulator runs are spread over worker processes and shared by the tests through one module fixture."""
import zlib

import numpy as np
import pytest

from rust_compress_amd import synth
from test_wavesim_deflate import _raws

KINDS = ("text", "words", "runs", "dna4")
WBITS = (-15, 15, 31)
ZLIB_FLEVEL = {1: 0x01, 2: 0x5E, 3: 0x5E, 4: 0x5E, 5: 0x5E, 6: 0x9C, 7: 0xDA, 8: 0xDA, 9: 0xDA}
RCX_RC_BAD_ARG = -1


def _blocks(kind):
    return [synth.gen(kind, 65536, s).tobytes() for s in range(100, 104)]


def _zlib_raw(r, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return len(c.compress(r) + c.flush())


@pytest.fixture(scope="module")
def runs():
    import sim_deflate_hc_run as S
    raws = _raws()
    a = synth.gen("text", 70000, 5).tobytes()
    jobs = {}
    for lv in range(9, 0, -1):                       # (the slowest first)
        for fmt in range(3):
            jobs[("rt", lv, fmt)] = (raws, fmt, lv)
        for k in KINDS:
            jobs[("ratio", lv, k)] = (_blocks(k), 0, lv)
    jobs[("pos", 8, "batch")] = ([a, b"\0" * 1000, a, b"", b"xyz", a], 1, 8)
    jobs[("pos", 8, "alone")] = ([a], 1, 8)
    res = S.encode_many(list(jobs.values()))
    return dict(zip(jobs, res))


@pytest.mark.parametrize("level", range(2, 10))
def test_round_trip(oracle, runs, level):
    raws = _raws()
    for fmt in range(3):
        rc, outs, st, out_len, in_used = runs[("rt", level, fmt)]
        assert rc == 0 and not st.any()
        assert [int(u) for u in in_used] == [len(r) for r in raws]
        for r, e in zip(raws, outs):
            assert zlib.decompress(e, WBITS[fmt]) == r
            if fmt == 0:
                out, used, flags = oracle.inflate(e, cap=max(len(r), 1))
                assert out == r and used == len(e) and flags == 0
            if fmt == 1:
                assert oracle.zlib_decode(e, cap=max(len(r), 1))[0] == r


def test_level_1_is_the_level_1_encoder(runs):
    import sim_deflate_run
    raws = _raws()
    for fmt in range(3):
        assert runs[("rt", 1, fmt)][1] == sim_deflate_run.encode(raws, fmt)[0]
    for k in KINDS:
        assert runs[("ratio", 1, k)][1] == sim_deflate_run.encode(_blocks(k), 0)[0]


def test_headers(runs):
    for lv in range(1, 10):
        for e in runs[("rt", lv, 1)][1]:
            assert e[0] == 0x78 and e[1] == ZLIB_FLEVEL[lv] and (e[0] << 8 | e[1]) % 31 == 0
        for e in runs[("rt", lv, 2)][1]:
            assert e[:3] == b"\x1f\x8b\x08" and e[3:8] == b"\0" * 5 and e[8] == (2 if lv == 9 else 0) and e[9] == 0xFF


def test_same_bytes_at_any_batch_position(runs):
    rc, outs, st, _, _ = runs[("pos", 8, "batch")]
    assert rc == 0 and not st.any()
    alone = runs[("pos", 8, "alone")][1][0]
    assert outs[0] == outs[2] == outs[5] == alone
    assert zlib.decompress(alone, 15) == synth.gen("text", 70000, 5).tobytes()


def test_too_small_slot(runs):
    import sim_deflate_hc_run as S
    raws = [_blocks(k)[0] for k in KINDS]
    outs = [runs[("ratio", 6, k)][1][0] for k in KINDS]
    caps = [len(e) for e in outs]
    caps[1] -= 1
    rc, outs2, st2, out_len2, _, buf, off = S.encode(raws, 0, 6, caps, full=True)
    assert rc == 0 and list(st2) == [0, 2, 0, 0] and int(out_len2[1]) == 0
    assert outs2[0] == outs[0] and outs2[2:] == outs[2:]
    assert (buf[int(off[1]):int(off[1]) + caps[1]] == 0xEE).all()          # nothing of the short slot is written


def test_scratch_too_small_and_bad_level():
    import sim_deflate_hc_run as S
    from rust_compress_amd import _native as N
    raws = [synth.gen("text", 30000, 1).tobytes(), synth.gen("words", 30000, 2).tobytes()]
    L = lambda n, max_block: int(N.lib().rcx_deflate_level_scratch_bytes(n, max_block))
    # the scratch grows linearly in the segments: what two streams need with room for exactly one segment, and no byte more
    per_segment = L(1, 2 * 65536) - L(1, 65536)
    one = L(2, 65536) - per_segment
    rc, outs, st, out_len, _ = S.encode(raws, 0, 4, scratch_bytes=one)
    assert rc == 0 and list(st) == [0, 3] and int(out_len[1]) == 0
    assert zlib.decompress(outs[0], -15) == raws[0]
    rc, outs, st, out_len, _ = S.encode(raws, 0, 4, scratch_bytes=one - 1)     # one byte less: no segment at all
    assert rc == 0 and list(st) == [3, 3] and not out_len.any()
    for lv in (0, 10):
        assert S.encode(raws, 0, lv)[0] == RCX_RC_BAD_ARG


def _totals(runs, level):
    return {k: sum(len(e) for e in runs[("ratio", level, k)][1]) for k in KINDS}


@pytest.mark.parametrize("level", (6, 9))
def test_ratio_against_zlib(runs, level):
    mine = _totals(runs, level)
    ref = {k: sum(_zlib_raw(r, level) for r in _blocks(k)) for k in KINDS}
    for k in KINDS:
        assert mine[k] <= ref[k], (k, mine[k], ref[k])
    assert sum(mine.values()) <= 0.98 * sum(ref.values()), (mine, ref)


def test_levels_do_not_grow(runs):
    tot = [sum(_totals(runs, lv).values()) for lv in range(1, 10)]
    for k in range(8):
        assert tot[k + 1] <= 1.005 * tot[k], tot
