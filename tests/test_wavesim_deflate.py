"""CPU suite: the UNMODIFIED DEFLATE encoder kernels (k_deflate_encode.hip) on the wave64 simulator of tests/wavesim.  Every output must
decode with Python's zlib (raw / zlib / gzip framing) and with the reference-faithful oracle; statuses and slot sizes as the C-ABI
promises.  (On a GPU, tests/test_gpu_deflate_encode.py checks that the device makes the same bytes.)"""
import zlib

import numpy as np
import pytest

from rust_compress_amd import synth


def _raws():
    raws = [b"", b"a", b"ab", b"abc", b"abcd", b"hello hello hello hello", bytes(range(256)) * 3]
    for i, k in enumerate(("text", "words", "dna4", "runs", "rand")):
        raws.append(synth.gen(k, 65536 + (i - 2), 3 + i).tobytes())
    raws.append(synth.gen("text", 150000, 9).tobytes())
    raws.append(b"\0" * 70000)
    raws.append((b"abcdefg" * 20000)[:131073])
    return raws


@pytest.mark.parametrize("fmt,wbits", [(0, -15), (1, 15), (2, 31)])
def test_round_trip(oracle, fmt, wbits):
    import sim_deflate_run
    raws = _raws()
    outs, st, out_len, in_used = sim_deflate_run.encode(raws, fmt)
    assert not st.any()
    assert [int(u) for u in in_used] == [len(r) for r in raws]
    for r, e in zip(raws, outs):
        assert zlib.decompress(e, wbits) == r
        if fmt == 0:
            out, used, flags = oracle.inflate(e, cap=max(len(r), 1))
            assert out == r and used == len(e) and flags == 0
        if fmt == 1:
            assert oracle.zlib_decode(e, cap=max(len(r), 1))[0] == r


def test_too_small_slot_and_compression_against_zlib_1():
    import sim_deflate_run
    raws = [synth.gen(k, 65536, 20 + i).tobytes() for i, k in enumerate(("text", "words", "dna4", "runs"))]
    outs, st, _, _ = sim_deflate_run.encode(raws, 0)
    assert not st.any()
    for r, e in zip(raws, outs):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        assert len(e) <= len(c.compress(r) + c.flush())
    caps = [len(e) for e in outs]
    caps[1] -= 1
    outs2, st2, out_len2, _ = sim_deflate_run.encode(raws, 0, caps)
    assert list(st2) == [0, 2, 0, 0] and int(out_len2[1]) == 0
    assert outs2[0] == outs[0] and outs2[2:] == outs[2:]


def test_compression_bound_values():
    from rust_compress_amd import _native as N
    b = N.lib().rcx_deflate_compression_bound
    assert [int(b(n)) for n in (0, 1, 65535, 65536, 65537, 1 << 20)] == [2, 14, 65548, 65549, 65561, (1 << 20) + 178]
    assert (N.DEFLATE_ENCODE, N.ZLIB_ENCODE, N.GZIP_ENCODE, N.CODEC_COUNT) == (26, 27, 28, 29)
