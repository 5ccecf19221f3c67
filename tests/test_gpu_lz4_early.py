"""GPU parity: emit6's history-only window matches (k_lz4_emit6.hip, RCX_X6_EARLY) -- the hand-built blocks of
tests/test_wavesim_lz4_early.py, a few hundred copies of each in one launch so that several waves share a CU, through the
default decoder and the v5 fallback, and 64 text blocks of 64 KiB: bytes, in_used and statuses as the oracle's."""
import pytest

from rust_compress_amd import _native as N
from rust_compress_amd import synth
from test_wavesim_lz4_early import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hand_built(oracle):
    blobs, raws = [], []
    for case in CASES:
        blob, b, _ = case()
        raw = oracle.lz4_decode_block(blob, cap=b.pos + 24)
        assert len(raw) == b.pos + 24
        blobs.append(blob); raws.append(raw)
    return blobs, raws


@pytest.fixture(scope="module")
def texts(oracle):
    raws = [synth.gen("text", 65536, 300 + i).tobytes() for i in range(64)]
    blobs = [oracle.lz4_encode_block(r) for r in raws]
    for b, r in zip(blobs, raws):
        assert oracle.lz4_decode_block(b, cap=len(r)) == r
    return blobs, raws


@pytest.mark.parametrize("variant", [0, 15])
def test_hand_built_blocks_many_to_a_cu(ctx, hand_built, variant):
    blobs, raws = hand_built
    reps = 300                                             # 1500 blocks: six to a CU, and the copies of a case not next to each other
    ctx.set_variant(N.LZ4_DECODE, variant)
    try:
        res = ctx.lz4_decode_blocks(blobs * reps, [len(r) for r in raws] * reps)
    finally:
        ctx.set_variant(N.LZ4_DECODE, 0)
    assert not res.status.any()
    assert list(res.in_used) == [len(b) for b in blobs] * reps
    for i, out in enumerate(res.outputs):
        assert out == raws[i % len(raws)], (i, i % len(raws))


@pytest.mark.parametrize("variant", [0, 15])
def test_text_blocks(ctx, texts, variant):
    blobs, raws = texts
    ctx.set_variant(N.LZ4_DECODE, variant)
    try:
        res = ctx.lz4_decode_blocks(blobs, [len(r) for r in raws])
    finally:
        ctx.set_variant(N.LZ4_DECODE, 0)
    assert not res.status.any()
    assert res.outputs == raws and list(res.in_used) == [len(b) for b in blobs]
