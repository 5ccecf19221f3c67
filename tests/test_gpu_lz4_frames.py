"""GPU parity: emit6's frame stores (k_lz4_emit6.hip) -- the hand-built blocks of tests/lz4_frame_cases.py through the shipped library,
the default decoder and the v5 fallback, every output buffer poisoned first: bytes, out_len, in_used and statuses as the oracle's,
and nothing written behind a block's last byte.

The wave simulator (tests/test_wavesim_lz4_frames.py) builds without the inline assembly: it stores a frame byte by byte and never
reads the mask table.  So this file is the only check of the hand-written paths -- the table at its row stride and the wide read of
a row, the ds_mskor_b32 stores with four and with five atomics, the copy rounds' paired reads, their wait counts and their skip of
the fifth atomic.  A few hundred copies of each block in one launch, so that several waves share a CU and its LDS."""
import numpy as np
import pytest
import torch

from rust_compress_amd import _native as N
import lz4_frame_cases as K

pytestmark = pytest.mark.gpu

REPS = 40                                                   # 320 blocks a launch: the copies of a case not next to each other
SLACK = 64                                                  # poisoned bytes behind every block's decoded bytes


@pytest.fixture(scope="module")
def hand_built(oracle):
    blobs, raws = [], []
    for case in K.CASES:
        blob, b, _ = case()
        raw = oracle.lz4_decode_block(blob, cap=b.pos + 24)
        assert len(raw) == b.pos + 24
        blobs.append(blob); raws.append(raw)
    return blobs, raws


@pytest.mark.parametrize("variant", [0, 15])
def test_frame_cases_many_to_a_cu(ctx, hand_built, variant):
    blobs, raws = hand_built
    ctx.set_variant(N.LZ4_DECODE, variant)
    try:
        res = ctx.lz4_decode_blocks(blobs * REPS, [len(r) for r in raws] * REPS)
    finally:
        ctx.set_variant(N.LZ4_DECODE, 0)
    assert not res.status.any(), np.nonzero(res.status)[0][:8]
    assert list(res.in_used) == [len(b) for b in blobs] * REPS
    assert list(res.out_len) == [len(r) for r in raws] * REPS
    for i, out in enumerate(res.outputs):
        assert out == raws[i % len(raws)], (i, K.CASES[i % len(raws)].__name__)


@pytest.mark.parametrize("variant", [0, 15])
def test_frame_cases_in_poisoned_buffers(ctx, hand_built, variant):
    """device buffers laid out here: each block's slot filled with 0xA5 first and SLACK bytes longer than its output -- the decoded bytes
    are the oracle's and the slack still holds the poison (a frame store's fifth dword reaches up to 19 bytes past a frame's start)"""
    from rust_compress_amd.api import DeviceBatch
    blobs, raws = hand_built
    dev = torch.device("cuda")
    T = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev)
    in_off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])[:-1]])
    inb = torch.tensor(np.frombuffer(b"".join(blobs) + bytes(64), np.uint8).copy(), device=dev)
    caps = [len(r) for r in raws]
    ooff, total = [], 0
    for c in caps:
        ooff.append(total)
        total += (c + SLACK + 255) & ~255
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    db = DeviceBatch(inb, T(in_off), T([len(b) for b in blobs]), out, T(ooff), T(caps))
    torch.cuda.synchronize()                                # (the context launches on a stream of its own)
    ctx.set_variant(N.LZ4_DECODE, variant)
    try:
        ctx.launch_dev(N.LZ4_DECODE, db)
        torch.cuda.synchronize()
    finally:
        ctx.set_variant(N.LZ4_DECODE, 0)
    host = out.cpu().numpy()
    status, out_len, in_used = db.status.cpu().numpy(), db.out_len.cpu().numpy(), db.in_used.cpu().numpy()
    assert not status.any(), status
    for i, r in enumerate(raws):
        o = ooff[i]
        assert int(out_len[i]) == len(r) and int(in_used[i]) == len(blobs[i]), i
        assert host[o: o + len(r)].tobytes() == r, K.CASES[i].__name__
        assert (host[o + len(r): o + len(r) + SLACK] == 0xA5).all(), K.CASES[i].__name__
