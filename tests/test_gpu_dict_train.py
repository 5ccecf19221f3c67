"""GPU suite of dictionary training (rcx_dict_train_batch; k_dict_train.hip): the jobs of tests/dict_train_cases.py from host and from
device memory against the serial reference's bytes (tests/dict_train_ref, host code run in this process); the call twice; and trained
dictionaries through the encoders and decoders behind shared dictionaries and through libz."""
import ctypes as C
import zlib

import numpy as np
import pytest

import dict_train_cases as K
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu

SENT = 0xEE


def _p(a):
    return a.ctypes.data if a is not None else None


class Trained:
    """One rcx_dict_train_batch call over jobs = [(samples, C)]: corpora three bytes apart, the slots three bytes apart among sentinels"""

    def __init__(self, ctx, jobs, k, d, f, device=False, expect=N.RC_OK):
        n = len(jobs)
        corp = [b"".join(s) for s, _ in jobs]
        self.in_len = np.array([len(c) for c in corp], np.uint64)
        self.in_off = (np.concatenate([[0], np.cumsum(self.in_len + np.uint64(3))[:-1]]) + 1).astype(np.uint64)
        inb = np.full(int(self.in_off[-1] + self.in_len[-1]) + 16, 0x5A, np.uint8)
        for o, c in zip(self.in_off, corp):
            inb[int(o):int(o) + len(c)] = np.frombuffer(c, np.uint8)
        nsamples = np.array([len(s) for s, _ in jobs], np.uint32)
        sample_len = np.array([len(x) for s, _ in jobs for x in s] or [0], np.uint64)
        self.out_cap = np.array([c for _, c in jobs], np.uint64)
        self.out_off = (np.concatenate([[0], np.cumsum(self.out_cap + np.uint64(3))[:-1]]) + 5).astype(np.uint64)
        out = np.full(int(self.out_off[-1] + self.out_cap[-1]) + 16, SENT, np.uint8)
        self.out_len, self.in_used, self.status = np.full(n, 0x7777, np.uint64), np.full(n, 0x7777, np.uint64), np.full(n, -1, np.int32)
        if device:
            import torch
            d_in, d_out = torch.from_numpy(inb).cuda(), torch.from_numpy(out).cuda()
            b = N.Batch(d_in.data_ptr(), _p(self.in_off), _p(self.in_len), d_out.data_ptr(), _p(self.out_off), _p(self.out_cap),
                        _p(self.out_len), _p(self.in_used), _p(self.status), n, N.MEM_DEVICE)
        else:
            b = N.Batch(_p(inb), _p(self.in_off), _p(self.in_len), _p(out), _p(self.out_off), _p(self.out_cap), _p(self.out_len),
                        _p(self.in_used), _p(self.status), n, N.MEM_HOST)
        self.rc = N.lib().rcx_dict_train_batch(ctx._h, C.byref(b), C.c_void_p(_p(nsamples)), C.c_void_p(_p(sample_len)), k, d, f)
        self.error = N.lib().rcx_last_error(ctx._h).decode()
        assert self.rc == expect, (self.rc, self.error)
        self.out = d_out.cpu().numpy() if device else out
        self.dicts = [bytes(self.out[int(o):int(o) + int(l)]) for o, l in zip(self.out_off, self.out_len)] if self.rc == N.RC_OK else None

    def untouched_outside(self):
        """only slot bytes were written (a slot's bytes beyond out_len are unspecified)"""
        mask = np.ones(self.out.size, bool)
        for o, c in zip(self.out_off, self.out_cap):
            mask[int(o):int(o) + int(c)] = False
        return bool((self.out[mask] == SENT).all())


def _calls():
    """(name, [(name, samples, C)], k, d, f): the batch of twelve, the size edges for both d, colliding hashes, k = 4096, and a job
    larger than any launch's grid times its tile beside one with C beyond the last launch's"""
    calls = [("batch", K.batch_jobs(), 64, 8, 20)]
    for d in (6, 8):
        calls.append(("sizes d=%d" % d, [(n, s, c) for n, s, c, _, _, _ in K.size_jobs(16, d)], 16, d, 20))
    t = K.text(65536, 21)
    calls.append(("f=10", [("f=10", K.split(t, [2048] * 31), 4096)], 256, 8, 10))
    calls += [(n, [(n, s, c)], k, d, f) for n, s, c, k, d, f in K.param_jobs() if k == 4096 or (k, f) == (d, 22)]
    big = K.text(200 * 1024, 33)
    calls.append(("large", [("one epoch", K.split(big, [70000, 65536]), 1000), ("large C", K.split(big[:150000], [4096] * 30), 32768)], 256, 8, 20))
    return calls


CALLS = _calls()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("call", CALLS, ids=[c[0] for c in CALLS])
def test_parity_with_the_reference(ctx, call, device):
    _, jobs, k, d, f = call
    t = Trained(ctx, [(s, c) for _, s, c in jobs], k, d, f, device)
    for i, (name, s, c) in enumerate(jobs):
        ref = K.ref_train(s, c, k, d, f)
        assert t.status[i] == 0 and int(t.in_used[i]) == sum(len(x) for x in s), name
        assert int(t.out_len[i]) == len(ref), (name, int(t.out_len[i]), len(ref))
        assert t.dicts[i] == ref, name
    assert t.untouched_outside()


def test_the_call_twice_gives_equal_bytes(ctx):
    jobs = [(s, c) for _, s, c in K.batch_jobs()]
    a, b = Trained(ctx, jobs, 64, 8, 20), Trained(ctx, jobs, 64, 8, 20)
    assert a.dicts == b.dicts and (a.out_len == b.out_len).all()
    order = [7, 2, 0, 11, 5, 9, 1, 3, 10, 4, 8, 6]
    p = Trained(ctx, [jobs[i] for i in order], 64, 8, 20, device=True)
    assert [p.dicts[order.index(i)] for i in range(12)] == a.dicts


def test_refusals(ctx):
    jobs = [([b"x" * 100], 64)]
    for kw in (dict(k=16, d=7, f=20), dict(k=7, d=8, f=20), dict(k=4097, d=8, f=20), dict(k=16, d=8, f=9), dict(k=16, d=8, f=23)):
        t = Trained(ctx, jobs, kw["k"], kw["d"], kw["f"], expect=N.RC_BAD_ARG)
        assert "dict train" in t.error
    b = N.Batch(None, None, None, None, None, None, None, None, None, 0, N.MEM_HOST)
    assert N.lib().rcx_dict_train_batch(ctx._h, C.byref(b), None, None, 256, 8, 20) == N.RC_OK
    assert N.lib().rcx_dict_train_scratch_bytes(256, 1 << 20, 32768, 256, 20) >= 256 * ((10 << 20) + (4 << 20) + 32768)


@pytest.fixture(scope="module")
def trained(ctx):
    """32 KiB from 256 text records of 2 KiB (Context.train_dictionary), the corpus head, and 1024 further records"""
    train = K.records("text", 256, 2048, 1000)
    d = ctx.train_dictionary(train, 32768)
    assert d == K.ref_train(train, 32768, 256, 8, 20) and len(d) == 32768
    return d, b"".join(train)[:32768], K.records("text", 1024, 2048, 5000)


def test_round_trip_behind_the_trained_dictionary(ctx, trained):
    """LZ4 HC level 9 and DEFLATE level 6 behind the trained dictionary decode to the records, and take less than behind the corpus
    head, which takes less than no dictionary.  (Through libz the trained dictionary is 14 % ahead of the head on these records, and this
    project's DEFLATE sizes lie within a few percent of libz's.)"""
    d, head, recs = trained
    caps = [len(r) for r in recs]
    tot = {}
    for name, dic in (("trained", d), ("head", head)):
        e = ctx.lz4_encode_hc_dict_blocks(recs, dic, level=9).check()
        assert ctx.lz4_decode_dict_blocks(e.outputs, dic, caps).check().outputs == recs
        z = ctx.deflate_encode_dict_blocks(recs, dic, level=6).check()
        assert ctx.inflate_dict_blocks(z.outputs, dic, caps).check().outputs == recs
        tot[name] = (int(e.out_len.sum()), int(z.out_len.sum()))
    tot["none"] = (int(ctx.lz4_encode_hc_blocks(recs, level=9).check().out_len.sum()), int(ctx.deflate_encode(recs, level=6).check().out_len.sum()))
    print("round trip totals (lz4 hc 9, deflate 6):", tot)
    for i in (0, 1):
        assert tot["trained"][i] < tot["head"][i] < tot["none"][i], tot


def test_zlib_streams_behind_the_trained_dictionary_are_libz_readable(ctx, trained):
    d, _, recs = trained
    z = ctx.zlib_encode(recs[:64], level=6, zdict=d, shared=True).check()
    for s, r in zip(z.outputs, recs):
        o = zlib.decompressobj(zdict=d)
        assert o.decompress(s) + o.flush() == r and o.eof
