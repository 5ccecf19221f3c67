"""GPU suite of DEFLATE with history: rcx_deflate_encode_hist_batch / rcx_zlib_encode_dict_batch (k_deflate_hc_hist.hip) and
rcx_inflate_hist_batch / rcx_zlib_decode_dict_batch (k_inflate_hist.hip).  The cases of tests/deflate_hist_cases.py against the wave
simulator's bytes and statuses, every encoded stream back through the decoders with history (from host and from device memory) and
through libz, hist_len NULL against the level encoder and the plain decoders, one batch of 4096 records behind a dictionary, the
argument checks, and the Python methods."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_hist_cases as K
import sim_deflate_hist_run as S
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu

SENT = 0xEE
LEVELS = K.LEVELS


def _p(a):
    return a.ctypes.data if a is not None else None


class Encoded:
    """One rcx_deflate_encode_hist_batch (dict_id None) or rcx_zlib_encode_dict_batch call over a laid-out buffer; the output slots lie
    in a buffer of sentinels"""

    def __init__(self, ctx, inb, in_off, lens, hist_len, level, caps=None, device=False, dict_id=None, expect=N.RC_OK):
        n = len(lens)
        self.in_off, self.in_len = np.array(in_off, np.uint64), np.array(lens, np.uint64)
        caps = [S.bound(int(l), dict_id is not None) for l in lens] if caps is None else caps
        self.out_cap = np.array(caps, np.uint64)
        self.out_off = (np.concatenate([[0], np.cumsum(self.out_cap + np.uint64(3))[:-1]]) + 5).astype(np.uint64)
        out = np.full(int(self.out_off[-1] + self.out_cap[-1]) + 16, SENT, np.uint8)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        hist = np.array(hist_len, np.uint64) if hist_len is not None else None
        ids = np.array(dict_id, np.uint32) if dict_id is not None else None
        if device:
            import torch
            d_in, d_out = torch.from_numpy(np.ascontiguousarray(inb).copy()).cuda(), torch.from_numpy(out).cuda()
            b = N.Batch(d_in.data_ptr(), _p(self.in_off), _p(self.in_len), d_out.data_ptr(), _p(self.out_off), _p(self.out_cap),
                        _p(self.out_len), _p(self.in_used), _p(self.status), n, N.MEM_DEVICE)
        else:
            b = N.Batch(_p(inb), _p(self.in_off), _p(self.in_len), _p(out), _p(self.out_off), _p(self.out_cap), _p(self.out_len),
                        _p(self.in_used), _p(self.status), n, N.MEM_HOST)
        if dict_id is None:
            self.rc = N.lib().rcx_deflate_encode_hist_batch(ctx._h, C.byref(b), level, C.c_void_p(_p(hist)))
        else:
            self.rc = N.lib().rcx_zlib_encode_dict_batch(ctx._h, C.byref(b), level, C.c_void_p(_p(hist)), C.c_void_p(_p(ids)))
        self.error = N.lib().rcx_last_error(ctx._h).decode()
        assert self.rc == expect, (self.rc, self.error)
        self.out = d_out.cpu().numpy() if device else out
        self.outputs = [bytes(self.out[int(o):int(o) + int(l)]) for o, l in zip(self.out_off, self.out_len)]

    def untouched_outside(self):
        mask = np.ones(self.out.size, bool)
        for o, l in zip(self.out_off, self.out_len):
            mask[int(o):int(o) + int(l)] = False
        return bool((self.out[mask] == SENT).all())


class Decoded:
    """One rcx_inflate_hist_batch (zlib False) or rcx_zlib_decode_dict_batch call in the buffers of S.decode_buffers; told: the
    hist_len array the call gets ("null": NULL; None: the histories' lengths); plain: rcx_inflate_batch / rcx_zlib_decode_batch"""

    def __init__(self, ctx, streams, hists, caps, zlib_form=False, dict_id=None, fronts=None, misalign=None, told=None, device=False,
                 plain=False, expect=N.RC_OK):
        n = len(streams)
        inb, in_off, in_len, out, out_off, out_cap = S.decode_buffers(streams, hists, caps, fronts, misalign)
        before = out.copy()
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        self.flags = np.full(n, 0xFFFFFFFF, np.uint32)
        hl = None if isinstance(told, str) else np.array([len(h or b"") for h in hists] if told is None else told, np.uint64)
        ids = np.array(dict_id if dict_id is not None else [0] * n, np.uint32)
        if device:
            import torch
            d_in, d_out = torch.from_numpy(inb).cuda(), torch.from_numpy(np.ascontiguousarray(out)).cuda()
            b = N.Batch(d_in.data_ptr(), _p(in_off), _p(in_len), d_out.data_ptr(), _p(out_off), _p(out_cap), _p(self.out_len),
                        _p(self.in_used), _p(self.status), n, N.MEM_DEVICE)
        else:
            b = N.Batch(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(self.out_len), _p(self.in_used),
                        _p(self.status), n, N.MEM_HOST)
        L = N.lib()
        if plain:
            self.rc = (L.rcx_zlib_decode_batch if zlib_form else L.rcx_inflate_batch)(ctx._h, C.byref(b), C.c_void_p(_p(self.flags)))
        elif zlib_form:
            self.rc = L.rcx_zlib_decode_dict_batch(ctx._h, C.byref(b), C.c_void_p(_p(self.flags)), C.c_void_p(_p(hl)), C.c_void_p(_p(ids)))
        else:
            self.rc = L.rcx_inflate_hist_batch(ctx._h, C.byref(b), C.c_void_p(_p(self.flags)), C.c_void_p(_p(hl)))
        self.error = L.rcx_last_error(ctx._h).decode()
        assert self.rc == expect, (self.rc, self.error)
        res = d_out.cpu().numpy() if device else out
        self.clean = S.only_slots_changed(res, before, out_off, out_cap)
        self.outputs = [bytes(res[int(o):int(o) + int(l)]) for o, l in zip(out_off, self.out_len)]

    def results(self):
        return self.outputs, list(self.out_len), list(self.in_used), list(self.status), list(self.flags)


# ------------------------------------------------------------------------------------------------------------------ the simulator
@pytest.fixture(scope="module")
def sim():
    """the simulator's answers, computed once: the encode batch per level, and the decode cases"""
    B = K.batch()
    inb = B.array()
    cs = K.decode_cases()
    lv = sorted(LEVELS, reverse=True)
    jobs = [("run", (inb, B.in_off, B.lens, B.hist_len, l), {"caps": B.caps}) for l in lv]
    jobs.append(("inflate", ([c["stream"] for c in cs], [c["hist"] for c in cs], [c["cap"] for c in cs]),
                 {"fronts": [c["front"] for c in cs], "misalign": [i % 16 for i in range(len(cs))]}))
    res = S.run_many(jobs)
    enc = dict(zip(lv, res[:len(lv)]))
    assert all(r[0] == 0 for r in enc.values())
    return enc, res[-1]


# ------------------------------------------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("level,device", [(2, False), (6, False), (9, False), (6, True)], ids=["2-host", "6-host", "9-host", "6-device"])
def test_encode_equals_the_simulator_and_round_trips(ctx, sim, level, device):
    B = K.batch()
    e = Encoded(ctx, B.array(), B.in_off, B.lens, B.hist_len, level, B.caps, device)
    rc, outs, st, out_len, in_used = sim[0][level][:5]
    small = B.index("small slot")
    assert list(e.status) == list(st) and e.status[small] == N.E_OUTPUT_TOO_SMALL and not np.delete(e.status, small).any()
    assert list(e.out_len) == list(out_len) and list(e.in_used) == list(in_used)
    bad = [B.names[i] for i in range(len(outs)) if e.outputs[i] != outs[i]]
    assert not bad, bad
    assert e.untouched_outside()
    assert e.outputs[B.index("bait x")] == e.outputs[B.index("bait y")]
    keep = [i for i in range(len(outs)) if i != small]
    d = Decoded(ctx, [e.outputs[i] for i in keep], [B.history(i) for i in keep], [B.lens[i] for i in keep], device=device,
                misalign=[i % 16 for i in keep])
    assert not any(d.status) and d.clean and d.outputs == [B.block(i) for i in keep]
    assert list(d.in_used) == [len(e.outputs[i]) for i in keep]


@pytest.mark.parametrize("level", LEVELS)
def test_zlib_form_round_trips_and_libz_reads_it(ctx, level):
    B = K.batch()
    pick = [i for i, nm in enumerate(B.names) if B.lens[i] <= 1000 or nm in ("h32768 n65536", "h0 n65836")]
    ids = [zlib.adler32(B.history(i)) if B.hist_len[i] else 0xDEADBEEF for i in pick]
    e = Encoded(ctx, B.array(), [B.in_off[i] for i in pick], [B.lens[i] for i in pick], [B.hist_len[i] for i in pick], level, dict_id=ids)
    raw = Encoded(ctx, B.array(), [B.in_off[i] for i in pick], [B.lens[i] for i in pick], [B.hist_len[i] for i in pick], level)
    plain = ctx.zlib_encode([B.block(i) for i in pick], level=level).check()
    assert not e.status.any() and e.untouched_outside()
    flevel = 1 if level <= 5 else 2 if level == 6 else 3
    for k, i in enumerate(pick):
        o, h, b = e.outputs[k], B.history(i), B.block(i)
        assert o[0] == 0x78 and (o[0] * 256 + o[1]) % 31 == 0 and o[1] >> 6 == flevel and o[-4:] == zlib.adler32(b).to_bytes(4, "big")
        if h:
            assert o[1] & 0x20 and o[2:6] == ids[k].to_bytes(4, "big") and o[6:-4] == raw.outputs[k], B.names[i]
            z = zlib.decompressobj(zdict=h)
            assert z.decompress(o) == b and z.eof, B.names[i]
        else:
            assert o == plain.outputs[k], B.names[i]
    for device in (False, True):
        d = Decoded(ctx, e.outputs, [B.history(i) for i in pick], [B.lens[i] for i in pick], zlib_form=True, dict_id=ids, device=device,
                    misalign=[(5 * k) % 16 for k in range(len(pick))])
        assert not any(d.status) and d.clean and d.outputs == [B.block(i) for i in pick]
        assert list(d.in_used) == [len(o) for o in e.outputs]


@pytest.mark.parametrize("level", LEVELS)
def test_without_history_every_result_is_the_level_encoders(ctx, level):
    B = K.batch()
    pick = [i for i, nm in enumerate(B.names) if nm.startswith("h0 ") or nm.startswith("chain")]
    raws = [B.block(i) for i in pick]
    buf, off = bytearray(), []
    for r in raws:
        buf += b"\xC3" * 3
        off.append(len(buf))
        buf += r
    inb = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8)
    for zl in (False, True):
        caps = [S.bound(len(r)) + (6 if zl else 0) for r in raws]
        caps[3] = 1                                                       # (a status that is not 0)
        want = (ctx.zlib_encode if zl else ctx.deflate_encode)(raws, caps, level)
        assert want.status[3] == N.E_OUTPUT_TOO_SMALL
        for hist in (None, [0] * len(raws)):
            e = Encoded(ctx, inb, off, [len(r) for r in raws], hist, level, caps, dict_id=[7] * len(raws) if zl else None)
            assert e.outputs == want.outputs
            assert list(e.status) == list(want.status) and list(e.out_len) == list(want.out_len) and list(e.in_used) == list(want.in_used)


def test_more_work_items_than_the_links_grid(ctx):
    B = K.many_batch()
    e = Encoded(ctx, B.array(), B.in_off, B.lens, B.hist_len, 2, B.caps)
    rc, outs, st = S.run(B.array(), B.in_off, B.lens, B.hist_len, 2, caps=B.caps, fill=None)[:3]
    assert not e.status.any() and e.outputs == outs
    tiny = [i for i in range(len(B.names)) if B.lens[i]]
    assert len(tiny) == 12 and all(len(e.outputs[i]) < 40 for i in tiny)
    d = Decoded(ctx, [e.outputs[i] for i in tiny], [B.history(i) for i in tiny], [B.lens[i] for i in tiny])
    assert d.outputs == [B.block(i) for i in tiny]


def test_bad_arguments_are_refused(ctx):
    t = K.text(5000, 3)
    inb = np.frombuffer(b"\xC3" * 100000 + t + b"\0" * 16, np.uint8)
    off, lens = [100000, 102000], [2000, 3000]
    Encoded(ctx, inb, off, lens, [32768, 32768], 6)                                          # (the most a history can be)
    e = Encoded(ctx, inb, off, lens, [0, 32769], 6, expect=N.RC_BAD_ARG)
    assert "block 1" in e.error
    e = Encoded(ctx, inb, [100, 102000], [2000, 3000], [101, 0], 6, expect=N.RC_BAD_ARG)     # more than lies in front of the block
    assert "block 0" in e.error
    e = Encoded(ctx, inb, off, lens, [0, 32769], 6, dict_id=[1, 2], expect=N.RC_BAD_ARG)
    assert "block 1" in e.error
    for level in (0, 1, 10, -1):                                                             # (level 1 has no history)
        Encoded(ctx, inb, off, lens, [10, 10], level, expect=N.RC_BAD_ARG)
        Encoded(ctx, inb, off, lens, None, level, expect=N.RC_BAD_ARG)
    s = zlib.compress(b"abc")
    d = Decoded(ctx, [s[2:-4], s[2:-4]], [b"x" * 10, b"y" * 10], [3, 3], told=[10, 32769], expect=N.RC_BAD_ARG)
    assert "block 1" in d.error
    d = Decoded(ctx, [s, s], [b"x" * 10, b"y" * 10], [3, 3], zlib_form=True, dict_id=[0, 0], told=[1 << 20, 0], expect=N.RC_BAD_ARG)
    assert "block 0" in d.error                                                              # (more than lies in front of the slot)
    assert N.lib().rcx_status_string(25) == b"zlib dictionary id mismatch"
    with pytest.raises(ValueError):
        ctx.deflate_encode_hist_blocks([b"a", b"b"], [None], 6)


# ------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_decode_equals_the_simulator(ctx, sim, device):
    cs = K.decode_cases()
    d = Decoded(ctx, [c["stream"] for c in cs], [c["hist"] for c in cs], [c["cap"] for c in cs], fronts=[c["front"] for c in cs],
                misalign=[i % 16 for i in range(len(cs))], device=device)
    outs, out_len, in_used, st, flags = sim[1]
    assert d.clean
    bad = [c["name"] for i, c in enumerate(cs) if (d.outputs[i], d.out_len[i], d.in_used[i], d.status[i], d.flags[i])
           != (outs[i], out_len[i], in_used[i], st[i], flags[i])]
    assert not bad, bad
    for i, c in enumerate(cs):
        assert d.status[i] == c["status"] and d.outputs[i] == c["want"], c["name"]


def test_decode_without_lengths_is_the_plain_decoder(ctx):
    cs = K.decode_cases()
    args = ([c["stream"] for c in cs], [c["hist"] for c in cs], [c["cap"] for c in cs])
    plain = Decoded(ctx, *args, plain=True).results()
    assert Decoded(ctx, *args, told="null").results() == plain
    assert Decoded(ctx, *args, told=[0] * len(cs)).results() == plain
    zs = K.zlib_decode_cases()
    args = ([c["stream"] for c in zs], [c["hist"] for c in zs], [len(c["want"]) + 5 for c in zs])
    plain = Decoded(ctx, *args, zlib_form=True, plain=True).results()
    assert Decoded(ctx, *args, zlib_form=True, told="null").results() == plain
    assert Decoded(ctx, *args, zlib_form=True, told=[0] * len(zs)).results() == plain
    assert plain[3][:3] == [K.E_ZLIB_DICT] * 3


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_zlib_decode_cases(ctx, device):
    cs = K.zlib_decode_cases()
    d = Decoded(ctx, [c["stream"] for c in cs], [c["hist"] for c in cs], [len(c["want"]) + 5 for c in cs], zlib_form=True,
                dict_id=[c["dict_id"] for c in cs], told=[c["told"] for c in cs], misalign=[3 * i for i in range(len(cs))], device=device)
    assert d.clean
    for i, c in enumerate(cs):
        assert d.status[i] == c["status"] and d.outputs[i] == c["want"], (c["name"], d.status[i])
        assert d.in_used[i] == (len(c["stream"]) if c["in_used"] is None else c["in_used"]), c["name"]


# ------------------------------------------------------------------------------------------------------------------ scale, methods
def test_4096_records_behind_one_dictionary(ctx):
    n, rl = 4096, 2048
    dic = K.text(32768, 99)
    recs = K.text(n * rl, 1234)
    one = np.frombuffer(dic, np.uint8)
    inb = np.zeros(n * (32768 + rl) + 16, np.uint8)
    img = inb[:n * (32768 + rl)].reshape(n, 32768 + rl)
    img[:, :32768] = one
    img[:, 32768:] = np.frombuffer(recs, np.uint8).reshape(n, rl)
    off = [k * (32768 + rl) + 32768 for k in range(n)]
    e = Encoded(ctx, inb, off, [rl] * n, [32768] * n, 6)
    assert not e.status.any() and e.untouched_outside()
    alone = Encoded(ctx, inb, off, [rl] * n, None, 6)
    assert int(e.out_len.sum()) < 0.8 * int(alone.out_len.sum())
    for k in range(n):
        assert zlib.decompressobj(-15, zdict=dic).decompress(e.outputs[k]) == recs[k * rl:(k + 1) * rl], k
    # back through rcx_inflate_hist_batch: the input image is the output image, the records' slots wiped
    streams = np.frombuffer(b"".join(e.outputs) + b"\0" * 16, np.uint8)
    in_len = e.out_len.copy()
    in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.uint64)
    out = inb.copy()
    out[:n * (32768 + rl)].reshape(n, 32768 + rl)[:, 32768:] = SENT
    out_off, out_cap, hl = np.array(off, np.uint64), np.full(n, rl, np.uint64), np.full(n, 32768, np.uint64)
    out_len, in_used, status, flags = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32), np.zeros(n, np.uint32)
    b = N.Batch(_p(streams), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_HOST)
    ctx._chk(N.lib().rcx_inflate_hist_batch(ctx._h, C.byref(b), C.c_void_p(_p(flags)), C.c_void_p(_p(hl))))
    assert not status.any() and (out == inb).all() and (in_used == in_len).all()


def test_python_methods(ctx, sim):
    B = K.batch()
    pick = [B.index(nm) for nm in ("h4096 n1000", "h32768 n65536", "slice first", "run", "h0 n1000", "h5 n0")]
    blocks, hists = [B.block(i) for i in pick], [B.history(i) or None for i in pick]
    res = ctx.deflate_encode_hist_blocks(blocks, hists, level=9).check()
    assert res.outputs == [sim[0][9][1][i] for i in pick]
    assert ctx.inflate_hist_blocks(res.outputs, hists, [len(b) for b in blocks]).check().outputs == blocks
    # zdict as Python's zlib takes it: one (long) dictionary for all, or one per blob
    dic = K.rand(3000, 5) + K.text(40000, 6)
    recs = [K.text(2048, s) for s in range(8)] + [b""]
    z = ctx.zlib_encode(recs, level=6, zdict=dic).check()
    for o, r in zip(z.outputs, recs):
        assert zlib.decompressobj(zdict=dic).decompress(o) == r
    assert ctx.zlib_decode(z.outputs, [len(r) for r in recs], zdict=dic).check().outputs == recs
    theirs = []
    for r in recs:
        c = zlib.compressobj(9, zdict=dic)
        theirs.append(c.compress(r) + c.flush())
    assert ctx.zlib_decode(theirs, [len(r) for r in recs], zdict=dic).check().outputs == recs
    per = [dic, None, K.text(100, 7)] + [dic] * 6
    z2 = ctx.zlib_encode(recs, level=2, zdict=per).check()
    assert not z2.outputs[1][1] & 0x20 and z2.outputs[1] == ctx.zlib_encode([recs[1]], level=2).outputs[0]
    assert ctx.zlib_decode(z2.outputs, [len(r) for r in recs], zdict=per).check().outputs == recs
    wrong = ctx.zlib_decode(z.outputs[:2], [2048] * 2, zdict=dic[1:])
    assert list(wrong.status) == [K.E_ZLIB_DICT_ID] * 2 and not wrong.out_len.any()
    assert ctx.zlib_encode(recs, level=6).outputs == ctx.zlib_encode(recs, level=6, zdict=None).outputs      # (the default keeps today's bytes)
