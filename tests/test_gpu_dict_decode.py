"""GPU suite of the decoders behind shared dictionaries (rcx_lz4_decode_shared_batch, rcx_inflate_shared_batch,
rcx_zlib_decode_shared_batch; k_lz4_dict.hip, k_inflate_dict.hip): the batches of tests/dict_decode_cases.py against the wave simulator's
results, from host and from device memory; against the history calls on the replicated layout, on the device too; a round trip of 4096
records behind one dictionary through the shared encoders; the Python methods; the refusals."""
import ctypes as C
import zlib

import numpy as np
import pytest

import dict_decode_cases as DC
from rust_compress_amd import _native as N
from rust_compress_amd import synth

pytestmark = pytest.mark.gpu

SENT = 0x5A
FN = {"lz4": "rcx_lz4_decode_shared_batch", "deflate": "rcx_inflate_shared_batch", "zlib": "rcx_zlib_decode_shared_batch"}
HIST_FN = {"lz4": "rcx_lz4_decode_linked_batch", "deflate": "rcx_inflate_hist_batch", "zlib": "rcx_zlib_decode_dict_batch"}


def _p(a):
    return a.ctypes.data if a is not None else None


def _call(ctx, kind, fn, inb, in_off, lens, out, out_off, caps, extra, device, expect=N.RC_OK):
    """one decode call -> the results in the form of sim_dict_decode_run.run's; extra: the arrays behind the batch (None: a NULL)"""
    n = len(lens)
    a_off, a_len = np.array(list(in_off) or [0], np.uint64), np.array(list(lens) or [0], np.uint64)
    o_off, o_cap = np.array(list(out_off) or [0], np.uint64), np.array(list(caps) or [0], np.uint64)
    out_len, in_used, status = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.full(max(n, 1), -99, np.int32)
    flags = np.zeros(max(n, 1), np.uint32)
    inb = np.ascontiguousarray(inb)
    if device:
        import torch
        d_in, d_out = torch.from_numpy(inb.copy()).cuda(), torch.from_numpy(out).cuda()
        b = N.Batch(d_in.data_ptr(), _p(a_off), _p(a_len), d_out.data_ptr(), _p(o_off), _p(o_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_DEVICE)
    else:
        b = N.Batch(_p(inb), _p(a_off), _p(a_len), _p(out), _p(o_off), _p(o_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_HOST)
    args = [ctx._h, C.byref(b)] + ([C.c_void_p(_p(flags))] if kind != "lz4" else []) + [C.c_void_p(_p(x)) for x in extra]
    rc = getattr(N.lib(), fn)(*args)
    err = N.lib().rcx_last_error(ctx._h).decode()
    assert rc == expect, (rc, err)
    res = d_out.cpu().numpy() if device else out
    return dict(rc=rc, err=err, status=status[:n], out_len=out_len[:n], in_used=in_used[:n], flags=flags[:n], out=res,
                outputs=[bytes(res[int(o):int(o) + int(l)]) for o, l in zip(o_off[:n], out_len[:n])])


def shared_call(ctx, B, device=False):
    inb, in_off, lens, d_off, d_len = B.layout()
    out_off, caps, size = B.slots()
    extra = [np.array(d_off, np.uint64), np.array(d_len, np.uint64)] + ([np.array(B.ids, np.uint32)] if B.kind == "zlib" else [])
    return _call(ctx, B.kind, FN[B.kind], inb, in_off, lens, np.full(size, SENT, np.uint8), out_off, caps, extra, device)


def hist_call(ctx, B, device=True):
    """the history call on the replicated layout: every stream's dictionary directly in front of its slot -> DC.hist_results' form"""
    n = len(B.blocks)
    in_len = [len(s) for s in B.blocks]
    in_off = list(np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.int64))
    inb = np.frombuffer(b"".join(B.blocks) + b"\0" * 16, np.uint8)
    img, out_off = bytearray(b"\x5A" * 16), []
    for i in range(n):
        img += B.front(i) + B.dictionary(i)
        out_off.append(len(img))
        img += b"\x5A" * (B.caps[i] + 3)
    out = np.frombuffer(bytes(img) + b"\x5A" * 16, np.uint8).copy()
    dl = np.array([len(B.dictionary(i)) for i in range(n)], np.uint64)
    extra = [np.zeros(n, np.uint8), dl] if B.kind == "lz4" else [dl] + ([np.array(B.ids, np.uint32)] if B.kind == "zlib" else [])
    r = _call(ctx, B.kind, HIST_FN[B.kind], inb, in_off, in_len, out, out_off, B.caps, extra, device)
    return r["status"], r["out_len"], r["in_used"], r["flags"] if B.kind != "lz4" else None, r["outputs"]


def _batches():
    """name -> batch: the case batches, the sharing batch in two orders, the 8200 blocks, the corrupted corpus, per family"""
    bs = {}
    for f in DC.FAMILIES:
        for k, B in enumerate(DC.case_batches(f)):
            bs["%s cases %d" % (f, k)] = B
        bs[f + " sharing"] = DC.sharing(f, 0)
        bs[f + " sharing reversed"] = DC.sharing(f, 1)
        bs[f + " many"] = DC.many(f)
        bs[f + " corrupted"] = DC.corrupted(f)
    return bs


NAMES = ["%s %s" % (f, w) for f in DC.FAMILIES for w in ("cases 0", "cases 1", "cases 2", "sharing", "sharing reversed", "many", "corrupted")] + ["deflate cases 3"]


@pytest.fixture(scope="module")
def batches():
    bs = _batches()
    assert sorted(bs) == sorted(NAMES)
    return bs


@pytest.fixture(scope="module")
def sim(batches):
    """the simulator's results of every batch.  The simulator's workers are forked by an interpreter of their own (this process holds
    the GPU), a fixed number of them."""
    import sim_dict_decode_run as DR
    res = dict(zip(batches, DR.run_many([DC.shared_job(B) for B in batches.values()], fresh=True)))
    assert all(r["rc"] == 0 for r in res.values())
    return res


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_batches_equal_the_simulator(ctx, batches, sim, name, device):
    B, s = batches[name], sim[name]
    got = shared_call(ctx, B, device)
    DC.check(B, got, (s["status"], s["out_len"], s["in_used"], s["flags"] if B.kind != "lz4" else None, s["outputs"]))
    if name.endswith("corrupted"):
        assert int((got["status"] != 0).sum()) >= 20 and int((got["status"] == 0).sum()) >= 150


@pytest.mark.parametrize("name", NAMES)
def test_the_history_calls_on_the_replicated_layout_give_the_same_results(ctx, batches, name):
    B = batches[name]
    DC.check(B, shared_call(ctx, B, True), hist_call(ctx, B, True))


def test_results_do_not_depend_on_the_order(ctx, batches):
    for f in DC.FAMILIES:
        a, z = shared_call(ctx, batches[f + " sharing"]), shared_call(ctx, batches[f + " sharing reversed"], True)
        assert a["outputs"] == z["outputs"][::-1] and not a["status"].any() and not z["status"].any()


# ------------------------------------------------------------------------------------------------------------------ the workload
@pytest.mark.parametrize("form", ["lz4", "deflate", "zlib"])
def test_4096_records_behind_one_dictionary_round_trip(ctx, form):
    recs = [synth.gen("text", 2048, 1000 + s).tobytes() for s in range(64)]
    recs = [recs[(i * 7) % 64][i % 5:] + recs[i % 64][:i % 5] for i in range(4096)]          # 4096 records of 2 KiB, all different
    dct = synth.gen("text", 32768, 99).tobytes()
    caps = [2048] * len(recs)
    if form == "lz4":
        enc = ctx.lz4_encode_hc_dict_blocks(recs, dct, 9).check()
        dec = ctx.lz4_decode_dict_blocks(enc.outputs, dct, caps).check()
    elif form == "deflate":
        enc = ctx.deflate_encode_dict_blocks(recs, dct, 6).check()
        dec = ctx.inflate_dict_blocks(enc.outputs, dct, caps).check()
    else:
        enc = ctx.zlib_encode(recs, level=6, zdict=dct, shared=True).check()
        dec = ctx.zlib_decode(enc.outputs, caps, zdict=dct, shared=True).check()
    assert dec.outputs == recs
    assert [int(u) for u in dec.in_used] == [len(o) for o in enc.outputs]


def test_the_public_methods_equal_the_history_methods(ctx):
    recs = [synth.gen("text", 1500, s).tobytes() for s in range(6)]
    d1, d2 = synth.gen("text", 5000, 50).tobytes(), synth.gen("text", 70000, 51).tobytes()
    dicts = [d1, None, d2, d1, d2, None]
    caps = [1500] * 6

    def same(a, b):
        assert a.outputs == b.outputs == recs and list(a.status) == list(b.status) and list(a.in_used) == list(b.in_used)
        assert list(a.out_len) == list(b.out_len) and (a.aux is None or list(a.aux) == list(b.aux))
    z = ctx.zlib_encode(recs, level=9, zdict=dicts).check().outputs
    same(ctx.zlib_decode(z, caps, zdict=dicts, shared=True), ctx.zlib_decode(z, caps, zdict=dicts))
    d = ctx.deflate_encode_hist_blocks(recs, dicts, 6).check().outputs
    same(ctx.inflate_dict_blocks(d, dicts, caps), ctx.inflate_hist_blocks(d, dicts, caps))
    l = ctx.lz4_encode_hc_hist_blocks(recs, dicts, 9).check().outputs
    got = ctx.lz4_decode_dict_blocks(l, dicts, caps).check()
    assert got.outputs == recs and [int(u) for u in got.in_used] == [len(x) for x in l]
    one = ctx.lz4_decode_dict_blocks([l[0], l[3]], d1, [1500, 1500]).check()
    assert one.outputs == [recs[0], recs[3]]
    # a wrong dictionary: the zlib form says so, stream by stream
    bad = ctx.zlib_decode(z, caps, zdict=[d2, None, d2, d1, d1, None], shared=True)
    assert [int(s) for s in bad.status] == [25, 0, 0, 0, 25, 0]
    with pytest.raises(ValueError):
        ctx.inflate_dict_blocks(d, [d1], caps)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", ["lz4", "deflate", "zlib"])
def test_bad_arguments_are_refused(ctx, form):
    fam = "lz4" if form == "lz4" else "deflate"
    most = 65536 if form == "lz4" else 32768
    t = synth.gen("text", 5000, 3).tobytes()
    blocks = [t[:2000], t[2000:]]
    if form == "lz4":
        streams = ctx.lz4_encode_hc_blocks(blocks, 9).check().outputs
    else:
        streams = [zlib.compress(b, 6) if form == "zlib" else DC.DH.libz_stream(b"", b, 6) for b in blocks]
    inb = np.frombuffer(b"\xC3" * 100000 + b"".join(streams) + b"\0" * 16, np.uint8)
    off, lens = [100000, 100000 + len(streams[0])], [len(s) for s in streams]
    out_off, caps = [0, 2005], [2000, 3000]
    ids = [np.array([1, 2], np.uint32)] if form == "zlib" else []
    u64 = lambda v: np.array(v, np.uint64)

    def call(extra, expect=N.RC_OK, device=False):
        return _call(ctx, form, FN[form], inb, off, lens, np.full(5100, SENT, np.uint8), out_off, caps, extra, device, expect)
    ok = call([u64([10, 10]), u64([most, most])] + ids)                                     # (the most a dictionary can be)
    assert not ok["status"].any() and ok["outputs"] == blocks
    e = call([u64([10, 10]), u64([0, most + 1])] + ids, N.RC_BAD_ARG)
    assert "block 1" in e["err"] and str(most) in e["err"]
    call([u64([10, 10]), None] + ids, N.RC_BAD_ARG)                                         # one array without the other
    call([None, u64([5, 5])] + ids, N.RC_BAD_ARG)
    if form == "zlib":
        call([u64([10, 10]), u64([5, 5]), None], N.RC_BAD_ARG)
    # both arrays NULL: the decoders without history; a length of 0 everywhere is no dictionary either, whatever the offsets say
    want = ctx.lz4_decode_blocks(streams, caps) if form == "lz4" else ctx.inflate(streams, caps) if form == "deflate" else ctx.zlib_decode(streams, caps)
    for extra in ([None, None] + ([None] if form == "zlib" else []), [u64([1 << 60, 7]), u64([0, 0])] + ids):
        for device in (False, True):
            r = call(extra, device=device)
            assert r["outputs"] == want.outputs == blocks and list(r["status"]) == list(want.status) and list(r["in_used"]) == list(want.in_used)
            assert form == "lz4" or list(r["flags"]) == list(want.aux)
