"""GPU suite of the encoders behind shared dictionaries (rcx_lz4_encode_hc_shared_batch, rcx_deflate_encode_shared_batch,
rcx_zlib_encode_shared_batch; k_lz4_hc_dict.hip, k_deflate_hc_dict.hip, lz_dict.h): the batches of tests/dict_shared_cases.py against the
wave simulator's bytes, from host and from device memory; against the history calls on the replicated layout, on the device too; a
round trip of 4096 records behind one dictionary through the existing decoders; the refusals."""
import ctypes as C
import zlib

import numpy as np
import pytest

import dict_shared_cases as K
import lz4_frame_ref as R
from rust_compress_amd import _native as N
from rust_compress_amd import synth

pytestmark = pytest.mark.gpu

SENT = 0xEE
FL = [(f, lv) for f in ("lz4", "deflate") for lv in K.LEVELS[f]]
FORMS = FL + [("zlib", lv) for lv in K.LEVELS["deflate"]]
FN = {"lz4": "rcx_lz4_encode_hc_shared_batch", "deflate": "rcx_deflate_encode_shared_batch", "zlib": "rcx_zlib_encode_shared_batch"}


def _p(a):
    return a.ctypes.data if a is not None else None


def _family(form):
    return "lz4" if form == "lz4" else "deflate"


def _caps(form, lens):
    return [K.bound(_family(form), int(n), 1 if form == "zlib" else 0) for n in lens]


class Encoded:
    """One *_shared_batch call over a laid-out buffer; the output slots lie in a buffer of sentinels"""

    def __init__(self, ctx, form, inb, in_off, lens, dict_off, dict_len, level, caps=None, dict_id=None, device=False, expect=N.RC_OK):
        n = len(lens)
        self.in_off, self.in_len = np.array(in_off, np.uint64), np.array(lens, np.uint64)
        self.out_cap = np.array(_caps(form, lens) if caps is None else caps, np.uint64)
        self.out_off = (np.concatenate([[0], np.cumsum(self.out_cap + np.uint64(3))[:-1]]) + 5).astype(np.uint64)
        out = np.full(int(self.out_off[-1] + self.out_cap[-1]) + 16, SENT, np.uint8)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        d_off = np.array(dict_off, np.uint64) if dict_off is not None else None
        d_len = np.array(dict_len, np.uint64) if dict_len is not None else None
        ids = np.array(dict_id if dict_id is not None else [0] * n, np.uint32)
        if device:
            import torch
            d_in, d_out = torch.from_numpy(np.ascontiguousarray(inb).copy()).cuda(), torch.from_numpy(out).cuda()
            b = N.Batch(d_in.data_ptr(), _p(self.in_off), _p(self.in_len), d_out.data_ptr(), _p(self.out_off), _p(self.out_cap),
                        _p(self.out_len), _p(self.in_used), _p(self.status), n, N.MEM_DEVICE)
        else:
            b = N.Batch(_p(inb), _p(self.in_off), _p(self.in_len), _p(out), _p(self.out_off), _p(self.out_cap), _p(self.out_len),
                        _p(self.in_used), _p(self.status), n, N.MEM_HOST)
        args = [ctx._h, C.byref(b), level, C.c_void_p(_p(d_off)), C.c_void_p(_p(d_len))]
        if form == "zlib":
            args.append(C.c_void_p(_p(ids) if dict_id is not None else None))
        self.rc = getattr(N.lib(), FN[form])(*args)
        self.error = N.lib().rcx_last_error(ctx._h).decode()
        assert self.rc == expect, (self.rc, self.error)
        self.out = d_out.cpu().numpy() if device else out
        self.outputs = [bytes(self.out[int(o):int(o) + int(l)]) for o, l in zip(self.out_off, self.out_len)]

    def untouched_outside(self):
        mask = np.ones(self.out.size, bool)
        for o, l in zip(self.out_off, self.out_len):
            mask[int(o):int(o) + int(l)] = False
        return bool((self.out[mask] == SENT).all())


def _batch(form):
    """the case batch of a form (the zlib form: K.zlib_subset of it, as the simulator suite runs it) and its DICTIDs"""
    B = K.cases(_family(form))
    if form == "zlib":
        B = B.reordered(K.zlib_subset(B))
    ids = [zlib.adler32(B.dictionary(i)) if B.of[i] is not None else 0 for i in range(len(B.blocks))] if form == "zlib" else None
    return B, ids


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.fixture(scope="module")
def sim():
    """the simulator's results of the case batches and of the sharing batch, per form and level.  The simulator's workers are forked by
    an interpreter of their own (this process holds the GPU), a fixed number of them."""
    import sim_dict_shared_run as S
    jobs = {}
    for form, lv in FORMS:
        B, ids = _batch(form)
        inb, in_off, lens, d_off, d_len = B.shared()
        kw = {"caps": B.out_caps(1 if form == "zlib" else 0)}
        if form == "zlib":
            kw.update(fmt=1, dict_id=ids)
        jobs[("cases", form, lv)] = ((_family(form), inb, in_off, lens, d_off, d_len, lv), kw)
    for f, lv in FL:
        inb, in_off, lens, d_off, d_len = K.sharing(f).shared()
        jobs[("sharing", f, lv)] = ((f, inb, in_off, lens, d_off, d_len, lv), {})
    res = dict(zip(jobs, S.run_many(list(jobs.values()), fresh=True)))
    assert all(r["rc"] == 0 for r in res.values())
    return res


@pytest.mark.parametrize("form,level,device", [(f, lv, dv) for dv in (False, True) for f, lv in FORMS],
                         ids=lambda v: str(v))
def test_cases_equal_the_simulator(ctx, sim, form, level, device):
    B, ids = _batch(form)
    inb, in_off, lens, d_off, d_len = B.shared()
    e = Encoded(ctx, form, inb, in_off, lens, d_off, d_len, level, B.out_caps(1 if form == "zlib" else 0), ids, device)
    s = sim[("cases", form, level)]
    small = B.index("small slot")
    assert list(e.status) == list(s["status"]) and e.status[small] == K.E_OUTPUT_TOO_SMALL and not np.delete(e.status, small).any()
    assert list(e.out_len) == list(s["out_len"]) and list(e.in_used) == list(s["in_used"])
    bad = [B.names[i] for i in range(len(lens)) if e.outputs[i] != s["outputs"][i]]
    assert not bad, bad
    assert e.untouched_outside()
    assert e.outputs[B.index("end bait x")] == e.outputs[B.index("end bait y")]
    assert e.outputs[B.index("front bait x")] == e.outputs[B.index("front bait y")]


@pytest.mark.parametrize("form,level", FORMS, ids=lambda v: str(v))
def test_the_history_calls_on_the_replicated_layout_give_the_same_bytes(ctx, form, level):
    B, ids = _batch(form)
    inb, in_off, lens, d_off, d_len = B.shared()
    keep = [i for i in range(len(lens)) if B.names[i] != "small slot"]
    e = Encoded(ctx, form, inb, in_off, lens, d_off, d_len, level, None, ids)
    blocks, hists = [B.blocks[i] for i in keep], [B.dictionary(i) or None for i in keep]
    if form == "lz4":
        want = ctx.lz4_encode_hc_hist_blocks(blocks, hists, level)
    elif form == "deflate":
        want = ctx.deflate_encode_hist_blocks(blocks, hists, level)
    else:
        want = ctx.zlib_encode(blocks, level=level, zdict=hists)
    assert not want.status.any() and not e.status.any()
    bad = [B.names[i] for k, i in enumerate(keep) if e.outputs[i] != want.outputs[k]]
    assert not bad, bad
    assert [int(e.in_used[i]) for i in keep] == [int(u) for u in want.in_used]


@pytest.mark.parametrize("family,level", FL, ids=lambda v: str(v))
def test_blocks_that_share_dictionaries(ctx, sim, family, level):
    B = K.sharing(family)
    e = Encoded(ctx, family, *B.shared(), level)
    assert not e.status.any() and e.outputs == sim[("sharing", family, level)]["outputs"]
    order = list(np.random.default_rng(11).permutation(len(B.blocks)))
    e2 = Encoded(ctx, family, *B.reordered(order).shared(), level, device=True)
    assert [e2.outputs[k] for k in np.argsort(order)] == e.outputs
    assert e.outputs[B.index("twin first")] != e.outputs[B.index("twin second")]


@pytest.mark.parametrize("family", ["lz4", "deflate"])
def test_more_work_items_than_the_grids_hold(ctx, family):
    """8200 segments for launches of 8192 workgroups at the most, 1030 distinct dictionaries for a build launch of 1024: every block is a
    copy of its 16-byte dictionary.  A block whose dictionary was not built or whose segment did not run cannot hold its match."""
    inb, in_off, lens, d_off, d_len = K.many(family)
    e = Encoded(ctx, family, inb, in_off, lens, d_off, d_len, K.LEVELS[family][1])
    assert not e.status.any()
    if family == "lz4":
        assert set(int(x) for x in e.out_len) == {9}             # one match of 11 bytes at distance 16, five literals
        assert all(R.block_decode(e.outputs[i], prefix=bytes(inb[d_off[i]:d_off[i] + 16])) == bytes(inb[in_off[i]:in_off[i] + 16])
                   for i in list(range(0, 8200, 97)) + list(range(8180, 8200)))
    else:
        assert int(e.out_len.max()) < 12                         # (16 random bytes alone take 18 and more)
        for i in list(range(0, 8200, 97)) + list(range(8180, 8200)):
            d = zlib.decompressobj(-15, zdict=bytes(inb[d_off[i]:d_off[i] + 16]))
            assert d.decompress(e.outputs[i]) == bytes(inb[in_off[i]:in_off[i] + 16])
    h = ctx.lz4_encode_hc_hist_blocks if family == "lz4" else ctx.deflate_encode_hist_blocks
    pick = list(range(0, 8200, 397)) + [1029, 1030, 8191, 8192, 8199]
    blocks = [bytes(inb[in_off[i]:in_off[i] + 16]) for i in pick]
    assert h(blocks, blocks, K.LEVELS[family][1]).outputs == [e.outputs[i] for i in pick]


# ------------------------------------------------------------------------------------------------------------------ the workload
@pytest.mark.parametrize("form", ["lz4", "deflate", "zlib"])
def test_4096_records_behind_one_dictionary_round_trip(ctx, form):
    recs = [synth.gen("text", 2048, 1000 + s).tobytes() for s in range(64)]
    recs = [recs[(i * 7) % 64][i % 5:] + recs[i % 64][:i % 5] for i in range(4096)]          # 4096 records of 2 KiB, all different
    dct = synth.gen("text", 32768, 99).tobytes()
    if form == "lz4":
        enc = ctx.lz4_encode_hc_dict_blocks(recs, dct, 9).check()
        n = len(recs)
        blob = b"".join(enc.outputs)
        in_len = np.array([len(o) for o in enc.outputs], np.uint64)
        in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.uint64)
        inb = np.frombuffer(blob + b"\0" * 16, np.uint8)
        stride = 32768 + 2048 + 16
        img = np.full(n * stride + 16, SENT, np.uint8)
        img.reshape(-1)[:n * stride].reshape(n, stride)[:, 16:16 + 32768] = np.frombuffer(dct, np.uint8)
        out_off = (np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(16 + 32768))
        out_cap, dlen = np.full(n, 2048, np.uint64), np.full(n, 32768, np.uint64)
        out_len, in_used, status, link = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
        b = N.Batch(_p(inb), _p(in_off), _p(in_len), _p(img), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_HOST)
        ctx._chk(N.lib().rcx_lz4_decode_linked_batch(ctx._h, C.byref(b), C.c_void_p(_p(link)), C.c_void_p(_p(dlen))))
        assert not status.any()
        dec = [bytes(img[int(o):int(o) + int(l)]) for o, l in zip(out_off, out_len)]
    elif form == "deflate":
        enc = ctx.deflate_encode_dict_blocks(recs, dct, 6).check()
        dec = ctx.inflate_hist_blocks(enc.outputs, [dct] * len(recs), [2048] * len(recs)).check().outputs
    else:
        enc = ctx.zlib_encode(recs, level=6, zdict=dct, shared=True).check()
        dec = ctx.zlib_decode(enc.outputs, [2048] * len(recs), zdict=dct).check().outputs
        d = zlib.decompressobj(zdict=dct)
        assert d.decompress(enc.outputs[77]) == recs[77]
    assert dec == recs
    plain = sum(len(o) for o in (ctx.lz4_encode_hc_blocks(recs[:64], 9) if form == "lz4" else ctx.deflate_encode(recs[:64], level=6)).outputs)
    behind = sum(len(o) for o in enc.outputs[:64]) - (10 * 64 if form == "zlib" else 0)
    print("%s: 64 records of 2 KiB: %d bytes behind the dictionary, %d without" % (form, behind, plain))
    assert behind < plain


def test_the_public_methods_lay_equal_dictionaries_out_once(ctx):
    recs = [synth.gen("text", 1500, s).tobytes() for s in range(6)]
    d1, d2 = synth.gen("text", 5000, 50).tobytes(), synth.gen("text", 70000, 51).tobytes()
    dicts = [d1, None, d2, d1, d2, None]
    assert ctx.lz4_encode_hc_dict_blocks(recs, dicts, 9).check().outputs == ctx.lz4_encode_hc_hist_blocks(recs, dicts, 9).check().outputs
    assert ctx.deflate_encode_dict_blocks(recs, dicts, 6).check().outputs == ctx.deflate_encode_hist_blocks(recs, dicts, 6).check().outputs
    assert ctx.zlib_encode(recs, level=9, zdict=dicts, shared=True).check().outputs == ctx.zlib_encode(recs, level=9, zdict=dicts).check().outputs
    assert ctx.lz4_encode_hc_dict_blocks(recs, d1, 3).check().outputs == ctx.lz4_encode_hc_hist_blocks(recs, [d1] * 6, 3).check().outputs
    with pytest.raises(ValueError):
        ctx.deflate_encode_dict_blocks(recs, [d1], 6)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", ["lz4", "deflate", "zlib"])
def test_bad_arguments_are_refused(ctx, form):
    t = synth.gen("text", 5000, 3).tobytes()
    inb = np.frombuffer(b"\xC3" * 100000 + t + b"\0" * 16, np.uint8)
    off, lens = [100000, 102000], [2000, 3000]
    most = K.MAX_DICT[_family(form)]
    lv = 9
    ids = [1, 2] if form == "zlib" else None
    ok = Encoded(ctx, form, inb, off, lens, [10, 10], [most, most], lv, dict_id=ids)                # (the most a dictionary can be)
    assert not ok.status.any()
    e = Encoded(ctx, form, inb, off, lens, [10, 10], [0, most + 1], lv, dict_id=ids, expect=N.RC_BAD_ARG)
    assert "block 1" in e.error and str(most) in e.error
    Encoded(ctx, form, inb, off, lens, [10, 10], None, lv, dict_id=ids, expect=N.RC_BAD_ARG)        # one array without the other
    Encoded(ctx, form, inb, off, lens, None, [5, 5], lv, dict_id=ids, expect=N.RC_BAD_ARG)
    if form == "zlib":
        Encoded(ctx, form, inb, off, lens, [10, 10], [5, 5], lv, dict_id=None, expect=N.RC_BAD_ARG)
    for level in ((0, 13, -1) if form == "lz4" else (0, 1, 10, -1)):
        Encoded(ctx, form, inb, off, lens, [10, 10], [5, 5], level, dict_id=ids, expect=N.RC_BAD_ARG)
        Encoded(ctx, form, inb, off, lens, None, None, level, dict_id=ids, expect=N.RC_BAD_ARG)
    # both arrays NULL: the encoders without history
    e = Encoded(ctx, form, inb, off, lens, None, None, lv, dict_id=ids)
    blocks = [t[:2000], t[2000:]]
    want = ctx.lz4_encode_hc_blocks(blocks, lv) if form == "lz4" else ctx.deflate_encode(blocks, level=lv) if form == "deflate" else ctx.zlib_encode(blocks, level=lv)
    assert e.outputs == want.outputs and not e.status.any()
    # a length of 0 everywhere is no dictionary either, whatever the offsets say
    e0 = Encoded(ctx, form, inb, off, lens, [1 << 60, 7], [0, 0], lv, dict_id=ids)
    assert e0.outputs == want.outputs
