"""GPU suite of the LZ4 HC encoder with history (rcx_lz4_encode_hc_hist_batch, k_lz4_hc_hist.hip) and of the linked / dictionary frames
rust_compress_amd.lz4frame writes with it: the cases of tests/lz4_hist_cases.py against the wave simulator's bytes and this library's
linked decoder, hist_len NULL against rcx_lz4_encode_hc_batch, the sizes a history must buy, and encode_frames against decode_frames,
the plain-Python reference (tests/lz4_frame_ref.py) and -- where ctypes finds it -- liblz4."""
import ctypes as C
import io
import itertools
import struct

import numpy as np
import pytest

import hc_inputs
import hc_stages as H
import lz4_frame_inputs as I
import lz4_frame_ref as R
import lz4_hist_cases as K
from rust_compress_amd import _native as N
from rust_compress_amd import lz4frame as F
from rust_compress_amd import synth

pytestmark = pytest.mark.gpu

SENT = 0xEE
LEVELS = K.LEVELS


def _p(a):
    return a.ctypes.data if a is not None else None


def _bound(n):
    return int(N.lib().rcx_lz4_compression_bound(n))


class Encoded:
    """One rcx_lz4_encode_hc_hist_batch call over a laid-out buffer; the output slots lie in a buffer of sentinels"""

    def __init__(self, ctx, inb, in_off, lens, hist_len, level, caps=None, device=False, expect=N.RC_OK):
        n = len(lens)
        self.in_off, self.in_len = np.array(in_off, np.uint64), np.array(lens, np.uint64)
        caps = [_bound(int(l)) for l in lens] if caps is None else caps
        self.out_cap = np.array(caps, np.uint64)
        self.out_off = (np.concatenate([[0], np.cumsum(self.out_cap + np.uint64(3))[:-1]]) + 5).astype(np.uint64)
        out = np.full(int(self.out_off[-1] + self.out_cap[-1]) + 16, SENT, np.uint8)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        hist = np.array(hist_len, np.uint64) if hist_len is not None else None
        if device:
            import torch
            d_in, d_out = torch.from_numpy(np.ascontiguousarray(inb).copy()).cuda(), torch.from_numpy(out).cuda()
            b = N.Batch(d_in.data_ptr(), _p(self.in_off), _p(self.in_len), d_out.data_ptr(), _p(self.out_off), _p(self.out_cap),
                        _p(self.out_len), _p(self.in_used), _p(self.status), n, N.MEM_DEVICE)
        else:
            b = N.Batch(_p(inb), _p(self.in_off), _p(self.in_len), _p(out), _p(self.out_off), _p(self.out_cap), _p(self.out_len),
                        _p(self.in_used), _p(self.status), n, N.MEM_HOST)
        self.rc = N.lib().rcx_lz4_encode_hc_hist_batch(ctx._h, C.byref(b), level, C.c_void_p(_p(hist)))
        self.error = N.lib().rcx_last_error(ctx._h).decode()
        assert self.rc == expect, (self.rc, self.error)
        self.out = d_out.cpu().numpy() if device else out
        self.outputs = [bytes(self.out[int(o):int(o) + int(l)]) for o, l in zip(self.out_off, self.out_len)]

    def untouched_outside(self):
        mask = np.ones(self.out.size, bool)
        for o, l in zip(self.out_off, self.out_len):
            mask[int(o):int(o) + int(l)] = False
        return bool((self.out[mask] == SENT).all())


def _decode_behind_histories(ctx, blocks, hists, lens):
    """every block through rcx_lz4_decode_linked_batch as a chain head with dict_len = its history's length and the history in front
    of its slot -> the decoded blocks"""
    n = len(blocks)
    buf, in_off = bytearray(), np.zeros(n, np.uint64)
    for i, b in enumerate(blocks):
        in_off[i] = len(buf)
        buf += b
    inb = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8)
    in_len = np.array([len(b) for b in blocks], np.uint64)
    img, out_off, out_cap, dlen = bytearray(), np.zeros(n, np.uint64), np.array([max(l, 1) for l in lens], np.uint64), np.zeros(n, np.uint64)
    for i in range(n):
        img += bytes([SENT]) * 8 + hists[i]
        dlen[i] = len(hists[i])
        out_off[i] = len(img)
        img += bytes([SENT]) * max(lens[i], 1)
    out = np.frombuffer(bytes(img) + bytes([SENT]) * 16, np.uint8).copy()
    out_len, in_used, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    link = np.zeros(n, np.uint8)
    b = N.Batch(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_HOST)
    ctx._chk(N.lib().rcx_lz4_decode_linked_batch(ctx._h, C.byref(b), C.c_void_p(_p(link)), C.c_void_p(_p(dlen))))
    assert not status.any(), list(np.flatnonzero(status))
    return [bytes(out[int(o):int(o) + int(l)]) for o, l in zip(out_off, out_len)]


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.fixture(scope="module")
def sim():
    """the simulator's bytes of the batch, per level"""
    import sim_lz4hist_run as S
    B = K.batch()
    inb = B.array()
    jobs = [("run", (inb, B.in_off, B.lens, B.hist_len, lv), {"caps": B.caps}) for lv in sorted(LEVELS, reverse=True)]
    res = dict(zip(sorted(LEVELS, reverse=True), S.run_many(jobs)))
    assert all(r[0] == 0 for r in res.values())
    return res


@pytest.mark.parametrize("level,device", [(1, False), (9, False), (12, False), (9, True)], ids=["1-host", "9-host", "12-host", "9-device"])
def test_cases_equal_the_simulator_and_decode_behind_their_histories(ctx, sim, level, device):
    B = K.batch()
    e = Encoded(ctx, B.array(), B.in_off, B.lens, B.hist_len, level, B.caps, device)
    rc, outs, st, out_len, in_used, _ = sim[level]
    small = B.index("small slot")
    assert list(e.status) == list(st) and e.status[small] == N.E_OUTPUT_TOO_SMALL and not np.delete(e.status, small).any()
    assert list(e.out_len) == list(out_len) and list(e.in_used) == list(in_used)
    bad = [B.names[i] for i in range(len(outs)) if e.outputs[i] != outs[i]]
    assert not bad, bad
    assert e.untouched_outside()
    keep = [i for i in range(len(outs)) if i != small]
    dec = _decode_behind_histories(ctx, [e.outputs[i] for i in keep], [B.history(i) for i in keep], [B.lens[i] for i in keep])
    assert dec == [B.block(i) for i in keep]
    assert e.outputs[B.index("bait x")] == e.outputs[B.index("bait y")]


def test_the_public_method_builds_the_same_buffer(ctx, sim):
    B = K.batch()
    pick = [B.index(nm) for nm in ("h4096 n1000", "h65536 n65536", "slice first", "run", "h0 n1000", "h5 n0")]
    res = ctx.lz4_encode_hc_hist_blocks([B.block(i) for i in pick], [B.history(i) or None for i in pick], level=9).check()
    assert res.outputs == [sim[9][1][i] for i in pick]
    assert [int(u) for u in res.in_used] == [B.lens[i] for i in pick]


@pytest.mark.parametrize("level", LEVELS)
def test_without_history_every_result_is_the_hc_encoders(ctx, level):
    cases = hc_inputs.window_cases(H.HC_WIN, 1) + hc_inputs.group_cases() + hc_inputs.length_cases(H.HC_MAXM, H.HC_RING, 1) \
        + hc_inputs.end_cases() + hc_inputs.small_cases() + hc_inputs.size_cases() + hc_inputs.synth_cases()
    raws = [c.raw for c in cases]
    caps = [_bound(len(r)) for r in raws]
    caps[3] -= 1                                                       # (a status that is not 0)
    want = ctx.lz4_encode_hc_blocks(raws, level, caps)
    assert want.status[3] == N.E_OUTPUT_TOO_SMALL
    buf, off = bytearray(), []
    for r in raws:
        buf += b"\xC3" * 3
        off.append(len(buf))
        buf += r
    inb = np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8)
    for hist in (None, [0] * len(raws)):
        e = Encoded(ctx, inb, off, [len(r) for r in raws], hist, level, caps)
        assert e.outputs == want.outputs
        assert list(e.status) == list(want.status) and list(e.out_len) == list(want.out_len) and list(e.in_used) == list(want.in_used)


def test_more_work_items_than_the_largest_grid(ctx):
    """8200 blocks of 16 bytes, each a copy of the 16 bytes of history in front of it: 8200 segments and 8200 history passes for a grid
    of 8192 workgroups.  A block whose history pass did not run cannot hold a match."""
    n = 8200
    rec = [K.rand(16, 500 + i) for i in range(n)]
    inb = np.frombuffer(b"".join(r + r for r in rec) + b"\0" * 16, np.uint8)
    e = Encoded(ctx, inb, [32 * i + 16 for i in range(n)], [16] * n, [16] * n, 9)
    assert not e.status.any()
    # 16 bytes behind themselves: one match of 11 bytes at distance 16 (the last 5 bytes are literals): 1 + 2 + 1 + 5 bytes
    assert set(int(x) for x in e.out_len) == {9}
    assert all(R.block_decode(o, prefix=r) == r for o, r in zip(e.outputs[::97] + e.outputs[-9:], rec[::97] + rec[-9:]))
    assert all(H.lz4_block_tokens(o)[0][1:] == (0, 11, 16) for o in e.outputs)


def test_bad_arguments_are_refused(ctx):
    t = synth.gen("text", 5000, 3).tobytes()
    inb = np.frombuffer(b"\xC3" * 100000 + t + b"\0" * 16, np.uint8)
    off, lens = [100000, 102000], [2000, 3000]
    Encoded(ctx, inb, off, lens, [65536, 65536], 9)                                          # (the most a history can be)
    e = Encoded(ctx, inb, off, lens, [0, 65537], 9, expect=N.RC_BAD_ARG)
    assert "block 1" in e.error
    e = Encoded(ctx, inb, [100, 102000], [2000, 3000], [101, 0], 9, expect=N.RC_BAD_ARG)     # more than lies in front of the block
    assert "block 0" in e.error
    for level in (0, 13, -1):
        Encoded(ctx, inb, off, lens, [10, 10], level, expect=N.RC_BAD_ARG)
        Encoded(ctx, inb, off, lens, None, level, expect=N.RC_BAD_ARG)
    with pytest.raises(ValueError):
        ctx.lz4_encode_hc_hist_blocks([b"a", b"b"], [None], 9)


# ------------------------------------------------------------------------------------------------------------------ what a history buys
@pytest.mark.parametrize("level", LEVELS)
def test_every_record_is_smaller_behind_a_dictionary(ctx, level):
    recs = [synth.gen("text", 2048, s).tobytes() for s in range(16)]
    dct = synth.gen("text", 32768, 99).tobytes()
    with_d = ctx.lz4_encode_hc_hist_blocks(recs, [dct] * 16, level).check()
    without = ctx.lz4_encode_hc_blocks(recs, level).check()
    sizes = [(len(a), len(b)) for a, b in zip(with_d.outputs, without.outputs)]
    print("level %d: with / without a dictionary: %s" % (level, sizes))
    assert all(a < b for a, b in sizes), sizes
    assert _decode_behind_histories(ctx, with_d.outputs, [dct] * 16, [2048] * 16) == recs


def test_linked_blocks_are_smaller_than_independent_ones(ctx):
    data = synth.gen("text", 4 * 65536 + 1000, 5).tobytes()
    inb = np.frombuffer(data + b"\0" * 16, np.uint8)
    off = [k * 65536 for k in range(5)]
    lens = [65536] * 4 + [1000]
    linked = Encoded(ctx, inb, off, lens, [min(o, 65536) for o in off], 9)
    indep = Encoded(ctx, inb, off, lens, None, 9)
    assert not linked.status.any() and not indep.status.any()
    a, b = int(linked.out_len.sum()), int(indep.out_len.sum())
    print("five linked blocks %d bytes, independent %d" % (a, b))
    assert a < b
    assert linked.outputs[0] == indep.outputs[0]
    # the chain decodes as one linked chain
    blob = R.build([(False, o) for o in linked.outputs], 4, False, False, None, len(data))
    assert F.decode_frames([blob]) == [data]


# ------------------------------------------------------------------------------------------------------------------ frames
def _lz4f_decompress_using_dict(lz4, blob, dictionary):
    """LZ4F_decompress_usingDict of a whole frame -> bytes, or None where this liblz4 does not export it"""
    if not hasattr(lz4, "LZ4F_decompress_usingDict"):
        return None
    lz4.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lz4.LZ4F_createDecompressionContext.restype = C.c_size_t
    fn = lz4.LZ4F_decompress_usingDict
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.c_void_p]
    lz4.LZ4F_isError.argtypes = [C.c_size_t]
    lz4.LZ4F_getErrorName.argtypes = [C.c_size_t]
    lz4.LZ4F_getErrorName.restype = C.c_char_p
    lz4.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    d = C.c_void_p()
    assert not lz4.LZ4F_isError(lz4.LZ4F_createDecompressionContext(C.byref(d), 100))
    out, dst, pos = bytearray(), C.create_string_buffer(1 << 20), 0
    dbuf = C.create_string_buffer(dictionary, len(dictionary))
    try:
        while True:
            dn, sn = C.c_size_t(len(dst)), C.c_size_t(len(blob) - pos)
            src = C.create_string_buffer(blob[pos:], len(blob) - pos) if pos < len(blob) else None
            r = fn(d, dst, C.byref(dn), src, C.byref(sn), dbuf, len(dictionary), None)
            if lz4.LZ4F_isError(r):
                raise ValueError(lz4.LZ4F_getErrorName(r).decode())
            out += dst.raw[:dn.value]
            pos += sn.value
            if r == 0 and pos >= len(blob):
                return bytes(out)
            if dn.value == 0 and sn.value == 0:
                raise ValueError("truncated")
    finally:
        lz4.LZ4F_freeDecompressionContext(d)


def _frame_blobs():
    rnd = K.rand(70000, 41)
    return [b"", b"a", synth.gen("text", 65536, 42).tobytes(), synth.gen("words", 65537, 43).tobytes(), synth.gen("text", 200000, 44).tobytes(),
            K.rand(150000, 45),                          # incompressible: stored blocks
            rnd + rnd[60000:65536]]                      # a stored first block, and a second one that ends with the first's last bytes


DICT = synth.gen("text", 70000, 46).tobytes()           # (its last 64 KiB count)


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("dictionary", [False, True], ids=["nodict", "dict"])
@pytest.mark.parametrize("linked", [False, True], ids=["independent", "linked"])
def test_frames_round_trip_through_every_reader(ctx, linked, dictionary, level):
    lz4 = I.load_lib("lz4")
    raws = _frame_blobs()
    dct = DICT if dictionary else None
    for bc, bs in itertools.product([False, True], [64 << 10, 256 << 10]):
        enc = F.encode_frames(raws, level=level, block_size=bs, block_checksum=bc, linked=linked, dictionary=dct)
        assert F.decode_frames(enc, dictionary=dct) == raws
        for e, r in zip(enc, raws):
            f = R.parse(e)
            assert len(f) == 1 and f[0].independent == (not linked) and f[0].block_checksum == bc and f[0].block_max == bs
            assert f[0].content_size == len(r) and f[0].dict_id is None
            assert R.decode(e, dictionary=dct) == r
            if lz4 is not None:
                got = _lz4f_decompress_using_dict(lz4, e, dct) if dct else I.lz4f_decompress(lz4, e)
                assert got is None or got == r
        assert all(s for s, _, _ in R.parse(enc[5])[0].blocks)                       # incompressible: stored, also in a linked frame
        if bs == 64 << 10:
            t = R.parse(enc[6])[0].blocks
            assert t[0][0] and t[1][0] != linked                                     # the second block compresses only behind the stored first
            assert not linked or R.block_uses_history(t[1][1])
        if linked or dictionary:                                                     # (text: a history makes it smaller)
            plain = F.encode_frames(raws[2:5], level=level, block_size=bs, block_checksum=bc)
            assert sum(map(len, enc[2:5])) <= sum(map(len, plain))
            assert dictionary or bs > 64 << 10 or len(enc[4]) < len(plain[2])         # (linked alone: where the blob has several blocks)
            assert not dictionary or all(len(a) < len(b) for a, b in zip(enc[2:5], plain))


def test_header_bytes_of_a_linked_frame_with_a_dictionary_id(ctx):
    e = F.encode_frames([b"hello"], level=1, linked=True, dictionary=b"hello world", dict_id=0x12345678, content_checksum=False, content_size=False)[0]
    # magic | FLG: version 01, B.Indep 0, no checksums, no size, dictID 1 | BD: 64 KiB | dictID | HC
    assert e[:11] == bytes([0x04, 0x22, 0x4D, 0x18, 0x41, 0x40, 0x78, 0x56, 0x34, 0x12, R.header_checksum(b"\x41\x40\x78\x56\x34\x12")])
    e = F.encode_frames([b"hello"], level=1, linked=True, dict_id=7)[0]
    assert e[4:6] == bytes([0x4D, 0x40]) and e[6:14] == struct.pack("<Q", 5) and e[14:18] == struct.pack("<I", 7)
    f = R.parse(e)[0]
    assert f.dict_id == 7 and not f.independent and R.decode(e) == b"hello"
    assert F.decode_frames([e], dictionary=b"x") == [b"hello"]


@pytest.mark.parametrize("level", [1, 9])
def test_default_options_write_the_bytes_they_wrote(ctx, level):
    raws = _frame_blobs()
    enc = F.encode_frames(raws, level=level)
    for e, r in zip(enc, raws):
        pieces = [r[at:at + 65536] for at in range(0, len(r), 65536)]
        comp = ctx.lz4_encode_hc_blocks(pieces, level).check().outputs if pieces else []
        blocks = [(False, c) if len(c) < len(p) else (True, p) for p, c in zip(pieces, comp)]
        assert e == R.build(blocks, 4, True, False, R.xxh32(r), len(r))


def test_history_needs_a_level(ctx):
    for kw in (dict(linked=True), dict(dictionary=b"abc"), dict(linked=True, dictionary=b"abc")):
        with pytest.raises(ValueError, match="level from 1 to 12"):
            F.encode_frames([b"hello"], **kw)
        with pytest.raises(ValueError, match="level from 1 to 12"):
            F.Encoder(io.BytesIO(), **kw)
    raw = synth.gen("text", 150000, 9).tobytes()
    w = io.BytesIO()
    enc = F.Encoder(w, level=3, linked=True, dictionary=DICT, dict_id=5)
    enc.write(raw[:1000]); enc.write(raw[1000:])
    enc.finish()
    assert R.decode(w.getvalue(), dictionary=DICT) == raw and R.parse(w.getvalue())[0].dict_id == 5
    assert F.Decoder(io.BytesIO(w.getvalue()), dictionary=DICT).read_to_end() == raw
