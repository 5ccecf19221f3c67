"""GPU suite of the bzip2 encoder (rcx_bzip2_encode_batch; k_bzip2_enc.hip): about 40 files in one call at levels 1, 5 and 9, from host and
from device memory, read back by libbz2 (strictly) and by rcx_bzip2_decode_batch, within the size cap of the specification; the small
cases byte for byte the wave simulator's; the size query and the exact retry with guard bytes; the Python layer; the round knob."""
import bz2
import ctypes as C
import io

import numpy as np
import pytest

import bz2_cases as BC
import bz2_enc_cases as EC
import sim_bzip2_enc_run as S
from rust_compress_amd import _native as N
from rust_compress_amd import bzip2
from rust_compress_amd import synth

pytestmark = pytest.mark.gpu
BZIP2_ENCODE = 47


def _p(a):
    return a.ctypes.data


def call(ctx, datas, caps, level, device=False):
    """one rcx_bzip2_encode_batch over the layout of sim_bzip2_run.layout -> results in the form of sim_bzip2_enc_run.run's"""
    n = len(datas)
    inb, in_off, in_len, out, out_off, out_cap = S.layout(datas, caps)
    out_len, in_used, status = np.full(n, 0x7777, np.uint64), np.full(n, 0x7777, np.uint64), np.full(n, -99, np.int32)
    if device:
        import torch
        d_in, d_out = torch.from_numpy(inb).cuda(), torch.from_numpy(out).cuda()
        b = N.Batch(d_in.data_ptr(), _p(in_off), _p(in_len), d_out.data_ptr(), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_DEVICE)
    else:
        b = N.Batch(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_HOST)
    rc = N.lib().rcx_bzip2_encode_batch(ctx._h, C.byref(b), level)
    if device:
        out = d_out.cpu().numpy()
    data = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) if status[i] == 0 else None for i in range(n)]
    return dict(rc=rc, err=N.lib().rcx_last_error(ctx._h).decode(), status=status, out_len=out_len, in_used=in_used, out=out, out_off=out_off,
                out_cap=out_cap, data=data)


def first_cap(d):
    return len(d) + len(d) // 64 + 1024


@pytest.fixture(scope="module")
def files():
    """level -> (names, datas): the cases at the real chunk size, spread over the levels, and the three large files"""
    small = [(name, data) for name, data, _, _ in EC.real_c()]
    assert len(small) >= 36
    by = {1: small[0::3], 5: small[1::3], 9: small[2::3]}
    by[1] = by[1] + [("text250000", synth.gen("text", 250000, 21).tobytes()), ("aaaab120000", b"aaaab" * 24000)]
    by[9] = by[9] + [("text950000", synth.gen("text", 950000, 22).tobytes())]
    return {lv: tuple(zip(*v)) for lv, v in by.items()}


@pytest.fixture(scope="module")
def host_runs(ctx, files):
    return {lv: call(ctx, datas, [first_cap(d) for d in datas], lv) for lv, (names, datas) in files.items()}


def check(names, datas, level, r):
    assert r["rc"] == N.RC_OK, r["err"]
    for i, (name, d) in enumerate(zip(names, datas)):
        assert int(r["status"][i]) == BC.OK, (name, int(r["status"][i]))
        s = r["data"][i]
        assert int(r["in_used"][i]) == len(d), name
        assert s[:4] == b"BZh" + bytes([0x30 + level]), name
        assert BC.strict(s) == (d, len(s)), name
        theirs = len(bz2.compress(d, level))
        print("level %d %s: %d bytes, libbz2 %d" % (level, name, len(s), theirs))
        assert len(s) <= theirs * 1.01 + 8, (name, len(s), theirs)
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])


@pytest.mark.parametrize("level", [1, 5, 9])
def test_libbz2_reads_every_file_from_host_memory(files, host_runs, level):
    check(files[level][0], files[level][1], level, host_runs[level])


@pytest.mark.parametrize("level", [1, 5, 9])
def test_from_device_memory_the_same_bytes(ctx, files, host_runs, level):
    names, datas = files[level]
    r = call(ctx, datas, [first_cap(d) for d in datas], level, device=True)
    check(names, datas, level, r)
    assert r["data"] == host_runs[level]["data"] and (r["out"] == host_runs[level]["out"]).all()


def test_block_structure_of_the_large_files(host_runs, files):
    """three blocks at level 1 (bit-unaligned joins), two at level 9, and the run-length step's expansion at the real block size: 120 000
    bytes of aaaab have a form of 144 000 bytes, so a chunk is 82 016 input bytes and the file two blocks, as libbz2 writes two"""
    def nblocks(s):
        v, mark = int.from_bytes(s, "big"), (0x314159265359).to_bytes(6, "big")
        return sum((v << k).to_bytes(len(s) + 1, "big").count(mark) for k in range(8))
    names1, names9 = files[1][0], files[9][0]
    assert nblocks(host_runs[1]["data"][names1.index("text250000")]) == 3
    assert nblocks(host_runs[1]["data"][names1.index("aaaab120000")]) == 2
    assert nblocks(host_runs[9]["data"][names9.index("text950000")]) == 2


def test_our_decoder_reads_them(ctx, files, host_runs):
    for level in (1, 5, 9):
        names, datas = files[level]
        got = bzip2.decode_many(host_runs[level]["data"], ctx=ctx)
        assert got == list(datas), level


def test_bytes_equal_the_wave_simulators(ctx, files, host_runs):
    """the cases below 4 KiB, the same layout both ways"""
    total = 0
    for level in (1, 5, 9):
        names, datas = files[level]
        keep = [i for i, d in enumerate(datas) if len(d) < 4096]
        total += len(keep)
        sub = [datas[i] for i in keep]
        caps = [first_cap(d) for d in sub]
        sim = S.run(sub, caps, level, stages=False)
        dev = call(ctx, sub, caps, level)
        assert sim["rc"] == 0 and dev["rc"] == 0
        assert sim["data"] == dev["data"] and (sim["out"] == dev["out"]).all()
        assert list(sim["out_len"]) == list(dev["out_len"]) and list(sim["status"]) == list(dev["status"])
        assert [host_runs[level]["data"][i] for i in keep] == dev["data"]
    assert total >= 24


def test_size_query_then_exact_retry_and_the_call_twice(ctx, files, host_runs):
    names, datas = files[5]
    want = host_runs[5]["data"]
    q = call(ctx, datas, [0] * len(datas), 5)
    assert q["rc"] == 0 and (q["out"] == 0xEE).all()
    assert all(int(s) == BC.E_TOO_SMALL for s in q["status"])
    assert [int(x) for x in q["out_len"]] == [len(w) for w in want] and not any(int(x) for x in q["in_used"])
    sizes = [int(x) for x in q["out_len"]]
    exact = call(ctx, datas, sizes, 5, device=True)
    assert exact["data"] == want and S.untouched_outside(exact["out"], exact["out_off"], exact["out_cap"])
    short = call(ctx, datas, [s - 1 for s in sizes], 5)
    assert all(int(s) == BC.E_TOO_SMALL for s in short["status"]) and [int(x) for x in short["out_len"]] == sizes
    assert (short["out"] == 0xEE).all()
    # a file that fits beside files that do not; the same call twice
    mixed = [s if i % 2 else s - 1 for i, s in enumerate(sizes)]
    a, b = call(ctx, datas, mixed, 5), call(ctx, datas, mixed, 5)
    assert [int(s) for s in a["status"]] == [BC.OK if i % 2 else BC.E_TOO_SMALL for i in range(len(datas))]
    assert a["data"] == b["data"] and (a["out"] == b["out"]).all()
    assert all(a["data"][i] == want[i] for i in range(1, len(datas), 2))
    assert S.untouched_outside(a["out"], a["out_off"], a["out_cap"])


def test_refusals(ctx):
    for level in (0, 10):
        r = call(ctx, [b"abc"], [100], level)
        assert r["rc"] == N.RC_BAD_ARG and "level" in r["err"] and (r["out"] == 0xEE).all()


def test_rounds_of_64_give_the_same_bytes(ctx, files, host_runs):
    names, datas = files[1]
    assert N.lib().rcx_ctx_set_param(ctx._h, BZIP2_ENCODE, 64) == N.RC_OK
    try:
        many = [d[:3000] for d in datas] * 6                                # more blocks than a round of 64
        few = call(ctx, many, [first_cap(d) for d in many], 1)
    finally:
        assert N.lib().rcx_ctx_set_param(ctx._h, BZIP2_ENCODE, 0) == N.RC_OK
    default = call(ctx, many, [first_cap(d) for d in many], 1)
    assert few["rc"] == 0 and default["rc"] == 0 and sum(1 for d in many if d) > 64
    assert few["data"] == default["data"] and (few["out"] == default["out"]).all()
    assert all(BC.strict(s)[0] == d for s, d in zip(few["data"][:20], many[:20]))
    assert N.lib().rcx_ctx_set_param(ctx._h, BZIP2_ENCODE, 5000) == N.RC_OK
    try:
        r = call(ctx, [b"abc"], [100], 1)
        assert r["rc"] == N.RC_BAD_ARG and "round" in r["err"]
    finally:
        assert N.lib().rcx_ctx_set_param(ctx._h, BZIP2_ENCODE, 0) == N.RC_OK


def test_python_layer(ctx, files):
    from rust_compress_amd import compress
    compress.set_context(ctx)
    names, datas = files[9]
    out = bzip2.encode_many(datas[:8], level=9, ctx=ctx)
    assert all(BC.strict(s) == (d, len(s)) for s, d in zip(out, datas[:8]))
    assert bzip2.encode_many([], ctx=ctx) == []
    rnd = np.random.default_rng(3).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    s = bzip2.encode_many([rnd, b"", b"x"], level=2, ctx=ctx)
    assert [BC.strict(x)[0] for x in s] == [rnd, b"", b"x"] and len(s[1]) == 14
    with pytest.raises(ValueError):
        bzip2.encode_many([b"x"], level=0, ctx=ctx)
    w = bzip2.Encoder(io.BytesIO(), level=3)
    text = datas[names.index("text12000")] if "text12000" in names else synth.gen("text", 12000, 1).tobytes()
    assert w.write(text[:5000]) == 5000 and w.write(text[5000:]) == len(text) - 5000
    w.flush()
    blob = w.finish().getvalue()
    assert blob[:4] == b"BZh3" and bz2.decompress(blob) == text
    d = bzip2.Decoder(io.BytesIO(blob + b"tail"))
    assert d.read_to_end() == text and d.finish().read(-1) == b"tail"
