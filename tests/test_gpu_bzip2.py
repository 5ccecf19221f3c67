"""GPU suite of the bzip2 decoder (rcx_bzip2_decode_batch; k_bzip2.hip): about 64 mixed files in one call against libbz2 read strictly, from
host and from device memory; the size query and the exact retry with guard bytes; failing files between good ones, twice; the Python
layer; the device's results against the wave simulator's on the same inputs; the 200 single-bit flips."""
import ctypes as C
import io

import numpy as np
import pytest

import bz2_cases as BC
import sim_bzip2_run as S
from rust_compress_amd import _native as N
from rust_compress_amd import bzip2

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data


def call(ctx, blobs, caps, device=False):
    """one rcx_bzip2_decode_batch over the layout of sim_bzip2_run.layout -> results in the form of sim_bzip2_run.run's"""
    n = len(blobs)
    inb, in_off, in_len, out, out_off, out_cap = S.layout(blobs, caps)
    out_len, in_used, status = np.full(n, 0x7777, np.uint64), np.full(n, 0x7777, np.uint64), np.full(n, -99, np.int32)
    if device:
        import torch
        d_in, d_out = torch.from_numpy(inb).cuda(), torch.from_numpy(out).cuda()
        b = N.Batch(d_in.data_ptr(), _p(in_off), _p(in_len), d_out.data_ptr(), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_DEVICE)
    else:
        b = N.Batch(_p(inb), _p(in_off), _p(in_len), _p(out), _p(out_off), _p(out_cap), _p(out_len), _p(in_used), _p(status), n, N.MEM_HOST)
    rc = N.lib().rcx_bzip2_decode_batch(ctx._h, C.byref(b))
    assert rc == N.RC_OK, (rc, N.lib().rcx_last_error(ctx._h).decode())
    if device:
        out = d_out.cpu().numpy()
    data = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) if status[i] == 0 else None for i in range(n)]
    return dict(status=status, out_len=out_len, in_used=in_used, out=out, out_off=out_off, out_cap=out_cap, data=data)


def check_against_oracle(names, blobs, r):
    for i, (name, blob) in enumerate(zip(names, blobs)):
        want = BC.expected(blob)
        st = int(r["status"][i])
        if want is None:
            assert st not in (BC.OK, BC.E_TOO_SMALL), (name, st)
            assert int(r["out_len"][i]) == 0 and int(r["in_used"][i]) == 0, name
        else:
            assert st == BC.OK, (name, st)
            assert int(r["out_len"][i]) == len(want[0]) and int(r["in_used"][i]) == want[1], name
            assert r["data"][i] == want[0], name
    assert S.untouched_outside(r["out"], r["out_off"], r["out_cap"])


def same(a, b):
    return (list(a["status"]) == list(b["status"]) and list(a["out_len"]) == list(b["out_len"]) and list(a["in_used"]) == list(b["in_used"])
            and a["data"] == b["data"])


@pytest.fixture(scope="module")
def mixed():
    names, blobs = zip(*BC.mixed64())
    assert 56 <= len(names) <= 72
    return names, blobs, [len(e[0]) if e else 64 for e in map(BC.expected, blobs)]


@pytest.fixture(scope="module")
def host_run(ctx, mixed):
    return call(ctx, mixed[1], mixed[2])


def test_parity_with_libbz2_from_host_memory(mixed, host_run):
    """failing files sit between good ones; slots of exactly the decoded size; guard bytes around every slot intact"""
    check_against_oracle(mixed[0], mixed[1], host_run)


def test_parity_with_libbz2_from_device_memory(ctx, mixed, host_run):
    r = call(ctx, mixed[1], mixed[2], device=True)
    check_against_oracle(mixed[0], mixed[1], r)
    assert same(r, host_run)


def test_the_same_call_twice(ctx, mixed, host_run):
    r = call(ctx, mixed[1], mixed[2])
    assert same(r, host_run) and (r["out"] == host_run["out"]).all()


def test_results_equal_the_wave_simulators(ctx, mixed):
    """the files of the mixed call below 4 KiB (the simulator takes a second per 100 000-byte block), the same layout both ways"""
    keep = [i for i, b in enumerate(mixed[1]) if len(b) < 4096]
    assert len(keep) >= 40
    blobs, caps = [mixed[1][i] for i in keep], [mixed[2][i] for i in keep]
    sim = S.run(blobs, caps)
    dev = call(ctx, blobs, caps)
    assert sim["rc"] == 0 and same(sim, dev) and (sim["out"] == dev["out"]).all()


def test_size_query_then_exact_retry(ctx, mixed, host_run):
    names, blobs, caps = mixed
    q = call(ctx, blobs, [0] * len(blobs))
    assert (q["out"] == 0xEE).all()
    for i, blob in enumerate(blobs):
        want = BC.expected(blob)
        if want is None:
            assert int(q["status"][i]) == int(host_run["status"][i]) and int(q["out_len"][i]) == 0, names[i]
        elif len(want[0]) == 0:
            assert int(q["status"][i]) == BC.OK
        else:
            assert int(q["status"][i]) == BC.E_TOO_SMALL and int(q["out_len"][i]) == len(want[0]), names[i]
    sizes = [int(x) for x in q["out_len"]]
    check_against_oracle(names, blobs, call(ctx, blobs, sizes))
    short = call(ctx, blobs, [max(s - 1, 0) for s in sizes], device=True)
    assert all(int(short["status"][i]) == BC.E_TOO_SMALL and int(short["out_len"][i]) == s for i, s in enumerate(sizes) if s)
    assert S.untouched_outside(short["out"], short["out_off"], short["out_cap"])


def test_statuses(ctx):
    blobs = [BC.short_cycle()[0], BC.randomised(), dict(BC.named())["bad_magic"], dict(BC.named())["stream_then_header"], dict(BC.named())["bad_block_crc"],
             dict(BC.named())["bad_stream_crc"], dict(BC.named())["too_few_selectors"]]
    r = call(ctx, blobs, [200] * len(blobs))
    assert list(r["status"]) == [BC.E_BLOCK_CRC, BC.E_RANDOMISED, BC.E_MAGIC, BC.E_EOF, BC.E_BLOCK_CRC, BC.E_STREAM_CRC, BC.E_DATA]
    assert N.lib().rcx_status_string(BC.E_MAGIC) == b"not a bzip2 file" and N.lib().rcx_status_string(BC.E_RANDOMISED).startswith(b"randomised")


def test_single_bit_flips(ctx):
    """200 seeded flips of the two-block file in one call: status nonzero exactly where the strict oracle raises, bytes equal elsewhere"""
    fl = BC.flips()
    names, blobs = ["flip%d" % b for b, _ in fl], [b for _, b in fl]
    assert len(blobs) == 200
    r = call(ctx, blobs, [len(e[0]) + 3 if e else 64 for e in map(BC.expected, blobs)], device=True)
    check_against_oracle(names, blobs, r)


def test_the_largest_inputs(ctx):
    """three blocks at level 1 and one block of 250 000 bytes at level 9 (left out of the mixed call)"""
    names = ("text250000_l1", "text250000_l9")
    blobs = [dict(BC.named())[k] for k in names]
    check_against_oracle(names, blobs, call(ctx, blobs, [250000, 250000]))


def test_python_layer(ctx, mixed):
    names, blobs, caps = mixed
    res = bzip2.decode_many(blobs, ctx=ctx, return_exceptions=True)
    kinds = {BC.E_EOF: bzip2.TruncatedError, BC.E_MAGIC: bzip2.MagicError, BC.E_DATA: bzip2.DataError, BC.E_BLOCK_CRC: bzip2.BlockChecksumError,
             BC.E_STREAM_CRC: bzip2.StreamChecksumError}
    for name, blob, got in zip(names, blobs, res):
        want = BC.expected(blob)
        if want is None:
            assert isinstance(got, bzip2.Bzip2Error) and type(got) is kinds[got.status], (name, got)
        else:
            assert got == want[0], name
    with pytest.raises(bzip2.FilesFailed):
        bzip2.decode_many(blobs[:12] + (dict(BC.named())["bad_magic"],), ctx=ctx)
    assert bzip2.decode_many([], ctx=ctx) == []
    from rust_compress_amd import compress
    compress.set_context(ctx)
    good = dict(BC.named())
    d = bzip2.Decoder(io.BytesIO(good["stream_xyz"]))
    want = BC.strict(good["stream_xyz"])[0]
    assert d.read(10) == want[:10] and d.read_to_end() == want[10:] and d.eof()
    assert d.finish().read(-1) == b"xyz"
    assert bzip2.Decoder(io.BytesIO(good["three_streams"])).read_to_end() == BC.strict(good["three_streams"])[0]
    with pytest.raises(bzip2.RandomisedError):
        bzip2.Decoder(io.BytesIO(BC.randomised())).read(1)
    with pytest.raises(bzip2.TruncatedError):
        bzip2.Decoder(io.BytesIO(good["trunc40"])).read_to_end()
