"""GPU: compression levels 2..9 of the batched DEFLATE / zlib / gzip encoder (k_deflate_hc.hip on top of k_deflate_encode.hip).  The
device must make the simulator's bytes, every output must decode with this library's decoders and Python's zlib, device-resident
launches take the level from the codec parameter, and the public interfaces take a level."""
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

from rust_compress_amd import synth
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("deflate", "zlib", "gzip")
WBITS = (-15, 15, 31)
CODECS = (N.DEFLATE_ENCODE, N.ZLIB_ENCODE, N.GZIP_ENCODE)


def _corpus():
    raws = [b"", b"a", b"abcd", b"hello hello hello hello", bytes(range(256)) * 3]
    for i, k in enumerate(("text", "words", "dna4", "runs", "rand", "mix")):
        raws.append(synth.gen(k, 65536 + 977 * (i - 2), 30 + i).tobytes())
    raws.append(synth.gen("text", 1 << 20, 37).tobytes())
    raws.append(b"\0" * 300000)
    raws.append((b"abcdefg" * 20000)[:131073])
    return raws


def test_device_equals_simulator(ctx):
    import sim_deflate_hc_run as S
    raws = [b"", b"abc", synth.gen("text", 70000, 1).tobytes(), synth.gen("dna4", 65536, 2).tobytes(),
            synth.gen("runs", 30000, 3).tobytes(), synth.gen("rand", 20000, 4).tobytes()]
    jobs = [(raws, fmt, lv) for lv in (2, 6, 9) for fmt in range(3)]
    for (_, fmt, lv), res in zip(jobs, S.encode_many(jobs)):
        assert res[0] == 0 and not res[2].any()
        assert getattr(ctx, NAMES[fmt] + "_encode")(raws, level=lv).outputs == res[1], (fmt, lv)


@pytest.mark.parametrize("level", range(2, 10))
def test_round_trip(ctx, level):
    raws = _corpus()
    caps = [max(len(r), 1) for r in raws]
    outs = {}
    for fmt, name in enumerate(NAMES):
        res = getattr(ctx, name + "_encode")(raws, level=level)
        assert not res.status.any()
        outs[fmt] = res.outputs
        for r, e in zip(raws, res.outputs):
            assert zlib.decompress(e, WBITS[fmt]) == r
    for fmt, dec in ((0, ctx.inflate), (1, ctx.zlib_decode), (2, ctx.gzip_decode)):
        res = dec(outs[fmt], caps)
        assert not res.status.any() and res.outputs == raws
    lvl1 = ctx.deflate_encode(raws).outputs
    assert sum(map(len, outs[0])) < sum(map(len, lvl1))


def _set_level(ctx, codec, level):
    assert N.lib().rcx_ctx_set_param(ctx._h, codec, level) == 0


@pytest.mark.parametrize("fmt", (0, 2))
def test_full_size_device_resident(ctx, fmt):
    import torch
    from rust_compress_amd.api import DeviceBatch, RcxError
    n, B, level = 4096, 65536, 6
    codec = CODECS[fmt]
    raws = [synth.gen(("text", "words", "runs", "rand")[i % 4], B, i % 64).tobytes() for i in range(n)]
    dev = torch.device("cuda")
    cap = int(N.lib().rcx_deflate_compression_bound(B)) + (0, 6, 18)[fmt]
    T = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev)
    inb = torch.tensor(np.frombuffer(b"".join(raws), np.uint8).copy(), device=dev)
    outb = torch.full((n * cap,), 0xEE, dtype=torch.uint8, device=dev)
    db = DeviceBatch(inb, T(np.arange(n) * B), T([B] * n), outb, T(np.arange(n) * cap), T([cap] * n))
    sb = int(N.lib().rcx_deflate_level_scratch_bytes(n, B))
    assert sb >= ctx.scratch_bytes(codec, n, B)
    scratch = torch.full((sb,), 0x5A, dtype=torch.uint8, device=dev)

    def run(lv, scr):
        outb.fill_(0xEE)
        torch.cuda.synchronize()                                  # (the context launches on a stream of its own)
        _set_level(ctx, codec, lv)
        try:
            ctx.launch_dev(codec, db, scr)
            torch.cuda.synchronize()
        finally:
            _set_level(ctx, codec, 0)
        st, ol, ob = db.status.cpu().numpy(), db.out_len.cpu().numpy(), outb.cpu().numpy()
        return st, ol, ob, [bytes(ob[i * cap:i * cap + int(ol[i])]) for i in range(n)]

    st, ol, ob, got = run(level, scratch)
    assert not st.any()
    for i in range(n):
        assert zlib.decompress(got[i], WBITS[fmt]) == raws[i]
        assert (ob[i * cap + int(ol[i]):(i + 1) * cap] == 0xEE).all()
    assert got[:64] == getattr(ctx, NAMES[fmt] + "_encode")(raws[:64], level=level).outputs
    # too little scratch: the streams it does not cover get RCX_E_MALFORMED, the covered ones are right
    st2, ol2, _, got2 = run(level, scratch[:sb // 2])
    cov = int((st2 == 0).sum())
    assert 0 < cov < n and (st2[:cov] == 0).all() and (st2[cov:] == 3).all() and (ol2[cov:] == 0).all()
    assert got2[:cov] == got[:cov]
    # parameter 0 (and 1): today's encoder
    today = getattr(ctx, NAMES[fmt] + "_encode")(raws).outputs
    for lv in (0, 1):
        st3, _, _, got3 = run(lv, scratch)
        assert not st3.any() and got3 == today
    _set_level(ctx, codec, 10)
    try:
        with pytest.raises(RcxError):
            ctx.launch_dev(codec, db, scratch)
    finally:
        _set_level(ctx, codec, 0)
    torch.cuda.synchronize()


def test_large_stream_level_9(ctx):
    raw = synth.gen("text", 64 << 20, 91).tobytes()
    res = ctx.gzip_encode([raw], level=9)
    assert not res.status.any()
    e = res.outputs[0]
    assert e[8] == 2 and zlib.decompress(e, 31) == raw
    assert len(e) < len(ctx.gzip_encode([raw]).outputs[0])
    dec = ctx.gzip_decode([e], [len(raw)])
    assert not dec.status.any() and dec.outputs[0] == raw


def test_python_interfaces(ctx):
    from rust_compress_amd import compress
    from rust_compress_amd.api import RcxError
    raw = synth.gen("words", 200000, 5).tobytes()
    for mod, wb, hdr in ((compress.flate, -15, None), (compress.zlib, 15, b"\x78\xda"), (compress.gzip, 31, None)):
        e = mod.Encoder(io.BytesIO(), level=9)
        e.write(raw[:70000])
        e.write(raw[70000:])
        z = e.finish().getvalue()
        assert zlib.decompress(z, wb) == raw
        if hdr:
            assert z[:2] == hdr
        d = mod.Encoder(io.BytesIO())
        d.write(raw)
        assert d.finish().getvalue() == mod.encode_many([raw])[0] == mod.encode_many([raw], level=1)[0]
        many = [raw[:i * 1000] for i in range(5)]
        assert [zlib.decompress(x, wb) for x in mod.encode_many(many, level=4)] == many
        for bad in (0, 10, -1):
            with pytest.raises(ValueError):
                mod.Encoder(io.BytesIO(), level=bad)
            with pytest.raises(ValueError):
                mod.encode_many(many, level=bad)
    for name in NAMES:
        for bad in (0, 10):
            with pytest.raises(RcxError):
                getattr(ctx, name + "_encode")([raw], level=bad)


def test_cpp_twin_levels():
    host = os.path.join(ROOT, "rust_compress_amd", "host")
    exe = os.path.join(host, "test_deflate_levels")
    csrc = os.path.join(ROOT, "rust_compress_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(host, "test_deflate_levels.cpp"), "-L" + csrc, "-lrcx",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CPP_DEFLATE_LEVELS_OK" in p.stdout, p.stdout + p.stderr
