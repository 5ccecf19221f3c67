"""GPU: the batched DEFLATE / zlib / gzip encoder (extension: the reference has no DEFLATE encoder).  Every output is checked by
independent decoders: Python's zlib and gzip, the reference-faithful oracle, and this library's own GPU decoders."""
import ctypes as C
import gzip as pygzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from rust_compress_amd import synth
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 65536
SIZES = [0, 1, 2, 3, 4, 257, 258, 259, 32767, 32768, 32769, 65535, 65536, 65537, SEG - 1, SEG + 1, (1 << 20) + 13]
KINDS = ("text", "words", "dna4", "runs", "rand", "mix")


def _corpus():
    raws = []
    for i, n in enumerate(SIZES):
        raws.append(synth.gen(KINDS[i % len(KINDS)], n, 40 + i).tobytes())
    for i, k in enumerate(KINDS):
        raws.append(synth.gen(k, 100000 + 977 * i, 70 + i).tobytes())
    raws.append(b"\0" * 300000)
    for per in range(1, 16):
        raws.append((bytes(range(7, 7 + per)) * (70000 // per + 1))[:70000 - per])
    return raws


def _bound(n):
    return int(N.lib().rcx_deflate_compression_bound(n))


def _wbits(fmt):
    return {"deflate": -15, "zlib": 15, "gzip": 31}[fmt]


@pytest.fixture(scope="module")
def corpus():
    return _corpus()


@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_round_trip_every_decoder(ctx, oracle, corpus, fmt):
    res = getattr(ctx, fmt + "_encode")(corpus)
    assert not np.asarray(res.status).any()
    assert [int(u) for u in res.in_used] == [len(r) for r in corpus]
    for r, e in zip(corpus, res.outputs):
        assert zlib.decompress(e, _wbits(fmt)) == r
    if fmt == "gzip":
        for r, e in zip(corpus, res.outputs):
            assert pygzip.decompress(e) == r
            assert e[:4] == b"\x1f\x8b\x08\x00" and e[4:8] == b"\0\0\0\0" and e[9] == 0xff
        dec = ctx.gzip_decode(res.outputs, [max(len(r), 1) for r in corpus])
    elif fmt == "zlib":
        for r, e in zip(corpus, res.outputs):
            assert oracle.zlib_decode(e, cap=max(len(r), 1))[0] == r
            assert ((e[0] << 8) | e[1]) % 31 == 0 and e[0] == 0x78
        dec = ctx.zlib_decode(res.outputs, [max(len(r), 1) for r in corpus])
    else:
        for r, e in zip(corpus, res.outputs):
            out, used, flags = oracle.inflate(e, cap=max(len(r), 1))
            assert out == r and used == len(e) and flags == 0
        dec = ctx.inflate(res.outputs, [max(len(r), 1) for r in corpus])
    assert not np.asarray(dec.status).any()
    assert dec.outputs == corpus
    assert not np.asarray(dec.aux).any()                           # no empty block in mid-stream (RCX_W_EMPTY_BLOCK_MIDSTREAM)
    assert [int(u) for u in dec.in_used] == [len(e) for e in res.outputs]


def test_one_64mib_stream(ctx):
    raw = synth.gen_blocks("text", 64, 1 << 20, 3).tobytes()
    res = ctx.gzip_encode([raw])
    assert res.status[0] == 0
    assert zlib.decompress(res.outputs[0], 31) == raw
    dec = ctx.gzip_decode(res.outputs, [len(raw)])
    assert dec.status[0] == 0 and dec.outputs[0] == raw


@pytest.mark.parametrize("kind", ["text", "words", "dna4", "runs", "rand"])
def test_ratio_against_zlib_level_1(ctx, kind):
    raws = [synth.gen(kind, 65536, 1000 + i).tobytes() for i in range(64)]
    ours = ctx.deflate_encode(raws)
    assert not np.asarray(ours.status).any()
    total = sum(len(e) for e in ours.outputs)
    z1 = 0
    for r in raws:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += len(c.compress(r) + c.flush())
    if kind == "rand":
        assert total <= sum(len(r) + len(r) // 1000 + 32 for r in raws)
    else:
        assert total <= z1, (kind, total, z1, total / z1)


def test_matches_reach_across_segments(ctx):
    """A 1 MiB stream of one 20 KiB random chunk repeated: an encoder that isolated its 64 KiB segments would pay for the random
    chunk once per segment (16 x 20 KiB).  (A bar of 24 KiB cannot be met by any DEFLATE encoder: the 20 KiB of random literals plus
    ~4000 matches of at most 258 bytes; zlib -9 makes 28.5 KB of it.)"""
    rep = synth.gen("rand", 20480, 5).tobytes()
    raw = (rep * 52)[:1 << 20]
    res = ctx.deflate_encode([raw])
    assert res.status[0] == 0 and zlib.decompress(res.outputs[0], -15) == raw
    assert len(res.outputs[0]) < 36 * 1024, len(res.outputs[0])


def test_deterministic_across_runs_and_batch_positions(ctx, corpus):
    a = ctx.zlib_encode(corpus).outputs
    b = ctx.zlib_encode(corpus).outputs
    assert a == b
    probe = synth.gen("text", 200000, 77).tobytes()
    alone = ctx.zlib_encode([probe]).outputs[0]
    mixed = [synth.gen(KINDS[i % len(KINDS)], 1000 + 5000 * (i % 7), i).tobytes() for i in range(60)]
    mixed[37] = probe
    assert ctx.zlib_encode(mixed).outputs[37] == alone
    assert ctx.zlib_encode(mixed[30:40]).outputs[7] == alone


def _raw_batch(fn, raws, caps, poison=0xEE, gap=64):
    n = len(raws)
    in_off = np.zeros(n, np.uint64)
    o = 0
    for i, r in enumerate(raws):
        in_off[i] = o
        o += len(r)
    inb = np.frombuffer(b"".join(raws) + b"\0", np.uint8).copy()
    in_len = np.array([len(r) for r in raws], np.uint64)
    out_off = np.zeros(n, np.uint64)
    o = gap
    for i, c in enumerate(caps):
        out_off[i] = o
        o += c + gap
    out = np.full(o, poison, np.uint8)
    out_cap = np.array(caps, np.uint64)
    out_len = np.zeros(n, np.uint64)
    in_used = np.zeros(n, np.uint64)
    st = np.full(n, -1, np.int32)
    p = lambda a: a.ctypes.data
    b = N.Batch(p(inb), p(in_off), p(in_len), p(out), p(out_off), p(out_cap), p(out_len), p(in_used), p(st), n, N.MEM_HOST)
    b._keep = (inb, in_off, in_len, out_cap, in_used)                  # (the struct holds raw pointers: keep the arrays alive)
    return b, out, out_off, out_len, st


@pytest.mark.parametrize("fmt,extra", [("deflate", 0), ("zlib", 6), ("gzip", 18)])
def test_slots_bounds_and_poison(ctx, fmt, extra):
    raws = [b"", b"x", synth.gen("rand", 70000, 1).tobytes(), synth.gen("text", 65536, 2).tobytes(),
            synth.gen("runs", 5000, 3).tobytes(), synth.gen("rand", 65536, 4).tobytes()]
    fn = getattr(N.lib(), "rcx_%s_encode_batch" % fmt)
    # at the bound: never fails; nothing outside a slot or past out_len is touched
    caps = [_bound(len(r)) + extra for r in raws]
    b, out, off, olen, st = _raw_batch(fn, raws, caps)
    assert fn(ctx._h, C.byref(b)) == 0
    assert not st.any()
    good = []
    for i, r in enumerate(raws):
        o, l = int(off[i]), int(olen[i])
        enc = bytes(out[o:o + l])
        assert zlib.decompress(enc, _wbits(fmt)) == r
        good.append(enc)
        assert (out[o + l:o + caps[i] + 64] == 0xEE).all()
    assert (out[:int(off[0])] == 0xEE).all()
    # one byte short for stream 2 and 5: RCX_E_OUTPUT_TOO_SMALL, nothing of them written, the neighbours as before
    caps2 = [len(g) for g in good]
    caps2[2] -= 1
    caps2[5] -= 1
    b, out, off, olen, st = _raw_batch(fn, raws, caps2)
    assert fn(ctx._h, C.byref(b)) == 0
    assert list(st) == [0, 0, N.E_OUTPUT_TOO_SMALL, 0, 0, N.E_OUTPUT_TOO_SMALL]
    for i in range(len(raws)):
        o = int(off[i])
        if st[i]:
            assert int(olen[i]) == 0 and (out[o:o + caps2[i] + 64] == 0xEE).all()
        else:
            assert bytes(out[o:o + int(olen[i])]) == good[i] and (out[o + int(olen[i]):o + caps2[i] + 64] == 0xEE).all()


@pytest.mark.parametrize("codec,name", [(N.DEFLATE_ENCODE, "deflate"), (N.ZLIB_ENCODE, "zlib"), (N.GZIP_ENCODE, "gzip")])
def test_launch_dev_matches_batch_call(ctx, codec, name):
    import torch
    from rust_compress_amd.api import DeviceBatch
    raws = [synth.gen(KINDS[i % len(KINDS)], [0, 17, 65536, 65537, 200000, 3000][i % 6], i).tobytes() for i in range(24)]
    want = getattr(ctx, name + "_encode")(raws).outputs
    dev = torch.device("cuda")
    in_off = np.cumsum([0] + [len(r) for r in raws[:-1]]).astype(np.int64)
    caps = [_bound(len(r)) + 18 for r in raws]
    gap = 64
    out_off = (np.cumsum([0] + caps[:-1]) + gap * np.arange(1, len(raws) + 1)).astype(np.int64)
    inb = torch.tensor(np.frombuffer(b"".join(raws) + b"\0", np.uint8).copy(), device=dev)
    outb = torch.full((sum(caps) + gap * (len(raws) + 1),), 0xEE, dtype=torch.uint8, device=dev)
    T = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev)
    db = DeviceBatch(inb, T(in_off), T([len(r) for r in raws]), outb, T(out_off), T(caps))
    sb = ctx.scratch_bytes(codec, len(raws), max(len(r) for r in raws))
    scratch = torch.full((sb,), 0x5A, dtype=torch.uint8, device=dev)          # (not zero: the encoder must not rely on it)
    ctx.launch_dev(codec, db, scratch)
    torch.cuda.synchronize()
    st = db.status.cpu().numpy()
    ol = db.out_len.cpu().numpy()
    ob = outb.cpu().numpy()
    assert not st.any()
    got = [bytes(ob[int(out_off[i]):int(out_off[i]) + int(ol[i])]) for i in range(len(raws))]
    assert got == want
    # nothing but the streams' own bytes was written: every byte past out_len in a slot and between slots is as it was
    written = np.zeros(ob.size, bool)
    for i in range(len(raws)):
        written[int(out_off[i]):int(out_off[i]) + int(ol[i])] = True
    assert (ob[~written] == 0xEE).all()


def test_stream_of_4gib_minus_1(ctx):
    """The largest stream a block may be (2^32 - 1 bytes), device-resident: the segment kernel's loops and guards run up to the last
    position without wrapping in 32 bits (its last segment is 65535 bytes long), and the stream decodes back."""
    import torch
    from rust_compress_amd.api import DeviceBatch
    dev = torch.device("cuda")
    n = (1 << 32) - 1
    P = 20480
    rep = synth.gen("rand", P, 11)
    inb = torch.tensor(rep, device=dev).repeat(n // P + 1)[:n]
    cap = _bound(n)
    outb = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device=dev)
    T = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev)
    db = DeviceBatch(inb, T([0]), T([n]), outb, T([0]), T([cap]))
    scratch = torch.empty(ctx.scratch_bytes(N.DEFLATE_ENCODE, 1, n), dtype=torch.uint8, device=dev)
    ctx.launch_dev(N.DEFLATE_ENCODE, db, scratch)
    torch.cuda.synchronize()
    assert int(db.status[0]) == 0
    ol = int(db.out_len[0])
    assert 0 < ol < n // 50                                      # (~16.6 M matches of at most 258 bytes: zlib -1 makes ~27 bits of each)
    enc = outb[:ol + 64].cpu().numpy()
    assert (enc[ol:] == 0xEE).all()
    del inb, scratch, outb
    d = zlib.decompressobj(-15)
    tile = np.tile(rep, (64 << 20) // P + 2)
    pos, buf = 0, enc[:ol].tobytes()
    while not d.eof:
        out = d.decompress(buf, 64 << 20)
        buf = d.unconsumed_tail
        k = len(out)
        assert k or d.eof
        assert np.array_equal(np.frombuffer(out, np.uint8), tile[pos % P:pos % P + k])
        pos += k
    assert pos == n and d.unused_data == b""


def test_stream_encoders(ctx):
    import io
    from rust_compress_amd import compress
    compress.set_context(ctx)
    raw = synth.gen("words", 300001, 9).tobytes()
    rng = np.random.default_rng(3)
    e = compress.zlib.Encoder(io.BytesIO())
    p = 0
    while p < len(raw):
        k = int(rng.integers(1, 40000))
        e.write(raw[p:p + k])
        p += k
    z = e.finish().getvalue()
    assert compress.zlib.Decoder(io.BytesIO(z)).read(len(raw) + 10) == raw
    g = compress.gzip.Encoder(io.BytesIO())
    g.write(raw[:1000])
    g.write(raw[1000:])
    assert pygzip.decompress(g.finish().getvalue()) == raw
    f = compress.flate.Encoder(io.BytesIO())
    f.write(raw)
    assert zlib.decompress(f.finish().getvalue(), -15) == raw
    many = [raw[:i * 1000] for i in range(5)]
    assert [zlib.decompress(x, 31) for x in compress.gzip.encode_many(many)] == many
    assert [zlib.decompress(x, 15) for x in compress.zlib.encode_many(many)] == many
    assert [zlib.decompress(x, -15) for x in compress.flate.encode_many(many)] == many


def test_cpp_twin_encoders():
    host = os.path.join(ROOT, "rust_compress_amd", "host")
    exe = os.path.join(host, "test_deflate_encode")
    csrc = os.path.join(ROOT, "rust_compress_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(host, "test_deflate_encode.cpp"), "-L" + csrc, "-lrcx",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CPP_DEFLATE_ENCODE_OK" in p.stdout, p.stdout + p.stderr


def test_gpu_bytes_equal_the_simulator(ctx):
    import sim_deflate_run
    raws = [b"", b"abc", synth.gen("text", 70000, 1).tobytes(), synth.gen("dna4", 65536, 2).tobytes(),
            synth.gen("runs", 30000, 3).tobytes(), synth.gen("rand", 66000, 4).tobytes()]
    for fmt, name in ((0, "deflate"), (1, "zlib"), (2, "gzip")):
        assert sim_deflate_run.encode(raws, fmt)[0] == getattr(ctx, name + "_encode")(raws).outputs
