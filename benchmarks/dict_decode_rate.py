#!/usr/bin/env python3
"""What a shared dictionary saves the decoders: RECORDS x 2 KiB G-text records behind ONE 32 KiB G-text dictionary, encoded by the shared
encoders at LZ4 HC level 9 and DEFLATE level 6, then decoded by the history calls on the REPLICATED layout (the dictionary copied in front
of every output slot: rcx_lz4_decode_linked_batch with dict_len, rcx_inflate_hist_batch) against the shared calls on the SHARED layout (the
dictionary once, in the input buffer beside the streams: rcx_lz4_decode_shared_batch, rcx_inflate_shared_batch).  One JSON line per
measurement:

  device   both layouts device-resident (RCX_MEM_DEVICE)
  host     both layouts in pageable host memory (RCX_MEM_HOST): the replicated output buffer crosses PCIe with every copy of the dictionary

The method is benchmarks/dict_shared_rate.py's: a time is the host clock around one synchronous *_batch call (descriptor copies and
launches included); the two calls alternate, REPS calls each after WARM warm-up calls; min, median and max are reported.  Every line
carries the exact footprints: input bytes, output-buffer bytes, and the bytes that cross PCIe each way from host memory (computed from the
layouts by the rules of rcx_api.hip, and checked against each other here).  The two calls' outputs are compared byte for byte.
RECORDS / REPS / FAMILIES / LEGS in the environment shrink the runs; --out FILE appends the lines to FILE."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import rust_compress_amd as R  # noqa: E402
from rust_compress_amd import _native as N, synth  # noqa: E402

RECORDS, REC, DICT = int(os.environ.get("RECORDS", "65536")), 2048, 32768
REPS, WARM = int(os.environ.get("REPS", "10")), 2
FAMILIES = [x for x in os.environ.get("FAMILIES", "lz4,deflate").split(",") if x]
LEGS = [x for x in os.environ.get("LEGS", "device,host").split(",") if x]
LEVEL = {"lz4": 9, "deflate": 6}
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda", 0)
ctx = R.Context(0)
lib = N.lib()
p = lambda a: a.ctypes.data


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def stats(ms, nbytes):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_min": round(ms[0], 3), "ms_median": round(med, 3), "ms_max": round(ms[-1], 3), "reps": len(ms),
            "gib_per_s_median": round(nbytes / 2**30 / med * 1e3, 3)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = fn()
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, lib.rcx_last_error(ctx._h)
    return dt


def alternate(fa, fb):
    for _ in range(WARM):
        once(fa); once(fb)
    ta, tb = [], []
    for _ in range(REPS):                                              # alternating: both see the same machine
        ta.append(once(fa)); tb.append(once(fb))
    return ta, tb


def encode(family, sh):
    """the records behind the dictionary at sh[:DICT], by the shared encoder -> (streams back to back as a uint8 tensor, their lengths)"""
    n = RECORDS
    bound = lib.rcx_lz4_compression_bound if family == "lz4" else lib.rcx_deflate_compression_bound
    cap = (int(bound(REC)) + 15) & ~15
    in_off, in_len = np.arange(n, dtype=np.uint64) * np.uint64(REC) + np.uint64(DICT), np.full(n, REC, np.uint64)
    out_off, out_cap = np.arange(n, dtype=np.uint64) * np.uint64(cap), np.full(n, cap, np.uint64)
    out_len, in_used, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    d_off, d_len = np.zeros(n, np.uint64), np.full(n, DICT, np.uint64)
    d_in, out = sh.to(dev), torch.zeros(n * cap + 64, dtype=torch.uint8, device=dev)
    b = N.Batch(d_in.data_ptr(), p(in_off), p(in_len), out.data_ptr(), p(out_off), p(out_cap), p(out_len), p(in_used), p(status), n, N.MEM_DEVICE)
    f = lib.rcx_lz4_encode_hc_shared_batch if family == "lz4" else lib.rcx_deflate_encode_shared_batch
    assert f(ctx._h, C.byref(b), LEVEL[family], C.c_void_p(p(d_off)), C.c_void_p(p(d_len))) == 0 and not status.any()
    o = out.cpu().numpy()
    lens = out_len.astype(np.int64)
    packed = np.concatenate([o[int(a):int(a) + int(l)] for a, l in zip(out_off, lens)])
    return torch.from_numpy(packed), lens


class Dec:
    """a decode batch: the streams at in_off / in_len of `inb`, the slots every `stride` bytes of `out`, the first at `first`"""

    def __init__(self, family, inb, in_off, in_len, out, stride, first):
        n = RECORDS
        self.family, self.inb, self.out, self.host = family, inb, out, isinstance(inb, np.ndarray)
        self.in_off, self.in_len = in_off.astype(np.uint64), in_len.astype(np.uint64)
        self.out_off = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(first)
        self.out_cap = np.full(n, REC, np.uint64)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        self.flags = np.zeros(n, np.uint32)
        self.b = N.Batch(p(inb) if self.host else inb.data_ptr(), p(self.in_off), p(self.in_len), p(out) if self.host else out.data_ptr(),
                         p(self.out_off), p(self.out_cap), p(self.out_len), p(self.in_used), p(self.status), n, N.MEM_HOST if self.host else N.MEM_DEVICE)
        self.input_bytes = int(inb.size if self.host else inb.numel()) - 64
        self.output_buffer_bytes = int(out.size if self.host else out.numel()) - 64

    def hist(self):
        self.h, self.link = np.full(RECORDS, DICT, np.uint64), np.zeros(RECORDS, np.uint8)
        if self.family == "lz4":
            return lambda: lib.rcx_lz4_decode_linked_batch(ctx._h, C.byref(self.b), C.c_void_p(p(self.link)), C.c_void_p(p(self.h)))
        return lambda: lib.rcx_inflate_hist_batch(ctx._h, C.byref(self.b), C.c_void_p(p(self.flags)), C.c_void_p(p(self.h)))

    def shared(self):
        self.d_off, self.d_len = np.zeros(RECORDS, np.uint64), np.full(RECORDS, DICT, np.uint64)
        if self.family == "lz4":
            return lambda: lib.rcx_lz4_decode_shared_batch(ctx._h, C.byref(self.b), C.c_void_p(p(self.d_off)), C.c_void_p(p(self.d_len)))
        return lambda: lib.rcx_inflate_shared_batch(ctx._h, C.byref(self.b), C.c_void_p(p(self.flags)), C.c_void_p(p(self.d_off)), C.c_void_p(p(self.d_len)))

    def records(self, stride, first):
        assert not self.status.any() and (self.out_len == REC).all(), self.status[:32]
        o = torch.from_numpy(self.out) if self.host else self.out.cpu()
        return o[:RECORDS * stride].view(RECORDS, stride)[:, first:first + REC]


def pcie(family, shared, comp):
    """bytes that cross PCIe each way in one RCX_MEM_HOST call (rcx_api.hip): [in, out]"""
    n = RECORDS
    if shared:                       # the input span (the dictionary and the streams) in; what was produced (the used span) back
        return DICT + comp, n * REC
    if family == "lz4":              # the streams and every replica of the dictionary in; what the chains wrote back
        return comp + n * DICT, n * REC
    span = n * (DICT + REC)          # preload_out: the whole output span in with the streams; the used span (to the last record's end) back
    return comp + span, span


def leg(where, family, packed, lens, dct, recs):
    n = RECORDS
    comp = int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    pad = torch.zeros(64, dtype=torch.uint8)
    in_rep = torch.cat([packed, pad])                                                   # the streams
    in_sh = torch.cat([dct, packed, pad])                                               # the dictionary once, then the streams
    out_rep = torch.cat([torch.cat([dct.expand(n, DICT), torch.zeros(n, REC, dtype=torch.uint8)], 1).contiguous().view(-1), pad])
    out_sh = torch.zeros(n * REC + 64, dtype=torch.uint8)
    if where == "device":
        in_rep, in_sh, out_rep, out_sh = (x.to(dev) for x in (in_rep, in_sh, out_rep, out_sh))
    else:
        in_rep, in_sh, out_rep, out_sh = (x.numpy() for x in (in_rep, in_sh, out_rep, out_sh))
    a = Dec(family, in_rep, off, lens, out_rep, DICT + REC, DICT)
    b = Dec(family, in_sh, off + DICT, lens, out_sh, REC, 0)
    ta, tb = alternate(a.hist(), b.shared())
    ra, rb = a.records(DICT + REC, DICT), b.records(REC, 0)
    assert torch.equal(ra, rb) and torch.equal(rb, recs) and (a.in_used == b.in_used).all() and (a.flags == b.flags).all()
    # the footprints, exactly
    assert a.input_bytes == comp and b.input_bytes == DICT + comp
    assert a.output_buffer_bytes == n * (DICT + REC) and b.output_buffer_bytes == n * REC
    common = {"memory": where, "family": family, "level": LEVEL[family], "records": n, "record_bytes": REC, "dictionary_bytes": DICT,
              "kind": "text", "compressed_bytes": comp}
    for name, e, t, sh in (("replicated_hist_call", a, ta, False), ("shared_call", b, tb, True)):
        pin, pout = pcie(family, sh, comp) if where == "host" else (0, 0)
        emit(dict({"bench": name, "input_bytes": e.input_bytes, "output_buffer_bytes": e.output_buffer_bytes, "pcie_bytes_in": pin,
                   "pcie_bytes_out": pout}, **common, **stats(t, n * REC)))
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    emit(dict({"bench": "shared_vs_replicated", "median_ratio": round(mb / ma, 4), "shared_is_faster": bool(mb < ma)}, **common))
    if where == "host":
        assert sum(pcie(family, True, comp)) < sum(pcie(family, False, comp))
        assert mb < ma, "from host memory the shared call must beat the replicated one (%s: %.3f against %.3f ms)" % (family, mb, ma)


if __name__ == "__main__":
    emit({"bench": "dict_decode_rate", "device": torch.cuda.get_device_name(0), "reps": REPS, "warm": WARM})
    recs = torch.from_numpy(synth.gen_blocks("text", RECORDS, REC, 0x4C5B)).view(RECORDS, REC)
    dct = torch.from_numpy(synth.gen("text", DICT, 99))
    sh = torch.cat([dct, recs.reshape(-1), torch.zeros(64, dtype=torch.uint8)])
    enc = {f: encode(f, sh) for f in FAMILIES}
    for where in LEGS:
        for f in FAMILIES:
            leg(where, f, enc[f][0], enc[f][1], dct, recs)
    ctx.close()
