#!/usr/bin/env python3
"""What history costs and buys the DEFLATE encoder (rcx_deflate_encode_hist_batch) and decoder (rcx_inflate_hist_batch), device-resident
data (RCX_MEM_DEVICE), one JSON line per measurement, at levels 2, 6 and 9 on G-text:

  (a) 4096 x 64 KiB independent blocks: rcx_deflate_encode_level_batch against the new call with hist_len NULL, calls alternating
  (b) the same bytes as chunks linked by 32 KiB (hist_len = 32768 for every block but the first) against the independent blocks:
      time and total size
  (c) 65536 x 2 KiB records, each behind a copy of one 32 KiB dictionary, against the records without one: time and total size --
      the leg that prices rebuilding the dictionary's chains for every record
  (d) the streams of (c) decoded: rcx_inflate_hist_batch behind the dictionary against rcx_inflate_batch on the dictionary-less streams

The method is benchmarks/lz4_hist_rate.py's: a time is the host clock around one synchronous *_batch call (descriptor
copies and launches included); REPS calls after WARM warm-up calls; min, median and max are reported.  (d) compares every decoded
record with the input.  NB / RECORDS / REPS / LEVELS in the environment shrink the runs; --out FILE appends the lines to FILE."""
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

BLOCK, HIST = 65536, 32768
NB = int(os.environ.get("NB", "4096"))
RECORDS, REC, DICT = int(os.environ.get("RECORDS", "65536")), 2048, 32768
REPS, WARM = int(os.environ.get("REPS", "10")), 2
LEVELS = [int(x) for x in os.environ.get("LEVELS", "2,6,9").split(",")]
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


class Enc:
    """a device-memory encode batch: n blocks of `size` bytes every `stride` bytes of d_in, the first at `first`"""

    def __init__(self, d_in, n, size, stride, first=0):
        cap = (int(lib.rcx_deflate_compression_bound(size)) + 15) & ~15
        self.n, self.size = n, size
        self.in_off = (np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(first))
        self.in_len = np.full(n, size, np.uint64)
        self.out_off, self.out_cap = np.arange(n, dtype=np.uint64) * np.uint64(cap), np.full(n, cap, np.uint64)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        self.d_in, self.d_out = d_in, torch.zeros(n * cap + 64, dtype=torch.uint8, device=dev)
        self.b = N.Batch(d_in.data_ptr(), p(self.in_off), p(self.in_len), self.d_out.data_ptr(), p(self.out_off), p(self.out_cap), p(self.out_len),
                         p(self.in_used), p(self.status), n, N.MEM_DEVICE)

    def level(self, level):
        return lambda: lib.rcx_deflate_encode_level_batch(ctx._h, C.byref(self.b), level)

    def hist(self, level, hist_len):
        self.h = np.ascontiguousarray(hist_len, np.uint64) if hist_len is not None else None
        return lambda: lib.rcx_deflate_encode_hist_batch(ctx._h, C.byref(self.b), level, C.c_void_p(p(self.h)) if self.h is not None else None)

    def total(self):
        assert not self.status.any(), self.status[:32]
        return int(self.out_len.sum())


class Dec:
    """the streams of an Enc decoded into an image like its input's (history | slot per block): hist_len None -- rcx_inflate_batch"""

    def __init__(self, enc, hist_len):
        n = enc.n
        self.enc = enc
        self.d_out = enc.d_in.clone()
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        self.flags = np.zeros(n, np.uint32)
        self.in_len = enc.out_len.copy()
        self.h = np.ascontiguousarray(hist_len, np.uint64) if hist_len is not None else None
        self.b = N.Batch(enc.d_out.data_ptr(), p(enc.out_off), p(self.in_len), self.d_out.data_ptr(), p(enc.in_off), p(enc.in_len), p(self.out_len),
                         p(self.in_used), p(self.status), n, N.MEM_DEVICE)

    def wipe(self):
        v = self.d_out[:self.enc.n * (DICT + REC)].view(self.enc.n, DICT + REC)
        v[:, DICT:] = 0

    def fn(self):
        if self.h is None:
            return lambda: lib.rcx_inflate_batch(ctx._h, C.byref(self.b), C.c_void_p(p(self.flags)))
        return lambda: lib.rcx_inflate_hist_batch(ctx._h, C.byref(self.b), C.c_void_p(p(self.flags)), C.c_void_p(p(self.h)))

    def check(self):
        assert not self.status.any(), self.status[:32]
        assert torch.equal(self.d_out, self.enc.d_in)


def alternate(fa, fb):
    for _ in range(WARM):
        once(fa); once(fb)
    ta, tb = [], []
    for _ in range(REPS):                                              # alternating: both see the same machine
        ta.append(once(fa)); tb.append(once(fb))
    return ta, tb


def blocks_and_chunks():
    data = torch.from_numpy(synth.gen_blocks("text", NB, BLOCK, 0x4C5A)).to(dev)
    data = torch.cat([data.view(-1), torch.zeros(64, dtype=torch.uint8, device=dev)])
    linked = np.array([0] + [HIST] * (NB - 1), np.uint64)
    for level in LEVELS:
        a, b, c = Enc(data, NB, BLOCK, BLOCK), Enc(data, NB, BLOCK, BLOCK), Enc(data, NB, BLOCK, BLOCK)
        ta, tb = alternate(a.level(level), b.hist(level, None))
        assert a.total() == b.total() and torch.equal(a.d_out, b.d_out)
        common = {"blocks": NB, "block_bytes": BLOCK, "kind": "text", "level": level}
        emit(dict({"bench": "deflate_encode_level_batch", "compressed_bytes": a.total()}, **common, **stats(ta, NB * BLOCK)))
        emit(dict({"bench": "deflate_encode_hist_batch_null", "compressed_bytes": b.total()}, **common, **stats(tb, NB * BLOCK)))
        f = c.hist(level, linked)
        tc = [once(f) for _ in range(WARM + REPS)][WARM:]
        emit(dict({"bench": "deflate_encode_hist_batch_linked", "history_bytes": HIST, "compressed_bytes": c.total(),
                   "size_vs_independent": round(c.total() / a.total(), 4)}, **common, **stats(tc, NB * BLOCK)))
        del a, b, c


def records():
    recs = torch.from_numpy(synth.gen_blocks("text", RECORDS, REC, 0x4C5B)).to(dev).view(RECORDS, REC)
    dct = torch.from_numpy(synth.gen("text", DICT, 99)).to(dev)
    both = torch.cat([dct.expand(RECORDS, DICT), recs], 1).contiguous().view(-1)          # dictionary | record, RECORDS times
    both = torch.cat([both, torch.zeros(64, dtype=torch.uint8, device=dev)])
    hist = np.full(RECORDS, DICT, np.uint64)
    for level in LEVELS:
        a, b = Enc(both, RECORDS, REC, DICT + REC, DICT), Enc(both, RECORDS, REC, DICT + REC, DICT)
        ta, tb = alternate(a.hist(level, None), b.hist(level, hist))
        common = {"records": RECORDS, "record_bytes": REC, "kind": "text", "level": level}
        emit(dict({"bench": "deflate_encode_hist_batch_records_no_dictionary", "compressed_bytes": a.total()}, **common, **stats(ta, RECORDS * REC)))
        emit(dict({"bench": "deflate_encode_hist_batch_records_dictionary", "dictionary_bytes": DICT, "compressed_bytes": b.total(),
                   "size_vs_no_dictionary": round(b.total() / a.total(), 4)}, **common, **stats(tb, RECORDS * REC)))
        da, db = Dec(a, None), Dec(b, hist)
        da.wipe(); db.wipe()
        ta, tb = alternate(da.fn(), db.fn())
        da.check(); db.check()
        emit(dict({"bench": "inflate_batch_records_no_dictionary", "compressed_bytes": a.total()}, **common, **stats(ta, RECORDS * REC)))
        emit(dict({"bench": "inflate_hist_batch_records_dictionary", "dictionary_bytes": DICT, "compressed_bytes": b.total()}, **common,
                  **stats(tb, RECORDS * REC)))
        del a, b, da, db


if __name__ == "__main__":
    emit({"bench": "deflate_hist_rate", "device": torch.cuda.get_device_name(0), "reps": REPS, "warm": WARM})
    blocks_and_chunks()
    records()
    ctx.close()
