#!/usr/bin/env python3
"""What sharing a dictionary saves the encoders: RECORDS x 2 KiB G-text records behind ONE 32 KiB G-text dictionary, through the history
calls on the REPLICATED layout (the dictionary copied in front of every record: rcx_lz4_encode_hc_hist_batch,
rcx_deflate_encode_hist_batch) against the shared calls on the SHARED layout (the dictionary once, then the records:
rcx_lz4_encode_hc_shared_batch, rcx_deflate_encode_shared_batch), at LZ4 levels 1, 9, 12 and DEFLATE levels 2, 6, 9.  One JSON line per
measurement:

  device   both layouts device-resident (RCX_MEM_DEVICE)
  host     both layouts in pageable host memory (RCX_MEM_HOST): the replicated input crosses PCIe with every copy of the dictionary
           (LZ4 level 9 and DEFLATE level 6 only, HOST_LEVELS in the environment)

The method is benchmarks/lz4_hist_rate.py's: a time is the host clock around one synchronous *_batch call (descriptor
copies and launches included); the two calls alternate, REPS calls each after WARM warm-up calls; min, median and max are reported.
Every line carries the exact footprints: input bytes and scratch bytes.  The two calls' outputs are compared byte for byte.
RECORDS / REPS / LZ4_LEVELS / DEFLATE_LEVELS / HOST_LEVELS in the environment shrink the runs; --out FILE appends the lines to FILE."""
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
LEVELS = {"lz4": [int(x) for x in os.environ.get("LZ4_LEVELS", "1,9,12").split(",") if x],
          "deflate": [int(x) for x in os.environ.get("DEFLATE_LEVELS", "2,6,9").split(",") if x]}
HOST_LEVELS = [x for x in os.environ.get("HOST_LEVELS", "lz4:9,deflate:6").split(",") if x]
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
    """an encode batch over `buf` (a device tensor or a numpy array): RECORDS records of REC bytes every `stride` bytes, the first at
    `first`"""

    def __init__(self, family, buf, stride, first):
        n = RECORDS
        bound = lib.rcx_lz4_compression_bound if family == "lz4" else lib.rcx_deflate_compression_bound
        cap = (int(bound(REC)) + 15) & ~15
        self.family, self.buf, self.host = family, buf, isinstance(buf, np.ndarray)
        self.in_off = (np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(first))
        self.in_len = np.full(n, REC, np.uint64)
        self.out_off, self.out_cap = np.arange(n, dtype=np.uint64) * np.uint64(cap), np.full(n, cap, np.uint64)
        self.out_len, self.in_used, self.status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
        self.out = np.zeros(n * cap + 64, np.uint8) if self.host else torch.zeros(n * cap + 64, dtype=torch.uint8, device=dev)
        self.b = N.Batch(p(buf) if self.host else buf.data_ptr(), p(self.in_off), p(self.in_len), p(self.out) if self.host else self.out.data_ptr(),
                         p(self.out_off), p(self.out_cap), p(self.out_len), p(self.in_used), p(self.status), n, N.MEM_HOST if self.host else N.MEM_DEVICE)
        self.input_bytes = int(buf.size if self.host else buf.numel()) - 64

    def hist(self, level):
        self.h = np.full(RECORDS, DICT, np.uint64)
        f = lib.rcx_lz4_encode_hc_hist_batch if self.family == "lz4" else lib.rcx_deflate_encode_hist_batch
        return lambda: f(ctx._h, C.byref(self.b), level, C.c_void_p(p(self.h)))

    def shared(self, level):
        self.d_off, self.d_len = np.zeros(RECORDS, np.uint64), np.full(RECORDS, DICT, np.uint64)
        f = lib.rcx_lz4_encode_hc_shared_batch if self.family == "lz4" else lib.rcx_deflate_encode_shared_batch
        return lambda: f(ctx._h, C.byref(self.b), level, C.c_void_p(p(self.d_off)), C.c_void_p(p(self.d_len)))

    def total(self):
        assert not self.status.any(), self.status[:32]
        return int(self.out_len.sum())

    def same_bytes(self, other):
        a, b = (torch.from_numpy(x.out) if x.host else x.out.cpu() for x in (self, other))
        return bool((self.out_len == other.out_len).all()) and torch.equal(a, b)


def alternate(fa, fb):
    for _ in range(WARM):
        once(fa); once(fb)
    ta, tb = [], []
    for _ in range(REPS):                                              # alternating: both see the same machine
        ta.append(once(fa)); tb.append(once(fb))
    return ta, tb


def scratch(family, shared):
    """what the batch path allocates: every record one segment; the history calls one more segment of links per record"""
    if family == "lz4":
        plain = int(lib.rcx_lz4_hc_scratch_bytes(RECORDS, REC))
        return int(lib.rcx_lz4_hc_shared_scratch_bytes(RECORDS, REC, 1)) if shared else int(lib.rcx_lz4_hc_hist_scratch_bytes(RECORDS, REC)), plain
    plain = int(lib.rcx_deflate_level_scratch_bytes(RECORDS, REC))
    return int(lib.rcx_deflate_shared_scratch_bytes(RECORDS, REC, 1)) if shared else int(lib.rcx_deflate_hist_scratch_bytes(RECORDS, REC)), plain


def leg(where, rep_buf, sh_buf, which):
    for family, level in which:
        a, b = Enc(family, rep_buf, DICT + REC, DICT), Enc(family, sh_buf, REC, DICT)
        ta, tb = alternate(a.hist(level), b.shared(level))
        assert a.total() == b.total() and a.same_bytes(b)
        common = {"memory": where, "family": family, "level": level, "records": RECORDS, "record_bytes": REC, "dictionary_bytes": DICT,
                  "kind": "text", "compressed_bytes": a.total()}
        for name, e, t, sh in (("replicated_hist_call", a, ta, False), ("shared_call", b, tb, True)):
            sb, plain = scratch(family, sh)
            emit(dict({"bench": name, "input_bytes": e.input_bytes, "scratch_bytes": sb, "scratch_bytes_beyond_no_history": sb - plain},
                      **common, **stats(t, RECORDS * REC)))
        ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        emit(dict({"bench": "shared_vs_replicated", "median_ratio": round(mb / ma, 4), "shared_is_faster": bool(mb < ma)}, **common))
        del a, b


if __name__ == "__main__":
    emit({"bench": "dict_shared_rate", "device": torch.cuda.get_device_name(0), "reps": REPS, "warm": WARM})
    recs = torch.from_numpy(synth.gen_blocks("text", RECORDS, REC, 0x4C5B)).view(RECORDS, REC)
    dct = torch.from_numpy(synth.gen("text", DICT, 99))
    pad = torch.zeros(64, dtype=torch.uint8)
    rep = torch.cat([torch.cat([dct.expand(RECORDS, DICT), recs], 1).contiguous().view(-1), pad])      # dictionary | record, RECORDS times
    sh = torch.cat([dct, recs.reshape(-1), pad])                                                        # the dictionary once, then the records
    d_rep, d_sh = rep.to(dev), sh.to(dev)
    leg("device", d_rep, d_sh, [(f, lv) for f in ("lz4", "deflate") for lv in LEVELS[f]])
    del d_rep, d_sh
    leg("host", rep.numpy(), sh.numpy(), [(x.split(":")[0], int(x.split(":")[1])) for x in HOST_LEVELS])
    ctx.close()
