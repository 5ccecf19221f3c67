#!/usr/bin/env python3
"""What dictionary training costs (rcx_dict_train_batch).  One JSON line per measurement:

  one_big      ONE 32 KiB dictionary from RECORDS x 2 KiB G-text records (128 MiB), device-resident and from pageable host memory, at
               k = 256 and k = 64 (d = 8, f = 20)
  many_small   JOBS jobs of 1 MiB each (512 records of 2 KiB, a seed per job) in one call, 32 KiB each, k = 256
  reference    tests/dict_train_ref on ONE host thread for the same jobs (--ref: once each, no device needed; of many_small the first
               REF_JOBS jobs, reported per job), the baseline to report against

The method is benchmarks/dict_shared_rate.py's: a time is the host clock around one synchronous call (descriptor copies, staging and the
launch loop included), REPS calls after WARM warm-up calls; min, median and max are reported.  There is no gate on a time.  The device's
bytes are compared with the reference's where --ref has produced them in the same run (--check), or earlier (--save-ref FILE there, --want FILE here).
RECORDS / JOBS / REPS / LEGS in the environment shrink the runs; --out FILE appends the lines to FILE."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rust_compress_amd import synth  # noqa: E402

RECORDS, REC, DICT = int(os.environ.get("RECORDS", "65536")), 2048, 32768
JOBS, JOB_RECORDS = int(os.environ.get("JOBS", "256")), 512
REF_JOBS = int(os.environ.get("REF_JOBS", "4"))
REPS, WARM = int(os.environ.get("REPS", "10")), 2
LEGS = [x for x in os.environ.get("LEGS", "one_big,many_small").split(",") if x]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REF, CHECK = "--ref" in sys.argv, "--check" in sys.argv
# --save-ref FILE: the reference's dictionaries, pickled; --want FILE: the device's are compared with them (the reference needs no device
# and minutes for 128 MiB: it may run elsewhere, earlier)
SAVE = sys.argv[sys.argv.index("--save-ref") + 1] if "--save-ref" in sys.argv else None
WANT = sys.argv[sys.argv.index("--want") + 1] if "--want" in sys.argv else None
saved = {}
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
            "mib_per_s_median": round(nbytes / 2**20 / med * 1e3, 1)}


def one_big():
    return synth.gen_blocks("text", RECORDS, REC, 0x7A11), np.array([RECORDS * REC], np.uint64), np.array([RECORDS], np.uint32), RECORDS


def many_small():
    corp = np.concatenate([synth.gen_blocks("text", JOB_RECORDS, REC, 0x7B00 + j) for j in range(JOBS)])
    return corp, np.full(JOBS, JOB_RECORDS * REC, np.uint64), np.full(JOBS, JOB_RECORDS, np.uint32), JOBS * JOB_RECORDS


def reference(name, corp, in_len, nsamples, k, jobs):
    import dict_train_cases as K
    lib = K.ref_lib()
    lens = np.full(int(nsamples[0]), REC, np.uint64)
    out, rounds, dicts, t = np.zeros(DICT, np.uint8), np.zeros(1, np.uint64), [], []
    for j in range(jobs):
        c = corp[j * int(in_len[0]):(j + 1) * int(in_len[0])]
        t0 = time.perf_counter()
        n = lib.ref_dict_train(p(c), int(in_len[0]), p(lens), int(nsamples[0]), k, 8, 20, p(out), DICT, p(rounds))
        t.append((time.perf_counter() - t0) * 1e3)
        dicts.append(bytes(out[:n]))
    emit({"bench": "reference_one_host_thread", "workload": name, "k": k, "jobs_timed": jobs, "job_bytes": int(in_len[0]),
          "ms_per_job_median": round(sorted(t)[len(t) // 2], 1), "ms_total": round(sum(t), 1), "rounds_last_job": int(rounds[0])})
    saved[(name, k, RECORDS if name == "one_big" else JOBS)] = dicts
    return dicts


def device_leg(name, corp, in_len, nsamples, nrec, k, where, want):
    import torch
    import rust_compress_amd as R
    from rust_compress_amd import _native as N
    global ctx
    if ctx is None:
        ctx = R.Context(0)
    lib = N.lib()
    n = len(in_len)
    in_off = (np.concatenate([[0], np.cumsum(in_len)[:-1]])).astype(np.uint64)
    sample_len = np.full(nrec, REC, np.uint64)
    out_cap, out_off = np.full(n, DICT, np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(DICT)
    out_len, in_used, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    if where == "device":
        d_in, d_out = torch.from_numpy(corp).cuda(), torch.zeros(n * DICT, dtype=torch.uint8, device="cuda")
        b = N.Batch(d_in.data_ptr(), p(in_off), p(in_len), d_out.data_ptr(), p(out_off), p(out_cap), p(out_len), p(in_used), p(status), n, N.MEM_DEVICE)
    else:
        h_out = np.zeros(n * DICT, np.uint8)
        b = N.Batch(p(corp), p(in_off), p(in_len), p(h_out), p(out_off), p(out_cap), p(out_len), p(in_used), p(status), n, N.MEM_HOST)
    ms = []
    for r in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rcx_dict_train_batch(ctx._h, C.byref(b), C.c_void_p(p(nsamples)), C.c_void_p(p(sample_len)), k, 8, 20)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and not status.any(), lib.rcx_last_error(ctx._h)
        if r >= WARM:
            ms.append(dt)
    o = d_out.cpu().numpy() if where == "device" else h_out
    dicts = [bytes(o[int(a):int(a) + int(l)]) for a, l in zip(out_off, out_len)]
    checked = 0
    for j, w in enumerate(want or []):
        assert dicts[j] == w, "job %d differs from the reference" % j
        checked += 1
    emit(dict({"bench": "rcx_dict_train_batch", "workload": name, "memory": where, "k": k, "d": 8, "f": 20, "jobs": n, "corpus_bytes": int(in_len.sum()),
               "dictionary_bytes": DICT, "out_len_min": int(out_len.min()), "jobs_equal_to_reference": checked,
               "scratch_bytes_upper": int(lib.rcx_dict_train_scratch_bytes(n, int(in_len.max()), DICT, k, 20))}, **stats(ms, int(in_len.sum()))))


ctx = None
if __name__ == "__main__":
    head = {"bench": "dict_train_rate", "reps": REPS, "warm": WARM, "reference": REF}
    if not REF or CHECK:
        import torch
        head["device"] = torch.cuda.get_device_name(0)
    emit(head)
    for leg in LEGS:
        corp, in_len, nsamples, nrec = one_big() if leg == "one_big" else many_small()
        for k in ((256, 64) if leg == "one_big" else (256,)):
            want = reference(leg, corp, in_len, nsamples, k, 1 if leg == "one_big" else min(REF_JOBS, JOBS)) if REF else None
            if REF and not CHECK:
                continue
            if WANT and want is None:
                import pickle
                with open(WANT, "rb") as fh:
                    want = pickle.load(fh).get((leg, k, RECORDS if leg == "one_big" else JOBS))
            for where in ("device", "host"):
                device_leg(leg, corp, in_len, nsamples, nrec, k, where, want)
    if SAVE:
        import pickle
        with open(SAVE, "wb") as fh:
            pickle.dump(saved, fh)
    if ctx is not None:
        ctx.close()
