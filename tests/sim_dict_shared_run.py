"""Builds and drives tests/sim_dict_shared/sim_dict_shared.cpp: the LZ4 HC and DEFLATE encoders behind shared dictionaries, with the
host's rcx_plan_dict, on the wave64 simulator (TEST INFRASTRUCTURE).  One library per family."""
import ctypes as C
import os
import subprocess

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEG = 65536
ALL = 0xFFFFFFFF
SEARCH = 4                              # stop_after: plan, build, links, search (of a raw encode with at least one dictionary)
FAMILIES = ("lz4", "deflate")
_libs = {}


def _out(family):
    return os.path.join(HERE, "sim_dict_shared", "build", "libsim_dict_shared_%s.so" % family)


def build(family):
    return build_sim(_out(family), os.path.join(HERE, "sim_dict_shared", "sim_dict_shared.cpp"),
                     ("k_lz4_hc.hip", "k_lz4_hc_dict.hip", "k_deflate_encode.hip", "k_deflate_hc.hip", "k_deflate_hc_hist.hip", "k_deflate_hc_dict.hip",
                      "k_inflate.hip", "k_crc32.hip", "lz_dict.h", "lz_match.h", "rcx_dev.h", "rcx_plan.h"),
                     ("-DSIM_LZ4" if family == "lz4" else "-DSIM_DEFLATE",))


def lib(family):
    if family not in _libs:
        _libs[family] = C.CDLL(build(family))
    return _libs[family]


def bound(family, n, fmt=0):
    """rcx_lz4_compression_bound(n) / rcx_deflate_compression_bound(n), + 10 for the zlib form with a dictionary"""
    if family == "lz4":
        return n + n // 255 + 20
    return n + 11 * ((n + SEG - 1) // SEG) + 2 + (10 if fmt else 0)


def slots(caps):
    """the output slots, three bytes apart and five from the buffer's start -> (out_off, out_cap, bytes)"""
    out_cap = np.array(list(caps) or [0], np.uint64)
    out_off = (np.concatenate([[0], np.cumsum(out_cap + np.uint64(3))[:-1]]) + 5).astype(np.uint64)
    return out_off, out_cap, int(out_off[-1] + out_cap[-1]) + 16


def run(family, inb, in_off, lens, dict_off, dict_len, level, fmt=0, dict_id=None, caps=None, stop_after=ALL, fill=0xA5, want_cand=False):
    """An encode at `level` of the blocks inb[in_off[i] : in_off[i] + lens[i]] behind the dictionaries inb[dict_off[i] : dict_off[i] +
    dict_len[i]] (as the C ABI takes them), of which the first stop_after launches run.  The output slots lie in a buffer of 0xEE.
    -> dict(rc, outputs, status, out_len, in_used, cand (per block, or None), out, out_off, ndict, scratch, span)"""
    n = len(lens)
    in_len = np.array(list(lens) or [0], np.uint64)
    in_off = np.ascontiguousarray(list(in_off) or [0], np.uint64)
    d_off = np.ascontiguousarray(list(dict_off) or [0], np.uint64)
    d_len = np.ascontiguousarray(list(dict_len) or [0], np.uint64)
    ids = np.zeros(max(n, 1), np.uint32)
    if dict_id is not None:
        ids[:n] = dict_id
    caps = [bound(family, int(l), fmt) for l in lens] if caps is None else caps
    out_off, out_cap, size = slots(caps)
    out = np.full(size, 0xEE, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    cand = np.zeros(int(in_len[:n].sum()) + 1, np.uint32) if want_cand else None
    info = np.zeros(3, np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    rc = lib(family).sim_dict_shared(fmt, level, P(inb), P(in_off), P(in_len), P(d_off), P(d_len), P(ids), P(out), P(out_off), P(out_cap),
                                     P(out_len), P(in_used), P(st), n, C.c_uint32(stop_after), 0xA5 if fill is None else fill, P(cand), P(info))
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    cands = None
    if want_cand:
        ends = np.cumsum(in_len[:n]).astype(np.int64)
        cands = [cand[int(e) - int(l):int(e)].copy() for e, l in zip(ends, in_len[:n])]
    return dict(rc=rc, outputs=outs, status=st[:n].copy(), out_len=out_len[:n].copy(), in_used=in_used[:n].copy(), cand=cands, out=out,
                out_off=out_off[:n], ndict=int(info[0]), scratch=int(info[1]), span=int(info[2]))


def untouched_outside(r):
    """nothing but the bytes the call reports was written"""
    mask = np.ones(r["out"].size, bool)
    for o, l in zip(r["out_off"], r["out_len"]):
        mask[int(o):int(o) + int(l)] = False
    return bool((r["out"][mask] == 0xEE).all())


WORKERS = 8                             # simulator processes at a time: a fixed number, whatever the machine says it has


def _job(args):
    a, kw = args
    return run(*a, **kw)


def run_many(jobs, workers=WORKERS, fresh=False):
    """jobs: (args, kwargs) of run, in at most `workers` forked worker processes -> the results in the jobs' order.  fresh: the workers
    are forked by a new interpreter started for them, not by the caller -- for a caller that holds a GPU, whose forked children would
    hold it too."""
    import pickle
    import sys
    import tempfile
    for f in FAMILIES:
        build(f)
    workers = max(1, min(len(jobs), workers))
    if fresh:
        with tempfile.TemporaryDirectory() as tmp:
            jin, jout = os.path.join(tmp, "jobs.pkl"), os.path.join(tmp, "results.pkl")
            with open(jin, "wb") as fh:
                pickle.dump((jobs, workers), fh)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), jin, jout], cwd=ROOT)
            with open(jout, "rb") as fh:
                return pickle.load(fh)
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("fork")) as ex:
        return list(ex.map(_job, jobs))


if __name__ == "__main__":              # run_many(fresh=True)'s child: jobs file, results file
    import pickle
    import sys
    sys.path.insert(0, ROOT)
    with open(sys.argv[1], "rb") as fh:
        _jobs, _workers = pickle.load(fh)
    _res = run_many(_jobs, _workers)
    with open(sys.argv[2], "wb") as fh:
        pickle.dump(_res, fh)
