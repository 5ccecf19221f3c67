"""Builds and drives tests/sim_dict_decode/sim_dict_decode.cpp: the LZ4 and DEFLATE / zlib decoders behind shared dictionaries, with the
host's rcx_plan_dict, on the wave64 simulator (TEST INFRASTRUCTURE)."""
import ctypes as C
import os
import subprocess

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "sim_dict_decode", "build", "libsim_dict_decode.so")
FAMILY = {"lz4": 0, "deflate": 1, "zlib": 2}
SENTINEL = 0x5A
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_dict_decode", "sim_dict_decode.cpp"),
                     ("k_inflate2.hip", "k_inflate_dict.hip", "k_lz4_dict.hip", "rcx_dev.h", "rcx_plan.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.sim_guarded.restype = C.c_void_p
        _lib.sim_guarded.argtypes = [C.c_uint64, C.c_int]
    return _lib


def guarded(data, front):
    """a copy of `data` (uint8 array) between two pages that cannot be touched: front -- it begins at a page's first byte, else it ends
    at a page's last"""
    n = max(int(data.size), 1)
    p = lib().sim_guarded(n, 1 if front else 0)
    assert p
    a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,))
    a[:data.size] = data
    return a[:data.size] if data.size else a[:0]


def run(family, inb, in_off, in_len, dict_off, dict_len, out_off, out_cap, out_size, dict_id=None):
    """One decode of the streams inb[in_off[i] : in_off[i] + in_len[i]] behind the dictionaries inb[dict_off[i] : dict_off[i] +
    dict_len[i]] (as the C ABI takes them) into the slots out_off / out_cap of an output buffer of out_size sentinels.  The input
    buffer ends at an untouchable page (a load beyond its last byte ends the process) and the output buffer begins at one.
    -> dict(rc, err, status, out_len, in_used, flags, out, outputs, ndict, span)"""
    n = len(in_len)
    u64 = lambda v: np.ascontiguousarray(list(v) or [0], np.uint64)
    in_off, in_len, d_off, d_len, out_off, out_cap = u64(in_off), u64(in_len), u64(dict_off), u64(dict_len), u64(out_off), u64(out_cap)
    ids = np.zeros(max(n, 1), np.uint32)
    if dict_id is not None:
        ids[:n] = dict_id
    gin = guarded(np.ascontiguousarray(inb, np.uint8), False)
    out = guarded(np.full(out_size, SENTINEL, np.uint8), True)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -99, np.int32)
    flags = np.zeros(max(n, 1), np.uint32)
    info = np.zeros(2, np.uint64)
    err = C.create_string_buffer(512)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_dict_decode(FAMILY[family], P(gin) if gin.size else None, P(in_off), P(in_len), P(d_off), P(d_len), P(ids), P(out), P(out_off),
                               P(out_cap), P(out_len), P(in_used), P(st), P(flags), n, P(info), err, 512)
    out = out.copy()
    outs = [bytes(out[int(o):int(o) + int(l)]) for o, l in zip(out_off[:n], out_len[:n])]
    return dict(rc=rc, err=err.value.decode(), status=st[:n].copy(), out_len=out_len[:n].copy(), in_used=in_used[:n].copy(),
                flags=flags[:n].copy(), out=out, outputs=outs, ndict=int(info[0]), span=int(info[1]))


def only_slots_changed(out, out_off, out_cap):
    """nothing outside [out_off[i], out_off[i] + out_cap[i]) was written"""
    mask = np.ones(out.size, bool)
    for o, c in zip(out_off, out_cap):
        mask[int(o):int(o) + int(c)] = False
    return bool((out[mask] == SENTINEL).all())


WORKERS = 8                             # simulator processes at a time: a fixed number, whatever the machine says it has


def _job(args):
    fn, a, kw = args
    if fn == "run":
        return run(*a, **kw)
    import importlib
    mod, name = fn.rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)(*a, **kw)


def run_many(jobs, workers=WORKERS, fresh=False):
    """jobs: (function, args, kwargs) -- "run", or "module.function" of the tests directory (the history kernels' runners) -- in at most
    `workers` forked worker processes -> the results in the jobs' order.  fresh: the workers are forked by a new interpreter started
    for them, not by the caller -- for a caller that holds a GPU, whose forked children would hold it too."""
    import pickle
    import sys
    import tempfile
    build()
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
    sys.path.insert(0, HERE)
    with open(sys.argv[1], "rb") as fh:
        _jobs, _workers = pickle.load(fh)
    _res = run_many(_jobs, _workers)
    with open(sys.argv[2], "wb") as fh:
        pickle.dump(_res, fh)
