"""Builds and drives tests/sim_dict_train/sim_dict_train.cpp: the dictionary trainer's kernels and launch loop with the host's
rcx_plan_train on the wave64 simulator (TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_dict_train", "build", "libsim_dict_train.so")
RC_BAD_ARG = -1
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_dict_train", "sim_dict_train.cpp"), ("k_dict_train.hip", "rcx_dev.h", "rcx_plan.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def run(jobs, k=256, d=8, f=20, fill=0xA5, lens_override=None):
    """One call over jobs = [(samples, C)], samples a list of bytes.  The corpora lie three bytes apart in the input buffer and the
    slots three bytes apart in a buffer of 0xEE.  lens_override: {job: sample lengths} handed to the call in place of the real ones.
    -> dict(rc, err, dicts, out_len, in_used, status, rounds, out, out_off, out_cap, scratch, launches, bound)"""
    n = len(jobs)
    corp = [b"".join(s) for s, _ in jobs]
    in_len = np.array([len(c) for c in corp] or [0], np.uint64)
    in_off = (np.concatenate([[0], np.cumsum(in_len + np.uint64(3))[:-1]]) + 1).astype(np.uint64)
    inb = np.full(int(in_off[-1] + in_len[-1]) + 16, 0x5A, np.uint8)
    for o, c in zip(in_off, corp):
        inb[int(o):int(o) + len(c)] = np.frombuffer(c, np.uint8)
    lens = [[len(x) for x in s] for s, _ in jobs]
    for j, l in (lens_override or {}).items():
        lens[j] = list(l)
    nsamples = np.array([len(l) for l in lens] or [0], np.uint32)
    sample_len = np.array([x for l in lens for x in l] or [0], np.uint64)
    out_cap = np.array([c for _, c in jobs] or [0], np.uint64)
    out_off = (np.concatenate([[0], np.cumsum(out_cap + np.uint64(3))[:-1]]) + 5).astype(np.uint64)
    out = np.full(int(out_off[-1] + out_cap[-1]) + 16, 0xEE, np.uint8)
    out_len = np.full(max(n, 1), 0x7777, np.uint64)
    in_used = np.full(max(n, 1), 0x7777, np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    rounds = np.zeros(max(n, 1), np.uint32)
    info = np.zeros(4, np.uint64)
    err = C.create_string_buffer(512)
    rc = lib().sim_dict_train(_p(inb), _p(in_off), _p(in_len), _p(nsamples), _p(sample_len), k, d, f, _p(out), _p(out_off), _p(out_cap),
                              _p(out_len), _p(in_used), _p(st), _p(rounds), n, fill, _p(info), err, 512)
    dicts = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)] if rc == 0 else None
    return dict(rc=rc, err=err.value.decode(), dicts=dicts, out_len=out_len[:n].copy(), in_used=in_used[:n].copy(), status=st[:n].copy(),
                rounds=rounds[:n].copy(), out=out, out_off=out_off[:n], out_cap=out_cap[:n], scratch=int(info[0]), launches=int(info[1]),
                bound=int(info[2]))


def plan_only(in_len, out_cap, nsamples, sample_len, k=256, d=8, f=20, null=None):
    """rcx_plan_train over sizes alone -> (rc, err).  null: the name of an array to hand over as a null pointer."""
    a = dict(in_len=np.array(in_len, np.uint64), out_cap=np.array(out_cap, np.uint64), nsamples=np.array(nsamples, np.uint32),
             sample_len=np.array(sample_len or [0], np.uint64))
    n = len(in_len)
    if null:
        a[null] = None
    err = C.create_string_buffer(512)
    rc = lib().sim_dict_train_plan(_p(a["in_len"]), _p(a["out_cap"]), _p(a["nsamples"]), _p(a["sample_len"]), k, d, f, n, err, 512)
    return rc, err.value.decode()


def untouched_outside(r):
    """only slot bytes were written (bytes of a slot beyond out_len are unspecified), and every byte between the slots is the sentinel"""
    mask = np.ones(r["out"].size, bool)
    for o, c in zip(r["out_off"], r["out_cap"]):
        mask[int(o):int(o) + int(c)] = False
    return bool((r["out"][mask] == 0xEE).all())
