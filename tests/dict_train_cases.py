"""The jobs of the dictionary-training tests and their serial reference (TEST INFRASTRUCTURE, shared by test_wavesim_dict_train.py and
test_gpu_dict_train.py).  A job is (name, samples, C, k, d, f); the reference is tests/dict_train_ref/dict_train_ref.cpp, written from the
specification of DESIGN.md 3.19 by definition and built here with g++."""
import ctypes as C
import os
import subprocess

import numpy as np

from rust_compress_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(HERE, "dict_train_ref", "build", "libdict_train_ref.so")
_ref = None
_memo = {}


def ref_lib():
    global _ref
    if _ref is None:
        src = os.path.join(HERE, "dict_train_ref", "dict_train_ref.cpp")
        if not (os.path.exists(REF_OUT) and os.path.getmtime(REF_OUT) >= os.path.getmtime(src)):
            os.makedirs(os.path.dirname(REF_OUT), exist_ok=True)
            tmp = REF_OUT + ".%d" % os.getpid()
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-o", tmp, src])
            os.replace(tmp, REF_OUT)
        _ref = C.CDLL(REF_OUT)
        _ref.ref_dict_train.restype = C.c_int64
        _ref.ref_dict_train.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_uint64, C.c_void_p]
    return _ref


def ref_train(samples, cap, k=256, d=8, f=20, with_rounds=False):
    """the reference's dictionary (bytes) for one job; computed once per job and kept"""
    key = (tuple(samples), cap, k, d, f)
    if key not in _memo:
        corpus = np.frombuffer(b"".join(samples) + b"\0" * 8, np.uint8)
        lens = np.array([len(s) for s in samples] or [0], np.uint64)
        out = np.zeros(max(cap, 1), np.uint8)
        rounds = np.zeros(1, np.uint64)
        n = ref_lib().ref_dict_train(corpus.ctypes.data, sum(len(s) for s in samples), lens.ctypes.data, len(samples), k, d, f,
                                     out.ctypes.data, cap, rounds.ctypes.data)
        assert n >= 0, "the reference refused the job"
        _memo[key] = (bytes(out[:n]), int(rounds[0]))
    return _memo[key] if with_rounds else _memo[key][0]


def text(n, seed):
    return synth.gen("text", n, seed).tobytes()


def records(kind, count, size, seed0):
    return [synth.gen(kind, size, seed0 + i).tobytes() for i in range(count)]


def split(raw, sizes):
    """raw cut into samples of the given sizes, the rest as the last one"""
    out, at = [], 0
    for s in sizes:
        out.append(raw[at:at + s])
        at += s
    out.append(raw[at:])
    return out


def size_jobs(k=16, d=8):
    """the corpus and capacity edges: (name, samples, C, k, d, f)"""
    t = text(4096, 11)
    jobs = [("n=0", [], 1000, k, d, 20), ("n=0, one empty sample", [b""], 1000, k, d, 20), ("n<d", [t[:d - 1]], 1000, k, d, 20),
            ("n=d, k>n", [t[:d]], 1000, k, d, 20), ("n=k", [t[:k]], 1000, k, d, 20), ("n=k+1", [t[:k + 1]], 1000, k, d, 20)]
    for cap in (0, d - 1, d, k - 1, k, 1000, 4096, 32768):
        jobs.append(("C=%d" % cap, split(t, [700, 900, 1100]), cap, k, d, 20))
    return jobs


def param_jobs():
    t = text(24576, 12)
    jobs = []
    for d in (6, 8):
        for k in (d, 16, 64, 256):
            for f in (10, 20, 22):
                jobs.append(("d=%d k=%d f=%d" % (d, k, f), split(t, [5000, 3000, 9000]), 2048, k, d, f))
    big = text(49152, 13)
    for d in (6, 8):
        jobs.append(("d=%d k=4096" % d, split(big, [20000, 9000]), 8192, 4096, d, 20))
    return jobs


def batch_jobs():
    """12 jobs of different sizes and round counts for ONE call (k = 64, d = 8, f = 20), an empty job between two full ones"""
    t = text(65536, 14)
    w = synth.gen("words", 30000, 15).tobytes()
    r = synth.gen("runs", 20000, 16).tobytes()
    g = synth.gen("dna4", 9000, 17).tobytes()
    x = synth.gen("rand", 5000, 18).tobytes()
    return [("text 64K", split(t, [2048] * 31), 4096), ("words", split(w, [1000] * 20), 2048), ("empty", [], 512),
            ("runs", split(r, [7, 0, 3000]), 1000), ("dna4", [g], 300), ("rand", [x], 640), ("short", [t[:63]], 256),
            ("text 8K", split(t[:8192], [100, 5, 1, 4000]), 32768), ("C=0", [t[:4000]], 0), ("words 2", [w[:12000]], 777),
            ("one segment", [t[:64]], 64), ("text 20K", split(t[3000:23000], [9999]), 1500)]
