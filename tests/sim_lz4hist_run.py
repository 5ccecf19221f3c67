"""Builds and drives tests/sim_lz4hist/sim_lz4hist.cpp: the LZ4 HC encoder with history on the wave64 simulator (TEST
INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_lz4hist", "build", "libsim_lz4hist.so")
SEG = 65536
ELEN = SEG + 64
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_lz4hist", "sim_lz4hist.cpp"), ("k_lz4_hc.hip", "k_lz4_hc_hist.hip", "lz_match.h", "rcx_dev.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.sim_lz4hist_scratch_bytes.restype = C.c_uint64
    return _lib


def bound(n):
    return n + n // 255 + 20


LAYOUT = ("link", "cand", "elen", "seg_first", "seg_nm", "seg_fm", "seg_le", "cap", "hslot")
LAUNCHES = ("plan", "hist_plan", "links", "search", "parse", "scan", "place")
ALL = 0xFFFFFFFF


def pack(blocks, hists, leads=0, front=None):
    """The input buffer: per block `lead` bytes (0xC3, or front[i]: the bytes that end right in front of the history), the history,
    the block.  -> (uint8 array, in_off)"""
    buf, offs = bytearray(), []
    for i, (r, h) in enumerate(zip(blocks, hists)):
        lead = leads[i] if isinstance(leads, (list, tuple)) else leads
        buf += front[i] if front is not None and front[i] is not None else b"\xC3" * lead
        buf += h or b""
        offs.append(len(buf))
        buf += r
    return np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8).copy(), np.array(offs or [0], np.uint64)


def run(inb, in_off, lens, hist_len, level, caps=None, stop_after=ALL, fill=0xA5, null_hist=False):
    """An encode at `level` of the blocks inb[in_off[i] : in_off[i] + lens[i]] with hist_len[i] bytes of history in front of each, of
    which the first stop_after launches run.  -> (rc, outputs, status, out_len, in_used, views): views[i] = the stage arrays of block
    i as the launches left them: link (history and block: hist + len entries), cand (per position of the block; valid before the
    parse ran), seg_nm / seg_fm / seg_le / elen per segment."""
    n = len(lens)
    in_len = np.array(list(lens) or [0], np.uint64)
    in_off = np.ascontiguousarray(in_off, np.uint64)
    hist = np.array([min(int(h), 65535) for h in hist_len] or [0], np.uint32)
    caps = [bound(int(l)) for l in lens] if caps is None else caps
    out_cap = np.array(list(caps) or [0], np.uint64)
    out_off = np.concatenate([[0], np.cumsum(out_cap)[:-1]]).astype(np.uint64)
    out = np.full(int(out_cap.sum()) + 16, 0xEE, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    nhist = 0 if null_hist else int((hist[:n] > 0).sum())
    segs = sum((int(l) + SEG - 1) // SEG for l in lens)
    sb = int(lib().sim_lz4hist_scratch_bytes(C.c_uint32(n), C.c_uint64(segs), C.c_uint64(nhist)))
    scratch = np.full(sb + 64, fill, np.uint8)
    lay = np.zeros(len(LAYOUT), np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_lz4hist_stages(level, P(inb), P(in_off), P(in_len), None if null_hist else P(hist), P(out), P(out_off), P(out_cap),
                                  P(out_len), P(in_used), P(st), n, C.c_uint32(nhist), C.c_uint32(stop_after), P(scratch), C.c_uint64(sb),
                                  P(lay))
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    lay = {k: int(v) for k, v in zip(LAYOUT, lay)}
    views = views_of(scratch, lay, lens, [0] * n if null_hist else hist[:n], st[:n] if stop_after >= 6 else None) if rc == 0 else None
    return rc, outs, st[:n].copy(), out_len[:n].copy(), in_used[:n].copy(), views


def views_of(scratch, lay, lens, hist, status=None):
    """per block the stage arrays (copies) of a scratch laid out by hc_hist_carve; None for a block without segments"""
    n = len(lens)
    arr = lambda off, dt, cnt: np.frombuffer(scratch, dt, cnt, off).copy() if cnt else np.zeros(0, dt)
    first = arr(lay["seg_first"], np.uint32, n + 1)
    hslot = arr(lay["hslot"], np.uint32, n + 1)
    views = []
    for b in range(n):
        f0, ns, ln, h = int(first[b]), int(first[b + 1]) - int(first[b]), int(lens[b]), int(hist[b])
        if ns == 0:
            views.append(None)
            continue
        assert ns == (ln + SEG - 1) // SEG and f0 + ns <= lay["cap"]
        own = 1 if h else 0
        assert int(hslot[b + 1]) - int(hslot[b]) == own
        v0 = (f0 + int(hslot[b]) + own) * SEG - h                 # the link array's entry of virtual position 0
        views.append({"link": arr(lay["link"] + 2 * v0, np.uint16, h + ln),
                      "cand": arr(lay["cand"] + 4 * f0 * SEG, np.uint32, ln),
                      "elen": arr(lay["elen"] + 4 * f0 * ELEN, np.uint32, ns * ELEN).reshape(ns, ELEN),
                      "seg_nm": arr(lay["seg_nm"] + 4 * f0, np.uint32, ns),
                      "seg_fm": arr(lay["seg_fm"] + 4 * f0, np.uint32, ns),
                      "seg_le": arr(lay["seg_le"] + 4 * f0, np.uint32, ns)})
    return views


def encode(blocks, hists, level, leads=0, front=None, **kw):
    """blocks[i] behind hists[i] (bytes or None) -> run(...)"""
    inb, off = pack(blocks, hists, leads, front)
    return run(inb, off, [len(r) for r in blocks], [len(h or b"") for h in hists], level, **kw)


def _job(args):
    kind, a, kw = args
    return (encode if kind == "encode" else run)(*a, **kw)


def run_many(jobs, workers=None):
    """jobs: ("encode" | "run", args, kwargs), in forked worker processes -> the results in the jobs' order"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    build()
    workers = workers or max(1, min(len(jobs), os.cpu_count() or 1))
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("fork")) as ex:
        return list(ex.map(_job, jobs))
