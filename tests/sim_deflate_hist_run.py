"""Builds and drives tests/sim_deflate_hist/sim_deflate_hist.cpp: the DEFLATE encoder (levels 2..9) and decoder with history on the
wave64 simulator (TEST INFRASTRUCTURE)."""
import ctypes as C
import os

import numpy as np

from wavesim.build import build_sim

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sim_deflate_hist", "build", "libsim_deflate_hist.so")
SEG = 65536
_lib = None


def build():
    return build_sim(OUT, os.path.join(HERE, "sim_deflate_hist", "sim_deflate_hist.cpp"),
                     ("k_deflate_encode.hip", "k_deflate_hc.hip", "k_deflate_hc_hist.hip", "k_inflate.hip", "k_inflate2.hip", "k_inflate_hist.hip", "k_crc32.hip", "lz_match.h", "rcx_dev.h"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.sim_deflate_hist_scratch_bytes.restype = C.c_uint64
    return _lib


def bound(n, fmt=0):
    """rcx_deflate_compression_bound(n), + 10 for the zlib form with a dictionary"""
    return n + 11 * ((n + SEG - 1) // SEG) + 2 + (10 if fmt else 0)


LAYOUT = ("link", "cand", "elen", "price", "pos", "seg_first", "seg_type", "seg_bits", "cap", "hslot", "end")
LAUNCHES = ("plan", "hist_plan", "links", "search", "price", "parse")          # of a raw encode, in order
SEARCH = 4                                                                     # stop_after: ... search (k_dh_parse leaves cand alone, later stages too)
ALL = 0xFFFFFFFF


def run(inb, in_off, lens, hist_len, level, fmt=0, dict_id=None, caps=None, stop_after=ALL, fill=0xA5, null_hist=False):
    """An encode at `level` (fmt 0 raw DEFLATE, 1 zlib with dict_id) of the blocks inb[in_off[i] : in_off[i] + lens[i]] with hist_len[i]
    bytes of history in front of each, of which the first stop_after launches run; fill None: the scratch is left as the allocator
    hands it out (a batch of very many blocks).  -> (rc, outputs, status, out_len, in_used, views, out, out_off): views[i] = the stage
    arrays of block i as the launches left them: link (history and block: hist + len entries), cand (per position of the block); out:
    the whole output buffer, which started as 0xEE."""
    n = len(lens)
    in_len = np.array(list(lens) or [0], np.uint64)
    in_off = np.ascontiguousarray(in_off, np.uint64)
    aux = np.zeros(2 * max(n, 1), np.uint32)
    aux[:n] = [int(h) for h in hist_len]
    if dict_id is not None:
        aux[n:2 * n] = dict_id
    caps = [bound(int(l), fmt) for l in lens] if caps is None else caps
    out_cap = np.array(list(caps) or [0], np.uint64)
    out_off = np.concatenate([[0], np.cumsum(out_cap)[:-1]]).astype(np.uint64)
    out = np.full(int(out_cap.sum()) + 16, 0xEE, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -1, np.int32)
    nhist = 0 if null_hist else int((aux[:n] > 0).sum())
    segs = sum((int(l) + SEG - 1) // SEG for l in lens)
    sb = int(lib().sim_deflate_hist_scratch_bytes(C.c_uint32(n), C.c_uint64(segs), C.c_uint64(nhist)))
    scratch = np.empty(sb + 64, np.uint8) if fill is None else np.full(sb + 64, fill, np.uint8)
    lay = np.zeros(len(LAYOUT), np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_deflate_hist_stages(fmt, level, P(inb), P(in_off), P(in_len), None if null_hist else P(aux), P(out), P(out_off),
                                       P(out_cap), P(out_len), P(in_used), P(st), n, C.c_uint32(nhist), C.c_uint32(stop_after),
                                       P(scratch), C.c_uint64(sb), P(lay))
    outs = [bytes(out[int(out_off[i]):int(out_off[i]) + int(out_len[i])]) for i in range(n)]
    lay = {k: int(v) for k, v in zip(LAYOUT, lay)}
    assert lay["end"] <= sb and lay["cap"] >= segs, (lay, sb, segs)
    views = views_of(scratch, lay, lens, [0] * n if null_hist else aux[:n]) if rc == 0 else None
    return rc, outs, st[:n].copy(), out_len[:n].copy(), in_used[:n].copy(), views, out, out_off[:n]


def views_of(scratch, lay, lens, hist):
    """per block the link and cand arrays (copies) of a scratch laid out by dh_hist_carve; None for a block without segments"""
    n = len(lens)
    arr = lambda off, dt, cnt: np.frombuffer(scratch, dt, cnt, off).copy() if cnt else np.zeros(0, dt)
    first = arr(lay["seg_first"], np.uint32, n + 1)
    hslot = arr(lay["hslot"], np.uint32, n + 1)
    views = []
    for b in range(n):
        f0, ns, ln, h = int(first[b]), int(first[b + 1]) - int(first[b]), int(lens[b]), min(int(hist[b]), 32768)
        if ns == 0:
            views.append(None)
            continue
        assert ns == (ln + SEG - 1) // SEG and f0 + ns <= lay["cap"]
        own = 1 if h else 0
        assert int(hslot[b + 1]) - int(hslot[b]) == own
        v0 = (f0 + int(hslot[b]) + own) * SEG - h                 # the link array's entry of virtual position 0
        views.append({"link": arr(lay["link"] + 2 * v0, np.uint16, h + ln), "cand": arr(lay["cand"] + 4 * f0 * SEG, np.uint32, ln)})
    return views


def pack(blocks, hists, leads=0, front=None):
    """The input buffer: per block `lead` bytes (0xC3, or front[i]), the history, the block.  -> (uint8 array, in_off)"""
    buf, offs = bytearray(), []
    for i, (r, h) in enumerate(zip(blocks, hists)):
        lead = leads[i] if isinstance(leads, (list, tuple)) else leads
        buf += front[i] if front is not None and front[i] is not None else b"\xC3" * lead
        buf += h or b""
        offs.append(len(buf))
        buf += r
    return np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8).copy(), np.array(offs or [0], np.uint64)


def encode(blocks, hists, level, leads=0, front=None, **kw):
    """blocks[i] behind hists[i] (bytes or None) -> run(...)"""
    inb, off = pack(blocks, hists, leads, front)
    return run(inb, off, [len(r) for r in blocks], [len(h or b"") for h in hists], level, **kw)


def decode_buffers(streams, hists, caps, fronts=None, misalign=None):
    """The decoders' buffers.  Input: the streams back to back.  ONE output buffer: per stream fronts[i] (default 0xC3 * 3), hists[i],
    the slot of caps[i] bytes (0xEE), 0x5A * 19; the first history byte lies misalign[i] bytes behind a 16-byte boundary of the
    buffer (which starts at one).  -> (inb, in_off, in_len, out, out_off, out_cap)"""
    n = len(streams)
    in_len = np.array([len(s) for s in streams] or [0], np.uint64)
    in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]]).astype(np.uint64)
    inb = np.frombuffer(b"".join(streams) + b"\0" * 16, np.uint8).copy()
    buf, offs = bytearray(b"\x5A" * 16), []
    for i in range(n):
        buf += fronts[i] if fronts is not None and fronts[i] is not None else b"\xC3" * 3
        if misalign is not None:
            buf += b"\x5A" * ((misalign[i] - len(buf)) % 16)
        buf += hists[i] or b""
        offs.append(len(buf))
        buf += b"\xEE" * caps[i] + b"\x5A" * 19
    raw = np.zeros(len(buf) + 64, np.uint8)
    sh = (-raw.ctypes.data) % 16
    out = raw[sh:sh + len(buf)]
    out[:] = np.frombuffer(bytes(buf), np.uint8)
    return inb, in_off, in_len, out, np.array(offs or [0], np.uint64), np.array(list(caps) or [0], np.uint64)


def only_slots_changed(out, before, out_off, out_cap):
    mask = np.ones(out.size, bool)
    for o, c in zip(out_off, out_cap):
        mask[int(o):int(o) + int(c)] = False
    return bool((out[mask] == before[mask]).all())


def inflate(streams, hists, caps, zlib=False, dict_id=None, fronts=None, misalign=None, hist_kernel=True, hist_len=None):
    """Streams decoded by k_inflate_hist (hist_kernel False: by k_inflate2, which knows no history) in decode_buffers(...).  hist_len:
    what the kernel is told (default: len(hists[i])).  Asserts that nothing but the slots changed (histories, fronts, sentinels).
    -> (outputs, out_len, in_used, status, flags)"""
    n = len(streams)
    inb, in_off, in_len, out, out_off, out_cap = decode_buffers(streams, hists, caps, fronts, misalign)
    before = out.copy()
    out_len = np.zeros(max(n, 1), np.uint64)
    in_used = np.zeros(max(n, 1), np.uint64)
    st = np.full(max(n, 1), -99, np.int32)
    aux = np.zeros(2 * max(n, 1), np.uint32)
    if hist_kernel:
        aux[:n] = [len(h or b"") for h in hists] if hist_len is None else hist_len
        if dict_id is not None:
            aux[n:2 * n] = dict_id
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib().sim_inflate_hist(1 if hist_kernel else 0, 1 if zlib else 0, P(inb), P(in_off), P(in_len), P(aux), P(out), P(out_off),
                                P(out_cap), P(out_len), P(in_used), P(st), n)
    assert rc == 0
    assert only_slots_changed(out, before, out_off[:n], out_cap[:n]), "the decoder wrote outside its slots (history, sentinels)"
    outs = [bytes(out[int(o):int(o) + int(l)]) for o, l in zip(out_off[:n], out_len[:n])]
    return outs, out_len[:n].copy(), in_used[:n].copy(), st[:n].copy(), aux[:n].copy()


def _job(args):
    kind, a, kw = args
    return {"encode": encode, "run": run, "inflate": inflate}[kind](*a, **kw)


def run_many(jobs, workers=None):
    """jobs: ("encode" | "run" | "inflate", args, kwargs), in forked worker processes -> the results in the jobs' order"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    build()
    workers = workers or max(1, min(len(jobs), os.cpu_count() or 1))
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("fork")) as ex:
        return list(ex.map(_job, jobs))
