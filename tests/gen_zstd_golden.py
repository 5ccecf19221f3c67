"""Writes tests/golden/zstd/*.zst and manifest.json.  Run once by hand where ctypes finds libzstd.so.1 (1.4.8 wrote the committed
files): python tests/gen_zstd_golden.py.  The raw inputs are recipes (tests/zstd_cases.raw_of), not files; every frame stays under
100 KiB.  Each entry names what its frame must reach (`needs`, the words of zstd_cases.props); the generator decodes what it wrote
with tests/zstd_ref.py and asserts them, so that another library version cannot silently lose a path.  FRAMES are the manifest's
"frames" (zstd_cases.golden()), MORE its "more" (zstd_cases.golden_more())."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import zstd_cases as cases  # noqa: E402
import zstd_ref as R  # noqa: E402

LIMIT = 100 * 1024
LEVEL, WINDOW_LOG, CHECKSUM = 100, 101, 201            # ZSTD_cParameter


class Buf(C.Structure):
    _fields_ = [("p", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def lib():
    z = C.CDLL("libzstd.so.1")
    for f in ("ZSTD_compress2", "ZSTD_compressBound", "ZSTD_CCtx_setParameter", "ZSTD_CCtx_loadDictionary", "ZSTD_compressStream2", "ZSTD_isError"):
        getattr(z, f).restype = C.c_size_t
    z.ZSTD_createCCtx.restype = C.c_void_p
    z.ZSTD_versionString.restype = C.c_char_p
    return z


def compress(z, raw, level=3, window_log=0, checksum=False, dictionary=None, stream=False):
    cctx = C.c_void_p(z.ZSTD_createCCtx())
    chk = lambda r: (_ for _ in ()).throw(RuntimeError("libzstd error %d" % r)) if z.ZSTD_isError(C.c_size_t(r)) else r
    chk(z.ZSTD_CCtx_setParameter(cctx, LEVEL, level))
    if window_log:
        chk(z.ZSTD_CCtx_setParameter(cctx, WINDOW_LOG, window_log))
    if checksum:
        chk(z.ZSTD_CCtx_setParameter(cctx, CHECKSUM, 1))
    if dictionary:
        chk(z.ZSTD_CCtx_loadDictionary(cctx, dictionary, C.c_size_t(len(dictionary))))
    cap = z.ZSTD_compressBound(C.c_size_t(len(raw))) + 64
    dst = C.create_string_buffer(cap)
    if not stream:
        n = chk(z.ZSTD_compress2(cctx, dst, C.c_size_t(cap), raw, C.c_size_t(len(raw))))
    else:                                               # no pledged size: the frame declares none
        src = C.create_string_buffer(raw, len(raw) or 1)
        ib, ob = Buf(C.addressof(src), len(raw), 0), Buf(C.addressof(dst), cap, 0)
        while ib.pos < ib.size:                         # ZSTD_e_continue first: ZSTD_e_end in the first call would pledge the size
            chk(z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), 0))
        while chk(z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), 2)):
            pass
        n = ob.pos
    z.ZSTD_freeCCtx(cctx)
    return dst.raw[:n]


T = lambda n, s=7: ["synth", "text", n, s]
RUNS = lambda n: ["synth", "runs", n, 7]
FRAMES = [
    # name, raw recipe, compress arguments, what the frame must reach
    ("empty", ["hex", ""], {}, ["raw_block_of_0"]),
    ("one_byte", ["hex", "78"], {}, ["raw_block"]),
    ("rand_5000", ["synth", "rand", 5000, 7], {}, ["raw_block"]),
    ("zeros_200000", ["zeros", 200000], {}, ["rle_block", "compressed_block", "lit_raw", "three_predef"]),
    ("text_5000_l3", T(5000), {}, ["huf4_fse", "three_fse", "nseq2"]),
    ("runs_5000_l3", RUNS(5000), {}, ["huf1_fse"]),
    ("bits3_4000_l1", ["bits3", 4000, 7], {"level": 1}, ["huf1_direct"]),
    ("bits3_4000_l19", ["bits3", 4000, 7], {"level": 19}, ["huf4_direct"]),
    ("abc_3000", ["rep", "616263", 3000], {}, ["overlap"]),
    ("text_8000_l19_w12", T(8000), {"level": 19, "window_log": 12}, ["blocks=2", "treeless4", "ll_repeat", "window"]),
    ("text_3000_l19_w10", T(3000), {"level": 19, "window_log": 10}, ["blocks=3", "of_repeat"]),
    ("text_40000_l19_w10", T(40000), {"level": 19, "window_log": 10}, ["blocks=40", "ml_repeat", "lit_raw", "huf4_fse"]),
    ("runs_3000_l1_w10", RUNS(3000), {"level": 1, "window_log": 10}, ["of_rle"]),
    ("runs_40000_l3_w10", RUNS(40000), {"window_log": 10}, ["ll_rle", "treeless1"]),
    ("words_20000_l1_w10", ["synth", "words", 20000, 7], {"level": 1, "window_log": 10}, ["treeless1"]),
    ("text_300000_l3_sum", T(300000), {"checksum": True}, ["blocks=3", "checksum", "fcs4"]),
    ("text_300000_l19_sum", T(300000), {"level": 19, "checksum": True}, ["far", "checksum"]),
    ("stream_no_size", T(6000, 3), {"stream": True}, ["fcs0", "window"]),
    ("record_behind_dictionary", T(2048, 9), {"dict": T(32768, 1)}, ["dict"]),
]
# written to the manifest's "more" (zstd_cases.golden_more()): libzstd alone writes Huffman streams, so the literals header of 5 bytes
# and a literals section that fills a block need frames of its making
MORE = [
    ("rand200_20000_l3", ["randmod", 20000, 7, 200], {}, ["hufhdr5"]),
    ("rand48_131072_l1", ["randmod", 131072, 7, 48], {"level": 1}, ["hufhdr5", "lit_full"]),
]


def write(z, entries):
    frames = []
    for name, recipe, args, needs in entries:
        raw = cases.raw_of(recipe)
        args = dict(args)
        drecipe = args.pop("dict", None)
        d = cases.raw_of(drecipe) if drecipe else None
        blob = compress(z, raw, dictionary=d, **args)
        assert len(blob) < LIMIT, (name, len(blob))
        trace = []
        data, used = R.decode(blob, d or b"", trace=trace)
        assert data == raw and used == len(blob), name
        got = cases.props(trace)
        missing = [w for w in needs if w not in got]
        assert not missing, "%s does not reach %s (it reaches %s)" % (name, missing, sorted(got))
        if d:
            plain = compress(z, raw, **args)
            print("  (%d bytes without the dictionary)" % len(plain))
        with open(os.path.join(cases.GOLDEN, name + ".zst"), "wb") as fh:
            fh.write(blob)
        e = {"name": name, "file": name + ".zst", "raw": recipe, "needs": needs, "bytes": len(blob)}
        if drecipe:
            e["dict"] = drecipe
        frames.append(e)
        print("%-28s %7d -> %6d  %s" % (name, len(raw), len(blob), " ".join(needs)))
    return frames


def main():
    z = lib()
    print("libzstd", z.ZSTD_versionString().decode())
    os.makedirs(cases.GOLDEN, exist_ok=True)
    frames, more = write(z, FRAMES), write(z, MORE)
    with open(os.path.join(cases.GOLDEN, "manifest.json"), "w") as fh:
        json.dump({"libzstd": z.ZSTD_versionString().decode(), "frames": frames, "more": more}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
