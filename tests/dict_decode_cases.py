"""Inputs for the tests of the decoders behind shared dictionaries (TEST INFRASTRUCTURE, shared by test_wavesim_dict_decode.py and
test_gpu_dict_decode.py).  A DBatch holds dictionaries and compressed streams and lays them out twice: SHARED -- every dictionary once
in the input buffer, before or behind the streams, which name it by offset and length -- and REPLICATED -- every stream's dictionary
directly in front of its output slot, what the history decoders take (the oracle: k_lz4_linked / k_inflate_hist on the simulator,
rcx_lz4_decode_linked_batch / rcx_inflate_hist_batch / rcx_zlib_decode_dict_batch on the device)."""
import zlib

import numpy as np

import corpus
import deflate_hist_cases as DH
import dict_shared_cases as S
import lz4_frame_inputs as LI
import lz4_frame_ref as R

FAMILIES = ("lz4", "deflate")
DICTS = {"deflate": (0, 1, 3, 4, 15, 16, 17, 111, 112, 113, 127, 128, 129, 258, 4096, 32767, 32768)}
DICTS["lz4"] = DICTS["deflate"] + (65535, 65536)
LENS = (0, 1, 5, 258, 1000, 65536, 65836)
E_MALFORMED, E_OUTPUT_TOO_SMALL, E_INVALID_HUFFMAN_CODE = 3, 2, 15
rand, text = S.rand, S.text


class DBatch(S.Batch):
    """kind: lz4 / deflate / zlib.  blocks = the compressed streams, caps = the slots, ids = the DICTIDs the decoder is told (zlib);
    want[i] = (status, bytes) where the case knows them, else None"""

    def __init__(self, kind):
        S.Batch.__init__(self, "lz4" if kind == "lz4" else "deflate")
        self.kind, self.ids, self.want = kind, [], []

    def rec(self, name, stream, d, cap, did=0, want=None):
        self.add(name, stream, d, cap)
        self.ids.append(did)
        self.want.append(want)

    def reorder(self, order):
        B = DBatch(self.kind)
        B.dicts = list(self.dicts)
        for i in order:
            B.rec(self.names[i], self.blocks[i], self.of[i], self.caps[i], self.ids[i], self.want[i])
        return B

    def layout(self):
        """the shared layout -> (buffer, in_off, in_len, dict_off, dict_len).  The buffer ends with the last thing placed in it: where
        that is a dictionary without bytes behind it, the dictionary ends at the buffer's last byte."""
        buf, in_off, lens, d_off, d_len = self.shared()
        return buf[:-16].copy(), in_off, lens, d_off, d_len

    def slots(self):
        """-> (out_off, out_cap, buffer size): the first slot at offset 0, the others three sentinels or more apart, their offsets
        running through every residue mod 16"""
        off, at = [], 0
        for i, c in enumerate(self.caps):
            if i:
                at += 3
                at += ((7 * i + 1) - at) % 16
            off.append(at)
            at += c
        return off, list(self.caps), at + 19

    def front(self, i):
        """what lies in front of block i's dictionary in the shared layout (a bait, or a lead of one to three bytes)"""
        if self.of[i] is None:
            return b"\xC3" * (1 + i % 3)
        d = self.dicts[self.of[i]]
        return d[1] if d[4] is None else b"\xC3"


def shared_job(B):
    """the decode behind shared dictionaries on the simulator: a job of sim_dict_decode_run.run_many"""
    buf, in_off, lens, d_off, d_len = B.layout()
    out_off, caps, size = B.slots()
    return ("run", (B.kind, buf, in_off, lens, d_off, d_len, out_off, caps, size), {"dict_id": B.ids if B.kind == "zlib" else None})


def hist_job(B):
    """the same streams through the history kernel on the replicated layout (slots at the same residues mod 16)"""
    n = len(B.blocks)
    dicts = [B.dictionary(i) for i in range(n)]
    if B.kind == "lz4":
        return ("sim_lz4frame_run.decode_linked", (list(B.blocks), [0] * n, list(B.caps), dicts), {})
    out_off = B.slots()[0]
    return ("dict_decode_cases.inflate_hist", (list(B.blocks), dicts, list(B.caps), B.kind == "zlib", list(B.ids), [B.front(i) for i in range(n)],
                                               [(o - len(d)) % 16 for o, d in zip(out_off, dicts)]), {})


def inflate_hist(streams, dicts, caps, zl, ids, fronts, misalign):
    import sim_deflate_hist_run as HR
    return HR.inflate(streams, [d or None for d in dicts], caps, zlib=zl, dict_id=ids if zl else None, fronts=fronts, misalign=misalign)


def hist_results(B, r):
    """a history runner's answer as (status, out_len, in_used, flags or None, outputs)"""
    if B.kind == "lz4":
        st, out_len, in_used, _, out, out_off, _ = r
        return st, out_len, in_used, None, [bytes(out[int(o):int(o) + int(l)]) for o, l in zip(out_off, out_len)]
    outs, out_len, in_used, st, flags = r
    return st, out_len, in_used, flags, outs


def check(B, got, ref):
    """got: sim_dict_decode_run.run's dict (or the library's, in the same form); ref: hist_results(...).  Bytes, out_len, in_used, status,
    flags; nothing outside the slots written; the cases' own expectations."""
    import sim_dict_decode_run as DR
    st, out_len, in_used, flags, outs = ref
    n = len(B.blocks)
    bad = [B.names[i] for i in range(n) if int(got["status"][i]) != int(st[i]) or int(got["out_len"][i]) != int(out_len[i])
           or int(got["in_used"][i]) != int(in_used[i]) or got["outputs"][i] != outs[i]
           or (flags is not None and int(got["flags"][i]) != int(flags[i]))]
    assert not bad, (B.kind, bad[:8], len(bad))
    out_off, caps, _ = B.slots()
    assert DR.only_slots_changed(got["out"], out_off, caps), "a byte outside the slots was written"
    for i, w in enumerate(B.want):
        if w is not None:
            assert int(got["status"][i]) == w[0] and (w[1] is None or got["outputs"][i] == w[1]), (B.names[i], int(got["status"][i]), w[0])


# ------------------------------------------------------------------------------------------------------------------------ streams
def lz4_block(rng, dct, n):
    """an LZ4 block that decodes to exactly n bytes behind dct: random literals, matches whose offsets reach anywhere into dictionary +
    block so far (half of them into the dictionary), now and then long or self-overlapping"""
    hist = bytes(dct)[-65535:]
    seqs, produced = [], 0
    while n - produced > 40:
        room = n - produced - 12
        L = min(int(rng.choice([0, 0, 1, 2, 3, 6, 14, 15, 16, 40, 300])), room - 4)
        if produced == 0 and not hist and L == 0:
            L = 1
        lit = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        produced += L
        reach = min(len(hist) + produced, 65535)
        if hist and rng.random() < 0.5 and reach > produced:
            off = int(rng.integers(produced + 1, reach + 1))
        else:
            off = int(rng.integers(1, reach + 1))
        if rng.random() < 0.1:
            off = min(reach, int(rng.choice([1, 2, 3, 15, 16, 17, 33])))
        M = int(rng.choice([4, 5, 8, 18, 19, 20, 64, 65, 70, 300, 1100])) if rng.random() < 0.3 else int(rng.integers(4, 19))
        M = max(4, min(M, room - L))
        seqs.append((lit, M, off))
        produced += M
    b = corpus.lz4_stream(seqs, rng.integers(0, 256, n - produced, dtype=np.uint8).tobytes())
    assert len(R.block_decode(b, hist)) == n
    return b


def lz_apply(hist, seqs, tail):
    """what LZ4 sequences decode to behind hist"""
    buf = bytearray(hist)
    for lit, m, off in seqs:
        buf += lit
        for _ in range(m):
            buf.append(buf[-off])
    return bytes(buf[len(hist):]) + tail


_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def grid(family, part):
    """dictionary lengths x block lengths; part 0: the blocks up to 1000 bytes, 1: the long ones.  Dictionaries at leads of 1-3 bytes,
    every other one behind the blocks; the last one placed ends at the buffer's last byte."""
    def make():
        B = DBatch(family)
        rng = np.random.default_rng(900 + part)
        k = 0
        for h in DICTS[family]:
            for n in LENS:
                if (n > 1000) != bool(part):
                    continue
                t = text(h + n, 100 + k)
                last = h == DICTS[family][-1] and n == [x for x in LENS if (x > 1000) == bool(part)][-1]
                d = B.dict(t[:h], front=b"\xC3" * (1 + k % 3), behind=b"" if last else b"\x3C\x3C", after=last or bool(k & 1)) if h else None
                if family == "lz4":
                    B.rec("h%d n%d" % (h, n), lz4_block(rng, t[:h], n), d, n)
                    if h and not part:
                        blk, raw = LI.random_chain(rng, 1, t[:h], nseq=(5, 40))
                        B.rec("h%d chain" % h, blk[0], d, len(raw[0]))
                else:
                    for m in DH.MODES:
                        if n > 1000 and m in (1, 9):
                            continue
                        B.rec("libz %s h%d n%d" % (m, h, n), DH.libz_stream(t[:h], t[h:], m), d, n, want=(0, t[h:]))
                k += 1
        return B
    return _memo(("grid", family, part), make)


def hand(family):
    """the hand-assembled cases: the dictionary's end at every residue mod 16 under a match that crosses it, first-symbol matches on both
    sides of every path's threshold, the reach, the bait pair, a slot one byte short"""
    def make():
        B = DBatch(family)
        lz4 = family == "lz4"
        ML = 300 if lz4 else 258

        def match_first(d, D):
            """the first symbol a match of ML bytes at distance d, then a literal and a short match"""
            if lz4:
                return corpus.lz4_stream([(b"", ML, d), (b"A", 7, 2)], b"tail!"), lz_apply(D, [(b"", ML, d), (b"A", 7, 2)], b"tail!")
            toks = DH.first_match_tokens(d)
            return DH.fixed_stream(toks), DH.lz_apply(D, toks)
        # the dictionary's end at every residue mod 16 of the buffer (the far gather splits there), the split at every byte of a gather
        for r in range(16):
            D = rand(200, 700 + r)
            d = B.dict(D, front=b"\xC3", behind=rand(40, 720 + r))           # (241 bytes apart: sixteen consecutive ends, every residue)
            s, w = match_first(112 + r, D)
            B.rec("end residue %d" % r, s, d, len(w), want=(0, w))
        D = rand(300, 11)
        d = B.dict(D, front=b"\xC3\xC3", behind=rand(300, 12))
        for dist in (1, 2, 3, 15, 16, 17, 111, 112, 113, 299, 300):
            s, w = match_first(dist, D)
            B.rec("first match d%d" % dist, s, d, len(w), want=(0, w))
        # the reach: output so far + dictionary, exactly; one more is an error, with the wanted byte as bait in front of the dictionary
        D = rand(100, 13)
        d = B.dict(D, front=b"\xC3" + rand(64, 14))
        bad = E_MALFORMED if lz4 else E_INVALID_HUFFMAN_CODE
        if lz4:
            B.rec("reach end+dict", corpus.lz4_stream([(b"FGHIJ", 9, 105)], b""), d, 14, want=(0, lz_apply(D, [(b"FGHIJ", 9, 105)], b"")))
            B.rec("reach end+dict+1", corpus.lz4_stream([(b"FGHIJ", 9, 106)], b""), d, 14, want=(bad, b""))
            B.rec("reach bait", corpus.lz4_stream([(b"", 9, 101)], b""), d, 9, want=(bad, b""))
            B.rec("offset 0", corpus.lz4_stream([(b"ab", 9, 0)], b""), d, 11, want=(bad, b""))
            for D16 in (65534, 65535, 65536):
                hd = rand(D16, 15)
                dd = B.dict(hd, front=b"\xC3" + hd[:2], after=D16 == 65535)
                # offset 65535 at position 0: the first byte of 65535, the second of 65536 (of which the first is out of reach)
                B.rec("off65535 D%d p0" % D16, corpus.lz4_stream([(b"", 20, 65535)], b""), dd, 20,
                      want=(bad, b"") if D16 == 65534 else (0, hd[D16 - 65535:][:20]))
                B.rec("off65535 D%d p1" % D16, corpus.lz4_stream([(b"\x09", 20, 65535)], b""), dd, 21, want=(0, b"\x09" + hd[D16 - 65534:][:20]))
        else:
            for c in DH.decode_cases():
                if c["name"].startswith("libz") or c["name"].startswith("first match"):
                    continue
                dd = B.dict(c["hist"], front=c["front"] or b"\xC3\xC3") if c["hist"] else None
                B.rec(c["name"], c["stream"], dd, c["cap"], want=(c["status"], c["want"]))
        # bait pair: twin dictionaries, different bytes directly behind them, a match that crosses the dictionary's end (100 bytes at
        # distance 130: the dictionary's last 130 bytes, then the block's own first bytes)
        A = rand(1000, 60)
        s, w = match_first(130, A)
        B.rec("end bait x", s, B.dict(A, front=b"\xC3\xC3", behind=rand(300, 61)), len(w), want=(0, w))
        B.rec("end bait y", s, B.dict(A, front=b"\xC3\xC3", behind=rand(300, 62), after=True), len(w), want=(0, w))
        # a slot one byte short, between good ones
        dA = B.dict(A, front=b"\xC3")
        B.rec("before short slot", s, dA, len(w) + 9, want=(0, w))
        B.rec("short slot", s, dA, len(w) - 1, want=(E_OUTPUT_TOO_SMALL, None))
        B.rec("after short slot", s, dA, len(w), want=(0, w))
        return B
    return _memo(("hand", family), make)


def zlib_cases():
    """the seven zlib_decode_cases() (FDICT, DICTID, the trailer over the block alone), each stream behind the dictionary it is told;
    the last one's dictionary, which its stream does use, ends at the buffer's last byte"""
    def make():
        B = DBatch("zlib")
        cs = DH.zlib_decode_cases()
        for k, c in enumerate(cs):
            D = c["hist"][len(c["hist"]) - c["told"]:] if c["told"] else b""
            last = k == len(cs) - 1
            d = B.dict(D, front=b"\xC3" * (1 + k % 3), behind=b"" if last else b"\x3C\x3C", after=last or bool(k & 1)) if D else None
            B.rec(c["name"], c["stream"], d, len(c["want"]) if c["status"] in (0, DH.E_ZLIB_CHECKSUM) else 16, did=c["dict_id"],
                  want=(c["status"], c["want"] if c["status"] == 0 else None))
        return B
    return _memo(("zlib",), make)


def case_batches(family):
    return [grid(family, 0), grid(family, 1), hand(family)] + ([zlib_cases()] if family == "deflate" else [])


def _stream(family, rng, D, rec, k):
    if family == "lz4":
        blk, raw = LI.random_chain(rng, 1, D, nseq=(5, 40))
        return blk[0], len(raw[0])
    return DH.libz_stream(D, rec, (1, 6, 9, "fixed")[k % 4]), len(rec)


def sharing(family, order=0):
    """300 records over three dictionaries -- two of them ranges of one text that overlap but differ -- and none; order 1: reversed"""
    def make():
        B = DBatch(family)
        t = text(9000, 300)
        d0 = B.dict(t[:8000], front=b"\xC3", behind=t[8000:] + b"\x3C")
        d1 = B.dict_within(d0, 100, 8000)
        d2 = B.dict(text(4096, 301), front=b"\xC3\xC3", after=True)
        rng = np.random.default_rng(302)
        for i in range(300):
            d = (d0, d1, d2, None)[i % 4]
            D = B.dicts[d][0] if d is not None else b""
            s, n = _stream(family, rng, D, text(int(rng.integers(200, 2001)), 400 + i), i)
            B.rec("rec %d" % i, s, d, n)
        return B
    B = _memo(("sharing", family), make)
    return B.reorder(range(len(B.blocks) - 1, -1, -1)) if order else B


def many(family, nblocks=8200, ndict=1030):
    """more blocks than a grid of 8192: block i is a copy of its dictionary, the 16 bytes at 16 * (i % ndict) of a random buffer"""
    def make():
        B = DBatch(family)
        Rb = rand(16 * ndict, 500)
        ds = [B.dict(Rb[16 * j:16 * j + 16], front=b"", behind=b"", after=True) for j in range(ndict)]
        for i in range(nblocks):
            D = Rb[16 * (i % ndict):16 * (i % ndict) + 16]
            s = corpus.lz4_stream([(b"", 11, 16)], D[11:]) if family == "lz4" else DH.fixed_stream([(16, 16)])
            B.rec("copy %d" % i, s, ds[i % ndict], 16, want=(0, D))
        return B
    return _memo(("many", family), make)


def corrupted(family, n=600, seed=5):
    """n streams behind one 32 KiB text dictionary, three in four with one to three flipped bits"""
    def make():
        B = DBatch(family)
        rng = np.random.default_rng(seed)
        D = text(32768, 77)
        d = B.dict(D, front=b"\xC3\xC3")
        for i in range(n):
            s, ln = _stream(family, rng, D, text(int(rng.integers(200, 801)), 1000 + i), i)
            s = bytearray(s)
            if i % 4:
                for _ in range(int(rng.integers(1, 4))):
                    s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            B.rec("stream %d" % i, bytes(s), d, ln + 64)
        return B
    return _memo(("corrupted", family, n, seed), make)
