"""Batch API over the C-ABI (include/rcx.h): host-memory batches (lists of bytes) and device-resident
batches (torch uint8 tensors, used by bench.py).  No CPU fallback, no oracle import."""
import ctypes as C

import numpy as np

from . import _native as N
from . import batch as B


def deflate_bound(n):
    """rcx_deflate_compression_bound(n): the largest raw DEFLATE stream the encoder makes from n bytes (zlib +6, gzip +18)."""
    return int(N.lib().rcx_deflate_compression_bound(n))


def _per_blob(zdict, n):
    """one dictionary for all blobs, or a list with one entry per blob"""
    if isinstance(zdict, (bytes, bytearray, memoryview)):
        return [bytes(zdict)] * n
    if len(zdict) != n:
        raise ValueError("zdict: bytes, or one entry (bytes or None) per blob")
    return [bytes(d) if d else b"" for d in zdict]


def _adler32(d):
    import zlib
    return zlib.adler32(d) if d else 0


def _ptr(a):
    """an optional array -> its address, or None: a null pointer"""
    return a.ctypes.data if a is not None else None


def _u64(a):
    """one of a batch's per-block arrays as the library reads it: contiguous uint64 (one zero where there is no block: memory behind the pointer)"""
    a = np.ascontiguousarray(a, np.uint64)
    return a if a.size else np.zeros(1, np.uint64)


def _slots(caps):
    """output capacities -> Context._batch's `out`: a zeroed buffer of 16-byte aligned slots, their offsets, the capacities"""
    total, off, cap = B.layout(caps)
    return np.zeros(total, dtype=np.uint8), off, cap


def _pack_hist(blobs, histories, limit):
    """the input buffer history, block, history, block, ...: -> (uint8 array, in_off, hist_len); a history's last `limit` bytes count"""
    buf, off, hl = bytearray(), [], []
    for blob, h in zip(blobs, histories):
        h = bytes(h)[-limit:] if h else b""
        buf += h
        off.append(len(buf))
        hl.append(len(h))
        buf += bytes(blob)
    return np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8), off, hl


def _pack_shared(blobs, dictionary, limit):
    """the input buffer of the *_shared calls: every distinct dictionary ONCE (its last `limit` bytes), then the blobs.  dictionary: bytes
    for all blobs, or a list with one entry (bytes or None) per blob.  -> (uint8 array, in_off, in_len, dict_off, dict_len, the dictionaries
    per blob)"""
    dicts = _per_blob(dictionary, len(blobs))
    buf, at = bytearray(), {}
    for d in dicts:
        d = d[-limit:]
        if d and d not in at:
            at[d] = len(buf)
            buf += d
    off, d_off, d_len = [], [], []
    for blob, d in zip(blobs, dicts):
        d = d[-limit:]
        off.append(len(buf))
        buf += bytes(blob)
        d_off.append(at[d] if d else 0)
        d_len.append(len(d))
    return np.frombuffer(bytes(buf) + b"\0" * 16, np.uint8), off, [len(b) for b in blobs], d_off, d_len, dicts


class RcxError(RuntimeError):
    pass


class BlockError(Exception):
    """One block failed: mirrors the reference's io::Error for that block."""

    def __init__(self, status, index=0):
        self.status = int(status)
        self.index = index
        msg = N.lib().rcx_status_string(int(status)).decode()
        super().__init__("block %d: status %d (%s)" % (index, status, msg))


class Result:
    __slots__ = ("outputs", "out_len", "in_used", "status", "aux")

    def __init__(self, outputs, out_len, in_used, status, aux):
        self.outputs, self.out_len, self.in_used, self.status, self.aux = outputs, out_len, in_used, status, aux

    def check(self):
        bad = np.nonzero(self.status)[0]
        if bad.size:
            raise BlockError(self.status[bad[0]], int(bad[0]))
        return self


class Context:
    """One rcx_ctx (one HIP device + stream).  Raises if there is no device: there is no CPU path."""

    def __init__(self, device=-1):
        self._h = C.c_void_p()
        rc = N.lib().rcx_ctx_create(device, C.byref(self._h))
        if rc != N.RC_OK:
            self._h = None
            raise RcxError("rcx_ctx_create failed rc=%d (%s)" % (rc, "no HIP device: this library has no CPU fallback"
                                                                 if rc == N.RC_NO_DEVICE else "HIP error"))

    def close(self):
        if getattr(self, "_h", None):
            N.lib().rcx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:           # interpreter shutdown: the module globals may already be gone
            pass

    def _chk(self, rc):
        if rc != N.RC_OK:
            raise RcxError("rcx call failed rc=%d: %s" % (rc, N.lib().rcx_last_error(self._h).decode()))

    def set_variant(self, codec, variant):
        self._chk(N.lib().rcx_ctx_set_variant(self._h, codec, variant))

    def set_stream(self, stream_ptr):
        self._chk(N.lib().rcx_ctx_set_stream(self._h, C.c_void_p(stream_ptr)))

    # ---------------- host-memory batches ----------------
    def _batch(self, fn_name, base, in_off, in_len, out, *extra, unpack=True):
        """THE host-memory call: builds the rcx_batch, calls fn_name, unpacks -> Result (aux None).  base: a numpy uint8 array; out: (buffer,
        out_off, out_cap), or None for the entry points without slots (the hashes: four null pointers).  extra: what follows the batch in
        include/rcx.h -- a numpy array goes as its address (the caller has made it contiguous and of the element type), None as a null
        pointer, anything else as it is.  unpack=False: outputs None, for the caller that reads the buffer itself (a chain of linked LZ4
        blocks shares its head's slot)."""
        n = len(in_off)
        in_off, in_len = _u64(in_off), _u64(in_len)
        if base.size == 0:
            base = np.zeros(1, np.uint8)
        buf, out_off, out_cap = (out[0], _u64(out[1]), _u64(out[2])) if out is not None else (None, None, None)
        out_len = np.zeros(max(n, 1), np.uint64)
        in_used = np.zeros(max(n, 1), np.uint64)
        status = np.zeros(max(n, 1), np.int32)
        b = N.Batch(_ptr(base), _ptr(in_off), _ptr(in_len), _ptr(buf), _ptr(out_off), _ptr(out_cap), _ptr(out_len) if out is not None else None,
                    _ptr(in_used), _ptr(status), n, N.MEM_HOST)
        args = [C.c_void_p(_ptr(a)) if a is None or isinstance(a, np.ndarray) else a for a in extra]
        self._chk(getattr(N.lib(), fn_name)(self._h, C.byref(b), *args))
        outs = None if not unpack else B.unpack(buf, out_off, out_len[:n]) if out is not None else [b""] * n
        return Result(outs, out_len[:n], in_used[:n], status[:n], None)

    def _run_host(self, fn_name, blobs, caps, extra_in=None, extra_out=False, n_out=None, needs_out=True, scalar=None):
        n = len(blobs)
        base, off, lens = B.pack(blobs)
        aux, extra = None, ()
        if scalar is not None:
            extra = (scalar,)
        elif extra_in is not None:
            aux = np.ascontiguousarray(extra_in, dtype=np.uint32)
            extra = (aux,)
        elif n_out is not None:
            extra = (np.ascontiguousarray(n_out, dtype=np.uint64),)
        elif extra_out:
            aux = np.zeros(max(n, 1), np.uint32)
            extra = (aux,)
        res = self._batch(fn_name, base, off, lens, _slots(caps if needs_out else [0] * n), *extra)     # (no output: slots of capacity 0)
        if not needs_out:
            res.outputs = [b""] * n
        res.aux = aux[:n] if aux is not None else None
        return res

    def lz4_decode_blocks(self, blobs, caps):
        return self._run_host("rcx_lz4_decode_batch", blobs, caps)

    def lz4_encode_blocks(self, blobs):
        return self._run_host("rcx_lz4_encode_batch", blobs, [max(int(N.lib().rcx_lz4_compression_bound(len(b))), 1) for b in blobs])

    def lz4_encode_hc_blocks(self, blobs, level=9, caps=None):
        """One LZ4 block per blob from the high-compression encoder (levels 1..12: rcx_lz4_encode_hc_batch).  The blocks decode
        with lz4_decode_blocks like the reference encoder's; caps default to rcx_lz4_compression_bound."""
        if caps is None:
            caps = [max(int(N.lib().rcx_lz4_compression_bound(len(b))), 1) for b in blobs]
        return self._run_host("rcx_lz4_encode_hc_batch", blobs, caps, scalar=int(level))

    def lz4_encode_hc_hist(self, base, in_off, in_len, hist_len, level=9, caps=None):
        """rcx_lz4_encode_hc_hist_batch over a buffer the caller laid out: block i is base[in_off[i] : in_off[i] + in_len[i]] (base: a
        numpy uint8 array) and its matches may reach into the hist_len[i] bytes below in_off[i] -- a dictionary put there, or the
        block before it (linked blocks).  hist_len None: no history."""
        if caps is None:
            caps = [max(int(N.lib().rcx_lz4_compression_bound(int(l))), 1) for l in in_len]
        return self._encode_hist("rcx_lz4_encode_hc_hist_batch", base, in_off, in_len, hist_len, level, caps)

    def _encode_hist(self, fn_name, base, in_off, in_len, hist_len, level, caps, dict_id=None):
        """one rcx_*_encode_hist_batch call (dict_id: rcx_zlib_encode_dict_batch) over a buffer the caller laid out (base: a numpy uint8 array)"""
        n = len(in_off)
        out = _slots(caps)
        hist = np.ascontiguousarray(hist_len, np.uint64) if hist_len is not None else None
        if hist is not None and hist.size != n:
            raise ValueError("hist_len: one entry per block")
        ids = (np.array(list(dict_id) or [0], np.uint32),) if dict_id is not None else ()
        return self._batch(fn_name, base, in_off, in_len, out, int(level), hist if n else None, *ids)     # (no block: a null pointer)

    def lz4_encode_hc_hist_blocks(self, blobs, histories, level=9, caps=None):
        """One LZ4 block per blob from the high-compression encoder, with HISTORY: histories[i] (bytes or None; its last 64 KiB count)
        is put directly in front of blobs[i] in the input buffer and the block's matches may reach into it.  The block decodes behind
        the same bytes (rcx_lz4_decode_linked_batch with dict_len, or any LZ4 decoder given them as its dictionary)."""
        if len(histories) != len(blobs):
            raise ValueError("histories: one entry (bytes or None) per blob")
        base, off, hl = _pack_hist(blobs, histories, 65536)
        return self.lz4_encode_hc_hist(base, off, [len(b) for b in blobs], hl, level, caps)

    def _shared(self, fn_name, base, in_off, in_len, dict_off, dict_len, caps, level=None, flags=False, dict_id=None):
        """one rcx_*_shared_batch call over a buffer the caller laid out (base: a numpy uint8 array): an encode (level) or a decode (flags: the
        entry point fills a flags array, the result's aux).  Nothing lies in front of a slot."""
        n = len(in_off)
        out = _slots(caps)
        if (dict_off is None) != (dict_len is None):
            raise ValueError("dict_off and dict_len: both or neither")
        d_off = d_len = None
        if dict_len is not None:
            d_off, d_len = _u64(dict_off), _u64(dict_len)
            if n and (d_off.size != n or d_len.size != n):
                raise ValueError("dict_off, dict_len: one entry per block")
        extra = [int(level)] if level is not None else []
        aux = np.zeros(max(n, 1), np.uint32) if flags else None
        if flags:
            extra.append(aux)
        extra += [d_off, d_len]
        if dict_id is not None:
            extra.append(np.array(list(dict_id) or [0], np.uint32))
        res = self._batch(fn_name, base, in_off, in_len, out, *extra)
        res.aux = aux[:n] if flags else None
        return res

    def lz4_encode_hc_shared(self, base, in_off, in_len, dict_off, dict_len, level=9, caps=None):
        """rcx_lz4_encode_hc_shared_batch over a buffer the caller laid out: block i is base[in_off[i] : in_off[i] + in_len[i]] (base: a
        numpy uint8 array) and its matches may reach into base[dict_off[i] : dict_off[i] + dict_len[i]] (at most 65536 bytes, anywhere in
        the buffer; 0: none).  Blocks that name the same range share one table, built once.  The bytes are lz4_encode_hc_hist's for the
        same block with the same dictionary directly in front of it.  dict_off and dict_len None: lz4_encode_hc_blocks' results."""
        if caps is None:
            caps = [max(int(N.lib().rcx_lz4_compression_bound(int(l))), 1) for l in in_len]
        return self._shared("rcx_lz4_encode_hc_shared_batch", base, in_off, in_len, dict_off, dict_len, caps, level)

    def lz4_encode_hc_dict_blocks(self, blobs, dictionary, level=9, caps=None):
        """One LZ4 HC block per blob behind a dictionary (bytes for all blobs, or a list with one entry, bytes or None, per blob; the last
        64 KiB count): equal dictionaries are placed in the input buffer once and their hash chains are built once
        (rcx_lz4_encode_hc_shared_batch).  The blocks decode as lz4_encode_hc_hist_blocks' do."""
        base, off, lens, d_off, d_len, _ = _pack_shared(blobs, dictionary, 65536)
        return self.lz4_encode_hc_shared(base, off, lens, d_off, d_len, level, caps)

    def deflate_encode_shared(self, base, in_off, in_len, dict_off, dict_len, level=6, caps=None):
        """rcx_deflate_encode_shared_batch (levels 2..9) over a buffer the caller laid out, as lz4_encode_hc_shared: dictionaries of at
        most 32768 bytes anywhere in the buffer; the bytes are deflate_encode_hist's for the same block with the same dictionary
        directly in front of it."""
        if caps is None:
            caps = [deflate_bound(int(l)) for l in in_len]
        return self._shared("rcx_deflate_encode_shared_batch", base, in_off, in_len, dict_off, dict_len, caps, level)

    def deflate_encode_dict_blocks(self, blobs, dictionary, level=6, caps=None):
        """One raw DEFLATE stream per blob (levels 2..9) behind a dictionary (bytes for all blobs, or a list with one entry, bytes or
        None, per blob; the last 32 KiB count): equal dictionaries are placed in the input buffer once and their hash chains are built
        once (rcx_deflate_encode_shared_batch).  The streams decode as deflate_encode_hist_blocks' do."""
        base, off, lens, d_off, d_len, _ = _pack_shared(blobs, dictionary, 32768)
        return self.deflate_encode_shared(base, off, lens, d_off, d_len, level, caps)

    def lz4_decode_shared(self, base, in_off, in_len, dict_off, dict_len, caps):
        """rcx_lz4_decode_shared_batch over a buffer the caller laid out: block i is base[in_off[i] : in_off[i] + in_len[i]] (base: a
        numpy uint8 array) and its matches may reach into base[dict_off[i] : dict_off[i] + dict_len[i]] (at most 65536 bytes, anywhere in
        the buffer; 0: none).  The results are those of a decode with the dictionary directly in front of the slot
        (rcx_lz4_decode_linked_batch with dict_len).  dict_off and dict_len None: lz4_decode_blocks' results."""
        return self._shared("rcx_lz4_decode_shared_batch", base, in_off, in_len, dict_off, dict_len, caps)

    def lz4_decode_dict_blocks(self, blobs, dictionary, caps):
        """One LZ4 block per blob, decoded behind a dictionary (bytes for all blobs, or a list with one entry, bytes or None, per blob; the
        last 64 KiB count): equal dictionaries are placed in the input buffer once, none in front of the slots
        (rcx_lz4_decode_shared_batch).  What lz4_encode_hc_dict_blocks and lz4_encode_hc_hist_blocks write."""
        base, off, lens, d_off, d_len, _ = _pack_shared(blobs, dictionary, 65536)
        return self.lz4_decode_shared(base, off, lens, d_off, d_len, caps)

    def inflate_shared(self, base, in_off, in_len, dict_off, dict_len, caps):
        """rcx_inflate_shared_batch over a buffer the caller laid out, as lz4_decode_shared: dictionaries of at most 32768 bytes anywhere
        in the buffer; the results (aux: the flags) are inflate_hist_blocks' for the same dictionary directly in front of the slot."""
        return self._shared("rcx_inflate_shared_batch", base, in_off, in_len, dict_off, dict_len, caps, flags=True)

    def inflate_dict_blocks(self, blobs, dictionary, caps):
        """One raw DEFLATE stream per blob, decoded behind a dictionary (bytes for all blobs, or a list with one entry, bytes or None,
        per blob; the last 32 KiB count): equal dictionaries are placed in the input buffer once (rcx_inflate_shared_batch)."""
        base, off, lens, d_off, d_len, _ = _pack_shared(blobs, dictionary, 32768)
        return self.inflate_shared(base, off, lens, d_off, d_len, caps)

    def train_dictionaries(self, corpora, sizes, k=256, d=8, f=20):
        """One raw-content dictionary per corpus (rcx_dict_train_batch): corpora is a list of lists of samples (bytes), sizes the
        dictionaries' capacities.  For every corpus the segments of k bytes that cover the most frequent d-byte substrings (d = 6 or 8,
        hashed into 2^f counters) are selected, the most valuable last; a dictionary may come out shorter than its capacity, or empty
        for a corpus shorter than k.  -> list of bytes, to be handed as they are to lz4_encode_hc_dict_blocks,
        deflate_encode_dict_blocks, zlib_encode(..., zdict=, shared=True) and their decoders."""
        n = len(corpora)
        if len(sizes) != n:
            raise ValueError("sizes: one entry per corpus")
        base, off, lens = B.pack([b"".join(bytes(s) for s in c) for c in corpora])
        nsamples = np.array([len(c) for c in corpora] or [0], np.uint32)
        sample_len = np.array([len(s) for c in corpora for s in c] or [0], np.uint64)
        res = self._batch("rcx_dict_train_batch", base, off, lens, _slots([int(x) for x in sizes]), nsamples, sample_len, int(k), int(d), int(f))
        return res.check().outputs

    def train_dictionary(self, samples, size, k=256, d=8, f=20):
        """train_dictionaries for one corpus -> bytes"""
        return self.train_dictionaries([samples], [size], k, d, f)[0]

    def inflate(self, blobs, caps):
        return self._run_host("rcx_inflate_batch", blobs, caps, extra_out=True)

    def zlib_decode(self, blobs, caps, zdict=None, shared=False):
        """One zlib stream per blob.  zdict (bytes for all blobs, or a list with one entry, bytes or None, per blob): the preset
        dictionary of streams that carry FDICT (rcx_zlib_decode_dict_batch): its last 32 KiB are placed in front of every slot and its
        Adler-32 must be the stream's DICTID.  None: rcx_zlib_decode_batch, which refuses FDICT.  shared=True: the same results from
        rcx_zlib_decode_shared_batch -- equal dictionaries lie in the input buffer once and nothing lies in front of the slots."""
        if zdict is None:
            return self._run_host("rcx_zlib_decode_batch", blobs, caps, extra_out=True)
        if shared:
            base, off, lens, d_off, d_len, dicts = _pack_shared(blobs, zdict, 32768)
            return self._shared("rcx_zlib_decode_shared_batch", base, off, lens, d_off, d_len, caps, flags=True,
                                dict_id=[_adler32(d) for d in dicts])
        dicts = _per_blob(zdict, len(blobs))
        return self._inflate_hist(blobs, dicts, caps, [_adler32(d) for d in dicts])

    def inflate_hist_blocks(self, blobs, histories, caps):
        """One raw DEFLATE stream per blob, decoded with HISTORY (rcx_inflate_hist_batch): histories[i] (bytes or None; its last
        32 KiB count) is put directly in front of blob i's slot in the output buffer and the stream's matches may reach into it."""
        if len(histories) != len(blobs):
            raise ValueError("histories: one entry (bytes or None) per blob")
        return self._inflate_hist(blobs, histories, caps, None)

    def _inflate_hist(self, blobs, histories, caps, dict_id):
        n = len(blobs)
        base, off, lens = B.pack(blobs)
        hists = [bytes(h)[-32768:] if h else b"" for h in histories]
        ooff, at = np.zeros(max(n, 1), np.uint64), 0
        for i in range(n):                                       # history, slot (16-byte aligned, as B.layout's), history, slot, ...
            at = (at + len(hists[i]) + 15) & ~15
            ooff[i] = at
            at += int(caps[i])
        out = np.zeros(at + 16, dtype=np.uint8)
        for i, h in enumerate(hists):
            if h:
                out[int(ooff[i]) - len(h):int(ooff[i])] = np.frombuffer(h, np.uint8)
        ocap = np.array(list(caps) or [0], np.uint64)
        hl = np.array([len(h) for h in hists] or [0], np.uint64)
        flags = np.zeros(max(n, 1), np.uint32)
        if dict_id is None:
            res = self._batch("rcx_inflate_hist_batch", base, off, lens, (out, ooff, ocap), flags, hl)
        else:
            res = self._batch("rcx_zlib_decode_dict_batch", base, off, lens, (out, ooff, ocap), flags, hl, np.array(list(dict_id) or [0], np.uint32))
        res.aux = flags[:n]
        return res

    def adler32(self, blobs):
        return self._run_host("rcx_adler32_batch", blobs, None, extra_out=True, needs_out=False)

    def crc32(self, blobs):
        """CRC-32 as in the gzip trailer (extension beyond the reference)."""
        return self._run_host("rcx_crc32_batch", blobs, None, extra_out=True, needs_out=False)

    def gzip_decode(self, blobs, caps):
        """One gzip member (RFC 1952) per blob: header, DEFLATE, CRC32 + ISIZE (extension)."""
        return self._run_host("rcx_gzip_decode_batch", blobs, caps, extra_out=True)

    def bzip2_decode(self, blobs, caps):
        """One whole .bz2 file per blob (rcx_bzip2_decode_batch; extension): one or more concatenated streams, optionally followed by
        other bytes.  status RCX_OK: outputs[i] the decoded bytes, in_used[i] the byte just after the last stream.  A cap too small
        gives E_OUTPUT_TOO_SMALL and out_len[i] = the exact size (caps of 0: a size query); any other failure the first one in stream
        order (E_BZ2_*, E_EOF) with out_len 0.  bzip2.decode_many does the two calls."""
        res = self._run_host("rcx_bzip2_decode_batch", blobs, caps)
        res.outputs = [o if st == 0 else b"" for o, st in zip(res.outputs, res.status)]     # (out_len of a slot too small is a size, not bytes)
        return res

    def bzip2_encode(self, blobs, caps, level=9):
        """One whole .bz2 file per blob (rcx_bzip2_encode_batch; extension): one stream at level 1..9.  status RCX_OK: outputs[i] the
        stream.  A cap too small gives E_OUTPUT_TOO_SMALL and out_len[i] = the exact size, at the full cost of encoding; there is no
        bound to ask for: bzip2.encode_many starts at n + n / 64 + 1024 and retries."""
        res = self._run_host("rcx_bzip2_encode_batch", blobs, caps, scalar=int(level))
        res.outputs = [o if st == 0 else b"" for o, st in zip(res.outputs, res.status)]
        return res

    def zstd_decode(self, blobs, caps, dictionary=None):
        """One whole .zst file per blob (rcx_zstd_decode_batch; extension): one or more concatenated frames, skippable frames skipped,
        optionally followed by other bytes.  dictionary (bytes for all blobs, or a list with one entry, bytes or None, per blob): raw
        content, history in front of every frame; equal dictionaries lie in the input buffer once.  status RCX_OK: outputs[i] the
        decoded bytes, in_used[i] the byte just after the last frame.  A cap too small gives E_OUTPUT_TOO_SMALL and out_len[i] = the
        exact size (caps of 0: a size query); any other failure the first one in stream order (E_ZSTD_*, E_EOF) with out_len 0.
        zstd.decode_many does the two calls."""
        if dictionary is None:
            base, off, lens = B.pack(blobs)
            d_off = d_len = None
        else:
            base, off, lens, d_off, d_len, _ = _pack_shared(blobs, dictionary, 1 << 32)
        res = self._shared("rcx_zstd_decode_batch", base, off, lens, d_off, d_len, caps)
        res.outputs = [o if st == 0 else b"" for o, st in zip(res.outputs, res.status)]     # (out_len of a slot too small is a size, not bytes)
        return res

    def xxh64(self, blobs, seed=0):
        """XXH64 of every blob (rcx_xxh64_batch; extension) -> a uint64 array.  A Zstandard frame's content checksum is the low 32 bits."""
        n = len(blobs)
        base, off, lens = B.pack(blobs)
        hashes = np.zeros(max(n, 1), np.uint64)
        self._batch("rcx_xxh64_batch", base, off, lens, None, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), hashes)
        return hashes[:n]

    def _deflate_encode(self, fn, blobs, caps, framing, level):
        caps = caps if caps is not None else [deflate_bound(len(b)) + framing for b in blobs]
        if level == 1:
            return self._run_host(fn + "_batch", blobs, caps)
        return self._run_host(fn + "_level_batch", blobs, caps, scalar=int(level))

    def deflate_encode(self, blobs, caps=None, level=1):
        """One raw DEFLATE stream (RFC 1951) per blob (extension: the reference has no DEFLATE encoder).  caps default to
        rcx_deflate_compression_bound.  level 1..9 (rcx_deflate_encode_level_batch; 1 is the default encoder's bytes)."""
        return self._deflate_encode("rcx_deflate_encode", blobs, caps, 0, level)

    def zlib_encode(self, blobs, caps=None, level=1, zdict=None, shared=False):
        """One zlib stream (RFC 1950: 78 01 at level 1, DEFLATE, Adler-32) per blob; caps default to the DEFLATE bound + 6.
        zdict (bytes for all blobs, or a list with one entry, bytes or None, per blob; levels 2..9): a preset dictionary as Python's
        zlib takes it (rcx_zlib_encode_dict_batch) -- its last 32 KiB are placed in front of every block, the stream carries FDICT and
        DICTID = zlib.adler32(zdict), and caps default to the bound + 10.  shared=True: the same streams from
        rcx_zlib_encode_shared_batch -- equal dictionaries lie in the input buffer once and their hash chains are built once."""
        if zdict is None:
            return self._deflate_encode("rcx_zlib_encode", blobs, caps, 6, level)
        if shared:
            base, off, lens, d_off, d_len, dicts = _pack_shared(blobs, zdict, 32768)
            if caps is None:
                caps = [deflate_bound(n) + 10 for n in lens]
            return self._shared("rcx_zlib_encode_shared_batch", base, off, lens, d_off, d_len, caps, level, dict_id=[_adler32(d) for d in dicts])
        dicts = _per_blob(zdict, len(blobs))
        base, off, hl = _pack_hist(blobs, dicts, 32768)
        return self._deflate_hist(base, off, [len(b) for b in blobs], hl, level, caps, [_adler32(d) for d in dicts])

    def deflate_encode_hist(self, base, in_off, in_len, hist_len, level=6, caps=None):
        """rcx_deflate_encode_hist_batch (levels 2..9) over a buffer the caller laid out: block i is base[in_off[i] : in_off[i] +
        in_len[i]] (base: a numpy uint8 array) and its matches may reach into the hist_len[i] (at most 32768) bytes below in_off[i]
        -- a dictionary put there, or the bytes before a chunk of one long input.  hist_len None: no history."""
        return self._deflate_hist(base, in_off, in_len, hist_len, level, caps, None)

    def deflate_encode_hist_blocks(self, blobs, histories, level=6, caps=None):
        """One raw DEFLATE stream per blob (levels 2..9), with HISTORY: histories[i] (bytes or None; its last 32 KiB count) is put
        directly in front of blobs[i] in the input buffer and the block's matches may reach into it.  The stream decodes behind the
        same bytes (inflate_hist_blocks, or zlib.decompressobj(-15, zdict=...))."""
        if len(histories) != len(blobs):
            raise ValueError("histories: one entry (bytes or None) per blob")
        base, off, hl = _pack_hist(blobs, histories, 32768)
        return self.deflate_encode_hist(base, off, [len(b) for b in blobs], hl, level, caps)

    def _deflate_hist(self, base, in_off, in_len, hist_len, level, caps, dict_id):
        if caps is None:
            caps = [deflate_bound(int(l)) + (10 if dict_id is not None else 0) for l in in_len]
        return self._encode_hist("rcx_deflate_encode_hist_batch" if dict_id is None else "rcx_zlib_encode_dict_batch", base, in_off, in_len, hist_len,
                                 level, caps, dict_id)

    def gzip_encode(self, blobs, caps=None, level=1):
        """One gzip member (RFC 1952, no optional header fields, MTIME 0, OS 255) per blob; caps default to the DEFLATE bound + 18."""
        return self._deflate_encode("rcx_gzip_encode", blobs, caps, 18, level)

    def bwt_forward(self, blobs):
        return self._run_host("rcx_bwt_forward_batch", blobs, [len(b) for b in blobs], extra_out=True)

    def bwt_suffixes(self, blobs):
        """compute_suffixes (src/bwt/mod.rs:136-166): outputs[i] = the block's suffix array, n little-endian u32; extra[i] = origin."""
        return self._run_host("rcx_bwt_suffixes_batch", blobs, [4 * len(b) for b in blobs], extra_out=True)

    def bwt_inversion_table(self, blobs, origins):
        """compute_inversion_table (src/bwt/mod.rs:223-239) of L = blobs[i] with origins[i]: n little-endian u32 entries."""
        return self._run_host("rcx_bwt_inversion_table_batch", blobs, [4 * len(b) for b in blobs], extra_in=origins)

    def bwt_inverse(self, blobs, origins):
        return self._run_host("rcx_bwt_inverse_batch", blobs, [len(b) for b in blobs], extra_in=origins)

    def bwt_inverse_minimal(self, blobs, origins):
        """The reference's decode_minimal (src/bwt/mod.rs:298-315), reproduced as it computes -- not the inverse of bwt_forward in general."""
        return self._run_host("rcx_bwt_inverse_minimal_batch", blobs, [len(b) for b in blobs], extra_in=origins)

    def mtf_encode(self, blobs):
        return self._run_host("rcx_mtf_encode_batch", blobs, [len(b) for b in blobs])

    def mtf_decode(self, blobs):
        return self._run_host("rcx_mtf_decode_batch", blobs, [len(b) for b in blobs])

    def dc_encode(self, blobs):
        return self._run_host("rcx_dc_encode_batch", blobs, [4 * (256 + len(b)) for b in blobs])

    def dc_decode(self, blobs, n_out):
        return self._run_host("rcx_dc_decode_batch", blobs, list(n_out), n_out=n_out)

    def dc_encode_ctx(self, blobs):
        """-> result whose outputs[i] = the words (first 4 * (256 + k) bytes), a gap, then k 8-byte contexts from byte
        4 * (256 + n) on (include/rcx.h); `dc_split_ctx` cuts it up"""
        return self._run_host("rcx_dc_encode_ctx_batch", blobs, [4 * (256 + len(b)) + 8 * len(b) for b in blobs])

    def dc_decode_ctx(self, blobs, n_out):
        return self._run_host("rcx_dc_decode_ctx_batch", blobs, [((n + 7) & ~7) + 8 * max(0, len(b) // 4 - 256) for b, n in zip(blobs, n_out)], n_out=n_out)

    def ari_byte_encode(self, blobs):
        return self._run_host("rcx_ari_byte_encode_batch", blobs, [int(N.lib().rcx_ari_byte_encode_bound(len(b))) for b in blobs])

    def ari_byte_decode(self, blobs, caps):
        return self._run_host("rcx_ari_byte_decode_batch", blobs, caps)

    def ari_binary_encode(self, blobs, rate):
        """bin::Model, 8 decisions per byte (src/entropy/ari/test.rs:22-50)."""
        return self._run_host("rcx_ari_binary_encode_batch", blobs, [int(N.lib().rcx_ari_byte_encode_bound(len(b))) for b in blobs], scalar=rate)

    def ari_binary_decode(self, blobs, rate, nbytes):
        """nbytes[i] = bytes to decode from stream i (the coding has no end marker)."""
        return self._run_host("rcx_ari_binary_decode_batch", blobs, list(nbytes), scalar=rate)

    def ari_proxy_encode(self, blobs):
        """table::SumProxy + bin::SumProxy (src/entropy/ari/test.rs:91-148)."""
        return self._run_host("rcx_ari_proxy_encode_batch", blobs, [int(N.lib().rcx_ari_byte_encode_bound(len(b))) for b in blobs])

    def ari_proxy_decode(self, blobs, nbytes):
        return self._run_host("rcx_ari_proxy_decode_batch", blobs, list(nbytes))

    def ari_apm_encode(self, blobs):
        """apm::Bit through apm::Gate (src/entropy/ari/test.rs:150-182); status E_MALFORMED = the reference panics on this input."""
        return self._run_host("rcx_ari_apm_encode_batch", blobs, [int(N.lib().rcx_ari_byte_encode_bound(len(b))) for b in blobs])

    def ari_apm_decode(self, blobs, nbytes):
        return self._run_host("rcx_ari_apm_decode_batch", blobs, list(nbytes))

    def rle_encode(self, blobs):
        return self._run_host("rcx_rle_encode_batch", blobs, [int(N.lib().rcx_rle_encode_bound(len(b))) for b in blobs])

    def rle_decode(self, blobs, caps):
        return self._run_host("rcx_rle_decode_batch", blobs, caps)

    # ---------------- device-resident batches (torch tensors) ----------------
    def launch_dev(self, codec, db, scratch=None):
        """db: DeviceBatch. Enqueues on the ctx stream and returns (no sync)."""
        sp = scratch.data_ptr() if scratch is not None else None
        sb = scratch.numel() if scratch is not None else 0
        self._chk(N.lib().rcx_launch_dev(self._h, codec, C.byref(db.c), C.c_void_p(sp), sb))

    def scratch_bytes(self, codec, nblocks, max_block):
        return int(N.lib().rcx_scratch_bytes(codec, nblocks, max_block))


class DeviceBatch:
    """Struct-of-arrays batch whose every array is a torch tensor in HBM."""

    def __init__(self, in_base, in_off, in_len, out_base, out_off, out_cap, aux=None):
        import torch
        dev = in_base.device
        n = in_off.numel()
        self.n = n
        self.in_base, self.in_off, self.in_len = in_base, in_off, in_len
        self.out_base, self.out_off, self.out_cap = out_base, out_off, out_cap
        self.out_len = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        self.in_used = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        self.status = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        self.aux = aux if aux is not None else torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.c = N.DevBatch(in_base.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), out_base.data_ptr(),
                            out_off.data_ptr(), out_cap.data_ptr(), self.out_len.data_ptr(), self.in_used.data_ptr(),
                            self.status.data_ptr(), self.aux.data_ptr(), n)

    def sub(self, lo, hi):
        """Blocks [lo, hi) of this batch as a batch of its own: the same tensors, sliced (results land in this batch's arrays)."""
        v = object.__new__(DeviceBatch)
        v.n = hi - lo
        v.in_base, v.out_base = self.in_base, self.out_base
        for name in ("in_off", "in_len", "out_off", "out_cap", "out_len", "in_used", "status", "aux"):
            setattr(v, name, getattr(self, name)[lo:hi])
        v.c = N.DevBatch(v.in_base.data_ptr(), v.in_off.data_ptr(), v.in_len.data_ptr(), v.out_base.data_ptr(),
                         v.out_off.data_ptr(), v.out_cap.data_ptr(), v.out_len.data_ptr(), v.in_used.data_ptr(),
                         v.status.data_ptr(), v.aux.data_ptr(), v.n)
        return v

    @staticmethod
    def from_host(blobs_base, off, lens, out_total, out_off, out_cap, device):
        import torch
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(device)
        return DeviceBatch(t(blobs_base, np.uint8), t(off.astype(np.uint64), np.int64), t(lens.astype(np.uint64), np.int64),
                           torch.zeros(out_total + 64, dtype=torch.uint8, device=device),
                           t(out_off.astype(np.uint64), np.int64), t(out_cap.astype(np.uint64), np.int64))
