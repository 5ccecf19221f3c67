"""A small writer for the Zstandard frames libzstd never writes: the frames tests/zstd_cases.py names as `must decode` and `must be
refused`.  No match finder and no FSE encoder: sequences are written with all three tables in RLE mode, where a state takes no bits and
a sequence is its extra bits alone; literals are raw or RLE; the table descriptions that must fail are written bit by bit.

A literal `distribution that oversums` cannot be written: a count is coded in a range that ends at what is left (RFC 8878 4.1.1), so
the decoder never sees a sum beyond the table.  What can go wrong with a distribution is written instead: a zero run that passes the
last symbol, and symbols that run out before the sum is reached."""
import struct

from zstd_ref import MAGIC, xxh64


def frame(blocks, fcs=None, fcs_bytes=None, single=False, window=0x50, checksum=None, dict_id=0, reserved=False, raw=b"", bad_checksum=False):
    """blocks: a list of block() results, the last one marked last by the caller.  fcs: the declared size (None: none, needs a window),
    fcs_bytes its field's width (default: the smallest).  raw: the decoded bytes, for the checksum.  checksum: True appends XXH64(raw)."""
    fhd = 0
    body = b""
    if fcs is not None and fcs_bytes is None:
        fcs_bytes = 1 if fcs < 256 and single else 2 if 256 <= fcs < 65536 + 256 else 4 if fcs < (1 << 32) else 8
        if fcs_bytes == 1 and not single:
            fcs_bytes = 4
    if fcs is not None:
        fhd |= {1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6
        assert fcs_bytes != 1 or single
    if single:
        fhd |= 0x20
    else:
        body += bytes([window])
    if reserved:
        fhd |= 8
    if checksum:
        fhd |= 4
    if dict_id:
        fhd |= 1
        body += bytes([dict_id])
    if fcs is not None:
        body += (fcs - 256 if fcs_bytes == 2 else fcs).to_bytes(fcs_bytes, "little")
    out = struct.pack("<I", MAGIC) + bytes([fhd]) + body + b"".join(blocks)
    if checksum:
        out += struct.pack("<I", (xxh64(raw) & 0xFFFFFFFF) ^ (1 if bad_checksum else 0))
    return out


def block(kind, payload, last=False, size=None):
    """kind 0 raw, 1 RLE (payload: one byte, size: the count), 2 compressed, 3 reserved"""
    size = len(payload) if size is None else size
    return (size << 3 | kind << 1 | (1 if last else 0)).to_bytes(3, "little") + payload


def skippable(payload, nibble=0):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + payload


def backward(fields):
    """fields: (value, bits) in the order they are read -> the bitstream's bytes, end mark included"""
    v = 1
    for val, n in fields:
        assert 0 <= val < (1 << n) or n == 0
        v = (v << n) | val
    return v.to_bytes((v.bit_length() + 7) // 8, "little")


def forward(fields):
    v, at = 0, 0
    for val, n in fields:
        v |= val << at
        at += n
    return v.to_bytes((at + 7) // 8, "little")


def literals(kind, data, size=None):
    """kind 0: raw bytes; kind 1: RLE of data[0], `size` times"""
    size = len(data) if size is None else size
    if size < 32:
        hdr = bytes([kind | size << 3])
    elif size < 4096:
        hdr = (kind | 1 << 2 | size << 4).to_bytes(2, "little")
    else:
        hdr = (kind | 3 << 2 | size << 4).to_bytes(3, "little")
    return hdr + (data if kind == 0 else data[:1])


def nseq_bytes(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([128 + (n >> 8), n & 255])
    return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")


LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def rle_sequences(ll_code, of_code, ml_code, extras, left_over=0, repeat=False):
    """the sequences section with all three tables in RLE mode: extras is one (offset bits, match length bits, literal length bits) per
    sequence; left_over: that many zero bits nobody reads; repeat: the three tables in repeat mode instead, for a block behind one
    that set these codes"""
    fields = []
    for ov, mv, lv in extras:
        fields += [(ov, of_code), (mv, ML_BITS[ml_code]), (lv, LL_BITS[ll_code])]
    if left_over:
        fields.append((0, left_over))
    return nseq_bytes(len(extras)) + (b"\xfc" if repeat else bytes([0x54, ll_code, of_code, ml_code])) + backward(fields)


def compressed(lits, seqs=b"\x00", last=False):
    return block(2, lits + seqs, last)


def huffman_literals_header(kind, size, body, streams=1):
    """3-byte header of compressed (2) or treeless (3) literals, sizes below 1024"""
    assert size < 1024 and len(body) < 1024
    return (kind | (0 if streams == 1 else 1) << 2 | size << 4 | len(body) << 14).to_bytes(3, "little") + body
