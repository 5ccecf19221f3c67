"""CPU suite: every codec kernel the wave simulator builds, held to the batch contract of include/rcx.h on layouts the other tests never
produce (tests/layout_cases.py): blocks and slots back to back, at every residue mod 16, in shuffled order, with poison in every byte that
is not a block's input.  Per call, layout and kernel variant: every block's status, out_len, in_used, aux and bytes are the oracle's for
that block alone, the same for both poison bytes; no byte outside the slots changes; the input buffer is untouched."""
import numpy as np
import pytest

import layout_cases as LC
from rust_compress_amd import _native as N

_CASES = {}
CALLS = {
    "mtf_encode": lambda o, r: LC.mtf(o, r, False), "mtf_decode": lambda o, r: LC.mtf(o, r, True),
    "rle_encode": lambda o, r: LC.rle(o, r, False), "rle_decode": lambda o, r: LC.rle(o, r, True),
    "dc_encode": lambda o, r: LC.dc_encode(o, r, False), "dc_encode_ctx": lambda o, r: LC.dc_encode(o, r, True),
    "dc_decode": lambda o, r: LC.dc_decode(o, r, False), "dc_decode_ctx": lambda o, r: LC.dc_decode(o, r, True),
    "ari_byte_encode": lambda o, r: LC.ari(o, r, "byte", False), "ari_byte_decode": lambda o, r: LC.ari(o, r, "byte", True),
    "ari_binary_encode": lambda o, r: LC.ari(o, r, "binary", False), "ari_binary_decode": lambda o, r: LC.ari(o, r, "binary", True),
    "ari_proxy_encode": lambda o, r: LC.ari(o, r, "proxy", False), "ari_proxy_decode": lambda o, r: LC.ari(o, r, "proxy", True),
    "ari_apm_encode": lambda o, r: LC.ari(o, r, "apm", False), "ari_apm_decode": lambda o, r: LC.ari(o, r, "apm", True),
    "bwt_forward": lambda o, r: LC.bwt(o, r, "forward"), "bwt_suffixes": lambda o, r: LC.bwt(o, r, "suffixes"),
    "bwt_inversion_table": lambda o, r: LC.bwt(o, r, "table"), "bwt_inverse": lambda o, r: LC.bwt(o, r, "inverse"),
    "bwt_inverse_minimal": lambda o, r: LC.bwt(o, r, "minimal"),
    "lz4_encode": lambda o, r: LC.lz4(o, r, False), "lz4_decode": lambda o, r: LC.lz4(o, r, True),
    "adler32": lambda o, r: LC.checksum(o, r, "adler32"), "crc32": lambda o, r: LC.checksum(o, r, "crc32"),
    "inflate": lambda o, r: LC.inflate_family(o, r, "inflate", 2), "zlib": lambda o, r: LC.inflate_family(o, r, "zlib", 2),
    "gzip": lambda o, r: LC.inflate_family(o, r, "gzip", 2),
}


def case(oracle, call):
    if "raws" not in _CASES:
        _CASES["raws"] = LC.block_set(oracle)
    if call not in _CASES:
        _CASES[call] = CALLS[call](oracle, _CASES["raws"])
    return _CASES[call]


def runs_of(c, oracle):
    """-> [(label, simulator variant, scratch bytes, scratch contents)]: the variants the codec's existing simulator test pins"""
    n, total, maxn = c.n, sum(len(b) for b in c.blocks), max(len(b) for b in c.blocks)
    if c.codec in (N.MTF_ENCODE, N.MTF_DECODE, N.RLE_ENCODE, N.RLE_DECODE, N.ARI_PROXY_ENCODE, N.ARI_PROXY_DECODE, N.BWT_INVERSION_TABLE,
                   N.ADLER32, N.CRC32):
        return [("v0", 0, 0, None)]
    if c.codec == N.DC_ENCODE:                                 # the simulator takes the contexts' switch as the variant; scratch: k_dcx_prep / k_dcx_main
        return [("ctx", 1, 0, None)] if c.param else [("wave", 0, 0, None), ("chunks", 0, n * 37632 + 256, None)]
    if c.codec == N.DC_DECODE:
        return [("ctx" if c.param else "plain", c.param, 0, None)]
    if c.codec in (N.ARI_BYTE_ENCODE, N.ARI_BYTE_DECODE):
        return [("lane", 1, 0, None), ("wave", 2, 0, None), ("quad", 3, 0, None)]
    if c.codec in (N.ARI_BINARY_ENCODE, N.ARI_BINARY_DECODE):
        return [("rate%d" % c.param, c.param, 0, None)]       # (the rate rides in the variant)
    if c.codec in (N.ARI_APM_ENCODE, N.ARI_APM_DECODE):
        stretch, gate = oracle.apm_tables()
        return [("v0", 0, 0, stretch.tobytes() + gate.tobytes())]
    if c.codec in (N.BWT_FORWARD, N.BWT_SUFFIXES):
        return [("v0", 0, 64 * total + (8 << 20), None)]
    if c.codec == N.BWT_INVERSE:
        return [("v%x" % v, v, n * (24 * maxn + (4 << 20)) + 256, None) for v in (0, 1, 2, 3, 4, 5, 0x10, 0x41, 0x60)]
    if c.codec == N.BWT_INVERSE_MINIMAL:
        return [("v%d" % v, v, n * (24 * maxn + (4 << 20)) + 256, None) for v in (0, 1)]
    if c.codec == N.LZ4_ENCODE:
        return [("v%d" % v, v, n * (1 << 19), None) for v in (0, 2, 1)]
    if c.codec == N.LZ4_DECODE:
        return [("v%d" % v, v, 0, None) for v in (0, 15)]
    if c.codec == N.ZLIB_DECODE:
        return [("v%d" % v, v, 13 * (n + 1) + 512, None) for v in (0, 11, 9, 2, 3, 4, 1)]
    if c.codec == N.INFLATE:
        return [("v0", 0, 13 * (n + 1) + 512, None)]
    assert c.codec == N.GZIP_DECODE
    return [("v0", 0, 48 * n + 256, None)]


@pytest.mark.parametrize("layout", ("packed", "residues", "shuffled"))
@pytest.mark.parametrize("call", sorted(CALLS))
def test_layout(oracle, call, layout):
    import simrun
    c = case(oracle, call)
    name = LC.layout_names(c.out_align)[("packed", "residues", "shuffled").index(layout)]      # (aligned4 / aligned8 stand in for residues)
    lays = {p: LC.build(name, c.blocks, c.caps, p, c.out_align, c.in_align) for p in LC.POISONS}
    for label, variant, sb, init in runs_of(c, oracle):
        gots = []
        for p, lay in lays.items():
            out, out_len, in_used, status, aux, inb = simrun.run_layout(c.codec, variant, lay, aux=c.aux_in, n_out=c.n_out, scratch_bytes=sb, scratch_init=init)
            got = LC.Got(out, out_len, in_used, status, aux if c.aux_out else None, inb)
            LC.check_all(lay, got, c.wants, tag=(call, label))
            gots.append((lay, got))
        LC.check_same(gots[0][0], gots[0][1], gots[1][0], gots[1][1], c.wants, tag=(call, label))


@pytest.mark.parametrize("call", ("dc_encode", "dc_encode_ctx", "dc_decode"))
def test_dc_words_at_odd_addresses_are_refused_by_the_kernels(oracle, call):
    """The DC kernels read and write their words through uint32_t pointers (include/rcx.h asks for 4-byte alignment): a word buffer at
    any other residue costs exactly that block -- RCX_E_OUTPUT_TOO_SMALL from the encoders, RCX_E_MALFORMED from the decoder, out_len 0,
    not a byte written -- and the blocks whose residue happens to be a multiple of 4 are coded as ever."""
    import simrun
    c = case(oracle, call)
    for p in LC.POISONS:
        lay = LC.build("residues", c.blocks, c.caps, p)       # slots and inputs at every residue mod 16
        out, out_len, in_used, status, aux, inb = simrun.run_layout(c.codec, c.param, lay, aux=c.aux_in, n_out=c.n_out)
        got = LC.Got(out, out_len, in_used, status, None, inb)
        words_at = lay.in_off if c.codec == N.DC_DECODE else lay.out_off
        odd = [int(o) % 4 != 0 for o in words_at]
        assert sum(odd) >= 20 and sum(not x for x in odd) >= 8
        refused = LC.Want(N.E_MALFORMED) if c.codec == N.DC_DECODE else LC.Want(N.E_OUTPUT_TOO_SMALL, out_len=0)
        wants = [refused if o else w for o, w in zip(odd, c.wants)]
        LC.check_all(lay, got, wants, tag=call)
        for i, o in enumerate(odd):
            if o:
                a = int(lay.out_off[i])
                assert (out[a: a + int(lay.out_cap[i])] == p).all(), (call, i, "a refused block's slot was written")
