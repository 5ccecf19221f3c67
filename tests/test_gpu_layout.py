"""GPU: every classic rcx_*_batch entry point held to the batch contract of include/rcx.h on layouts Context._run_host never produces
(tests/layout_cases.py): blocks and slots back to back, at every residue mod 16, in shuffled order, with poison (0xA5, then 0x5A) in
every byte that is not a block's input -- from pageable host memory, from page-locked host memory (the decoders that store into the
caller's buffer themselves) and from device memory.  Per call, layout, memory kind and kernel variant: every block's status, out_len,
in_used, aux and bytes are the oracle's for that block alone and the same for both poisons; no byte of the output buffer outside the
slots changes (from host memory the copy back is held to that too); the input buffer is untouched."""
import ctypes as C

import numpy as np
import pytest

import layout_cases as LC
from rust_compress_amd import _native as N

pytestmark = pytest.mark.gpu

LAYOUTS = ("packed", "residues", "shuffled")
_CASES = {}


def case(oracle, call, build):
    if "raws" not in _CASES:
        _CASES["raws"] = LC.block_set(oracle)
    if call not in _CASES:
        _CASES[call] = build(oracle, _CASES["raws"])
    return _CASES[call]


def _entry(c):
    """-> (entry point, the arguments behind the batch as a function of (aux array pointer, n_out pointer))"""
    L = N.lib()
    simple = {N.MTF_ENCODE: "rcx_mtf_encode_batch", N.MTF_DECODE: "rcx_mtf_decode_batch", N.RLE_ENCODE: "rcx_rle_encode_batch",
              N.RLE_DECODE: "rcx_rle_decode_batch", N.ARI_BYTE_ENCODE: "rcx_ari_byte_encode_batch", N.ARI_BYTE_DECODE: "rcx_ari_byte_decode_batch",
              N.ARI_PROXY_ENCODE: "rcx_ari_proxy_encode_batch", N.ARI_PROXY_DECODE: "rcx_ari_proxy_decode_batch",
              N.ARI_APM_ENCODE: "rcx_ari_apm_encode_batch", N.ARI_APM_DECODE: "rcx_ari_apm_decode_batch",
              N.LZ4_ENCODE: "rcx_lz4_encode_batch", N.LZ4_DECODE: "rcx_lz4_decode_batch"}
    with_aux = {N.BWT_FORWARD: "rcx_bwt_forward_batch", N.BWT_SUFFIXES: "rcx_bwt_suffixes_batch", N.BWT_INVERSION_TABLE: "rcx_bwt_inversion_table_batch",
                N.BWT_INVERSE: "rcx_bwt_inverse_batch", N.BWT_INVERSE_MINIMAL: "rcx_bwt_inverse_minimal_batch", N.ADLER32: "rcx_adler32_batch",
                N.CRC32: "rcx_crc32_batch", N.INFLATE: "rcx_inflate_batch", N.ZLIB_DECODE: "rcx_zlib_decode_batch", N.GZIP_DECODE: "rcx_gzip_decode_batch"}
    if c.codec in simple:
        return getattr(L, simple[c.codec]), lambda aux, n_out: ()
    if c.codec in with_aux:
        return getattr(L, with_aux[c.codec]), lambda aux, n_out: (C.c_void_p(aux),)
    if c.codec == N.DC_ENCODE:
        return (L.rcx_dc_encode_ctx_batch if c.param else L.rcx_dc_encode_batch), lambda aux, n_out: ()
    if c.codec == N.DC_DECODE:
        return (L.rcx_dc_decode_ctx_batch if c.param else L.rcx_dc_decode_batch), lambda aux, n_out: (C.c_void_p(n_out),)
    if c.codec in (N.ARI_BINARY_ENCODE, N.ARI_BINARY_DECODE):
        return (L.rcx_ari_binary_decode_batch if c.codec == N.ARI_BINARY_DECODE else L.rcx_ari_binary_encode_batch), lambda aux, n_out: (c.param,)
    assert c.name == "xxh32"
    return L.rcx_xxh32_batch, lambda aux, n_out: (c.param, C.c_void_p(aux))


def call_raw(ctx, c, lay, mem, expect_rc=0):
    """One raw batch call on the layout's buffers in memory kind `mem` (host | pinned | device) -> LC.Got (the output copied back with
    torch for device memory); with expect_rc != 0, (the return code, LC.Got of what the refused call left)."""
    import torch
    p = lambda a: a.ctypes.data
    n = lay.n
    if mem == "host":
        inb, out = lay.in_buf.copy(), lay.fresh_out()
        ip, op = p(inb), p(out)
    else:
        ti, to = torch.from_numpy(lay.in_buf.copy()), torch.from_numpy(lay.fresh_out())
        ti, to = (ti.pin_memory(), to.pin_memory()) if mem == "pinned" else (ti.to("cuda:0"), to.to("cuda:0"))
        ip, op = ti.data_ptr(), to.data_ptr()
    off, lens = np.ascontiguousarray(lay.in_off, np.uint64), np.ascontiguousarray(lay.in_len, np.uint64)
    ooff, ocap = np.ascontiguousarray(lay.out_off, np.uint64), np.ascontiguousarray(lay.out_cap, np.uint64)
    out_len, in_used, status = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -9, np.int32)
    aux = c.aux_in.copy() if c.aux_in is not None else np.zeros(n, np.uint32)
    n_out = c.n_out if c.n_out is not None else np.zeros(n, np.uint64)
    b = N.Batch(ip, p(off), p(lens), op, p(ooff), p(ocap), p(out_len), p(in_used), p(status), n, N.MEM_HOST if mem != "device" else N.MEM_DEVICE)
    fn, extra = _entry(c)
    rc = fn(ctx._h, C.byref(b), *extra(p(aux), p(n_out)))
    msg = N.lib().rcx_last_error(ctx._h)
    assert expect_rc != 0 or rc == 0, (c.name, lay.name, mem, rc, msg)
    if mem != "host":
        torch.cuda.synchronize()
        inb, out = ti.cpu().numpy(), to.cpu().numpy()
    got = LC.Got(out, out_len, in_used, status, aux if c.aux_out else None, inb)
    return got if expect_rc == 0 else (rc, got)


def run_case(ctx, c, layout, mem, variants=(0,), variant_codec=None):
    name = LC.layout_names(c.out_align)[LAYOUTS.index(layout)]                  # (aligned4 / aligned8 stand in for residues)
    lays = [LC.build(name, c.blocks, c.caps, p, c.out_align, c.in_align) for p in LC.POISONS]
    vc = c.codec if variant_codec is None else variant_codec
    try:
        for v in variants:
            if variants != (0,):
                ctx.set_variant(vc, v)
            gots = []
            for lay in lays:
                got = call_raw(ctx, c, lay, mem)
                # (include/rcx.h: into a page-locked buffer the default LZ4 decoder writes nothing beyond out_len of a block that decodes)
                LC.check_all(lay, got, c.wants, tag=(c.name, mem, "variant", v), tight=c.codec == N.LZ4_DECODE and mem == "pinned" and v == 0)
                gots.append(got)
            LC.check_same(lays[0], gots[0], lays[1], gots[1], c.wants, tag=(c.name, mem, "variant", v))
    finally:
        if variants != (0,):
            ctx.set_variant(vc, 0)


MEMS = ("host", "device")
MEMS_MIRROR = ("host", "pinned", "device")

MTF_RLE = {"mtf_encode": lambda o, r: LC.mtf(o, r, False), "mtf_decode": lambda o, r: LC.mtf(o, r, True),
           "rle_encode": lambda o, r: LC.rle(o, r, False), "rle_decode": lambda o, r: LC.rle(o, r, True)}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call", sorted(MTF_RLE))
def test_mtf_rle(ctx, oracle, call, layout, mem):
    run_case(ctx, case(oracle, call, MTF_RLE[call]), layout, mem)


DC = {"dc_encode": lambda o, r: LC.dc_encode(o, r, False), "dc_encode_ctx": lambda o, r: LC.dc_encode(o, r, True),
      "dc_decode": lambda o, r: LC.dc_decode(o, r, False), "dc_decode_ctx": lambda o, r: LC.dc_decode(o, r, True)}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call", sorted(DC))
def test_dc(ctx, oracle, call, layout, mem):
    """The word buffers 4-byte aligned (the decoder's context slot 8-byte), as include/rcx.h asks; DC_ENCODE variant 0 (the lane-per-chunk
    kernels take the blocks of 8 KiB over at most 64 symbols) and 1 (the wave-per-block kernel alone)."""
    c = case(oracle, call, DC[call])
    run_case(ctx, c, layout, mem, variants=(0, 1) if call == "dc_encode" else (0,))


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("call", ("dc_encode", "dc_encode_ctx", "dc_decode"))
def test_dc_refuses_a_misaligned_word_buffer(ctx, oracle, call, mem):
    """Word slots and word inputs at every residue mod 16: the batch calls refuse the batch with RCX_RC_BAD_ARG, name the first block
    whose words are not 4-byte aligned, and write nothing."""
    c = case(oracle, call, DC[call])
    lay = LC.build("residues", c.blocks, c.caps, LC.POISONS[0])
    words_at = lay.in_off if c.codec == N.DC_DECODE else lay.out_off
    first = [int(o) % 4 != 0 for o in words_at].index(True)
    # (a torch allocation is at least 256-byte aligned: in device memory the offsets' residues are the addresses')
    rc, got = call_raw(ctx, c, lay, mem, expect_rc=N.RC_BAD_ARG)
    assert rc == N.RC_BAD_ARG
    msg = N.lib().rcx_last_error(ctx._h).decode()
    assert ("block %d:" % first) in msg and "4-byte aligned" in msg, msg
    # nothing was written: both buffers and the result arrays are as they were handed over
    assert (got.out == lay.poison).all() and np.array_equal(got.in_after, lay.in_buf)
    assert (got.status == -9).all() and not got.out_len.any() and not got.in_used.any()


ARI = {"ari_byte_encode": lambda o, r: LC.ari(o, r, "byte", False), "ari_byte_decode": lambda o, r: LC.ari(o, r, "byte", True),
       "ari_binary_encode": lambda o, r: LC.ari(o, r, "binary", False), "ari_binary_decode": lambda o, r: LC.ari(o, r, "binary", True),
       "ari_proxy_encode": lambda o, r: LC.ari(o, r, "proxy", False), "ari_proxy_decode": lambda o, r: LC.ari(o, r, "proxy", True),
       "ari_apm_encode": lambda o, r: LC.ari(o, r, "apm", False), "ari_apm_decode": lambda o, r: LC.ari(o, r, "apm", True)}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call", sorted(ARI))
def test_range_coders(ctx, oracle, call, layout, mem):
    """ARI_BYTE_* variants 1, 2, 3: a lane, a wave and a quad of lanes per stream; the binary model at rate 5."""
    run_case(ctx, case(oracle, call, ARI[call]), layout, mem, variants=(1, 2, 3) if call.startswith("ari_byte") else (0,))


BWT = {"bwt_forward": lambda o, r: LC.bwt(o, r, "forward"), "bwt_suffixes": lambda o, r: LC.bwt(o, r, "suffixes"),
       "bwt_inversion_table": lambda o, r: LC.bwt(o, r, "table"), "bwt_inverse": lambda o, r: LC.bwt(o, r, "inverse"),
       "bwt_inverse_minimal": lambda o, r: LC.bwt(o, r, "minimal")}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call", sorted(BWT))
def test_bwt(ctx, oracle, call, layout, mem):
    """The suffix array's and the inversion table's slots 4-byte aligned, as include/rcx.h asks (aligned4 for residues); BWT_INVERSE
    variants 0, 1, 2, 4 and BWT_INVERSE_MINIMAL 0, 1."""
    variants = {"bwt_inverse": (0, 1, 2, 4), "bwt_inverse_minimal": (0, 1)}.get(call, (0,))
    run_case(ctx, case(oracle, call, BWT[call]), layout, mem, variants=variants)


LZ4 = {"lz4_encode": lambda o, r: LC.lz4(o, r, False), "lz4_decode": lambda o, r: LC.lz4(o, r, True)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call,mem", [("lz4_encode", m) for m in MEMS] + [("lz4_decode", m) for m in MEMS_MIRROR])
def test_lz4(ctx, oracle, call, layout, mem):
    """The greedy encoder; the decoder's default kernel and its fallback (pageable host memory: one span copied back; page-locked: the
    decoder stores into the caller's buffer itself)."""
    run_case(ctx, case(oracle, call, LZ4[call]), layout, mem, variants=(0, N.LZ4_DECODE_VARIANTS[1]) if call == "lz4_decode" else (0,))


SUMS = {"adler32": lambda o, r: LC.checksum(o, r, "adler32"), "crc32": lambda o, r: LC.checksum(o, r, "crc32"),
        "xxh32": lambda o, r: LC.checksum(o, r, "xxh32")}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call", sorted(SUMS))
def test_checksums(ctx, oracle, call, layout, mem):
    """Input side only: the sums of blocks at every residue, back to back and shuffled, whatever lies around them; an output buffer
    handed over all the same is not touched."""
    run_case(ctx, case(oracle, call, SUMS[call]), layout, mem)


INFLATE = {"%s_%dbad" % (f, k): (lambda o, r, f=f, k=k: LC.inflate_family(o, r, f, k)) for f in ("inflate", "zlib", "gzip") for k in (2, 20, 22)}


@pytest.mark.parametrize("mem", MEMS_MIRROR)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call", sorted(INFLATE))
def test_inflate_family(ctx, oracle, call, layout, mem):
    """40 streams of which 2, 20 or 22 are corrupted.  Into a page-locked buffer the streams the first pass hands back -- every corrupted
    one at least -- are copied out one by one when they are few and as one span when they are more than n / 8 + 16 = 21: the 22 take that
    branch for certain, on the `packed` layout, whose slots tile the span; on a layout with gaps the span would carry the staging buffer's
    bytes between the slots, and the streams go one by one however many they are."""
    run_case(ctx, case(oracle, call, INFLATE[call]), layout, mem)


def test_a_later_call_does_not_see_an_earlier_one(ctx, oracle):
    """The staging buffer of a context outlives a call.  A host-memory MTF encode of 0x77-filled blocks leaves 0x77 all over it; a call of
    another codec on the `residues` layout through the same context must still leave every byte outside its slots as the caller had it."""
    fill = [b"\x77" * n for n in (20000, 30000, 4097, 65536)]
    res = ctx.mtf_encode(fill).check()
    assert res.outputs == [oracle.mtf_encode(f) for f in fill]
    res = ctx.lz4_decode_blocks([oracle.lz4_encode_block(f) for f in fill], [len(f) for f in fill]).check()      # (0x77 all over the output staging)
    assert res.outputs == fill
    for call, table in (("rle_encode", MTF_RLE), ("bwt_forward", BWT), ("ari_proxy_decode", ARI)):
        c = case(oracle, call, table[call])
        for p in LC.POISONS:
            lay = LC.build("residues", c.blocks, c.caps, p)
            got = call_raw(ctx, c, lay, "host")
            LC.check_all(lay, got, c.wants, tag=(call, "after 0x77"))
