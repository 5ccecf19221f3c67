"""A DEFLATE assembler and a token model (TEST INFRASTRUCTURE, shared by test_deflate_craft.py, test_wavesim_deflate_craft.py and
test_gpu_deflate_craft.py through deflate_craft_cases.py).  Streams are written bit by bit, with every choice libz never makes left
to the caller: code lengths that are not Huffman-optimal (15-bit codes), the code-length code and HCLEN, the run-length spelling of
the lengths list as an explicit list of (symbol, extra) -- valid or not --, HLIT / HDIST fields that lie, the spelling of a length,
raw symbols without a meaning, a wrong NLEN.  What a stream decodes to comes from the token model alone (Stream.expected), from no
decoder.  Codes are assigned as RFC 1951 section 3.2.2 says."""
from deflate_hist_cases import _Bits as Bits  # noqa: F401  (the LSB-first bit writer; re-exported)

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577)
DEXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8          # 288 symbols: 286 and 287 have codes and no meaning
FIXED_D = [5] * 32                                              # 32 codes of 5 bits: 30 and 31 have no meaning


def canonical(lengths):
    """{symbol: (code, bits)} of the symbols with a length, RFC 1951 3.2.2.  An over-subscribed list still gets codes (they overflow
    their lengths and are cut to them): such a header is refused before a code is read."""
    count = [0] * 17
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def complete_lens(symbols, size):
    """`size` lengths, a complete code over `symbols` (two at least) with lengths k - 1 and k: the first ones get the shorter"""
    symbols = sorted(set(symbols))
    n = len(symbols)
    assert n >= 2
    k = (n - 1).bit_length()
    short = (1 << k) - n
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = k - 1 if i < short else k
    return lens


def length_symbol(length):
    """the usual spelling: (symbol, extra)"""
    assert 3 <= length <= 258
    k = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
    return 257 + k, length - LBASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DBASE[i] <= dist)
    return k, dist - DBASE[k]


# Tokens.  (0, byte): a literal.  (length, distance): a match in its usual spelling.  (length, distance, symbol, extra): a match
# with the length spelt as this symbol and these extra bits (258 as 284 + 31).  ("sym", s): the lit/len symbol s as it stands, with
# no meaning to the model (286, 287, a length whose distance the caller writes himself).  ("dsym", s): the distance symbol s as it
# stands (30, 31).  ("bits", value, count): raw bits.
def used_symbols(tokens, eob=True):
    """(lit/len symbols, distance symbols) the tokens need"""
    ll, d = {256} if eob else set(), set()
    for t in tokens:
        if t[0] == "sym":
            ll.add(t[1])
        elif t[0] == "dsym":
            d.add(t[1])
        elif t[0] == "bits":
            pass
        elif t[0] == 0:
            ll.add(t[1])
        else:
            ll.add(t[2] if len(t) > 2 else length_symbol(t[0])[0])
            d.add(dist_symbol(t[1])[0])
    return ll, d


def lens_for(tokens, nll=None, nd=None):
    """(lit/len lengths, distance lengths): complete codes over what the tokens use (a second symbol is added where there is one only;
    no distance code at all is one zero length)"""
    ll, d = used_symbols(tokens)
    if len(ll) < 2:
        ll.add(0 if 0 not in ll else 1)
    nll = nll or max(257, max(ll) + 1)
    if not d:
        return complete_lens(ll, nll), [0] * (nd or 1)
    if len(d) < 2:
        d.add(0 if 0 not in d else 1)
    return complete_lens(ll, nll), complete_lens(d, nd or max(d) + 1)


def plain_rle(lengths):
    """the lengths list without a repeat symbol"""
    return [(v, 0) for v in lengths]


def greedy_rle(lengths):
    """the lengths list with 18 / 17 for runs of zeros and 16 for repeats, longest first"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11)); run -= k
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3)); run -= k
            out += [(v, 0)] * run
        i = j
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def expand_rle(rle):
    """the lengths a spelling stands for, as RFC 1951 reads it (a 16 behind a 17 or an 18 repeats their zero)"""
    out = []
    for s, x in rle:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


def kraft(lens):
    """the code space the lengths take, in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - v) for v in lens if v)


class Stream:
    """One raw DEFLATE stream under construction: blocks append at the current bit position.  `model` collects what the blocks stand
    for -- ("data", bytes) and ("tokens", list) --, `nbits` the bits written, `empty_mid` whether a non-final block added nothing."""

    def __init__(self):
        self.w = Bits()
        self.model = []
        self.nbits = 0
        self.blocks = []                   # (type, final, the model's output length behind the block)

    # ---- bits
    def put(self, v, nb):
        self.w.put(v, nb)
        self.nbits += nb

    def code(self, c, nb):
        self.w.code(c, nb)
        self.nbits += nb

    def align(self):
        self.put(0, -self.nbits % 8)

    def _head(self, final, btype):
        self.put(1 if final else 0, 1)
        self.put(btype, 2)

    # ---- blocks
    def stored(self, data, final=False, nlen=None, length=None):
        """LEN defaults to len(data), NLEN to its complement; either can lie"""
        self._head(final, 0)
        self.align()
        ln = len(data) if length is None else length
        self.put(ln, 16)
        self.put((ln ^ 0xffff) if nlen is None else nlen, 16)
        for b in data:
            self.put(b, 8)
        self.model.append(("data", bytes(data)))
        self.blocks.append((0, final))
        return self

    def _tokens(self, tokens, ll, dc, eob):
        for t in tokens:
            if t[0] == "sym":
                self.code(*ll[t[1]])
            elif t[0] == "dsym":
                self.code(*dc[t[1]])
            elif t[0] == "bits":
                self.put(t[1], t[2])
            elif t[0] == 0:
                self.code(*ll[t[1]])
            else:
                ls, lx = (t[2], t[3]) if len(t) > 2 else length_symbol(t[0])
                assert LBASE[ls - 257] + lx == t[0] and lx < (1 << LEXTRA[ls - 257])
                ds, dx = dist_symbol(t[1])
                self.code(*ll[ls])
                self.put(lx, LEXTRA[ls - 257])
                self.code(*dc[ds])
                self.put(dx, DEXTRA[ds])
        if eob:
            self.code(*ll[256])
        self.model.append(("tokens", [t for t in tokens if not isinstance(t[0], str)]))

    def fixed(self, tokens, final=False, eob=True):
        self._head(final, 1)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)
        self.blocks.append((1, final))
        return self

    def dynamic(self, tokens, ll_lens=None, d_lens=None, final=False, cl_lens=None, hclen=None, rle=None, hlit=None, hdist=None, eob=True,
                header_only=False):
        """ll_lens / d_lens: the code lengths (default: complete codes over what the tokens use).  rle: the lengths list's spelling,
        [(symbol, extra)] (default: plain_rle -- no repeats); a function takes the list and returns the spelling.  cl_lens: the 19
        code-length code lengths (default: a complete code over the spelling's symbols).  hlit / hdist / hclen: the header fields'
        VALUES (257.., 1.., 4..; default: the lists' sizes, and the shortest HCLEN)."""
        if ll_lens is None or d_lens is None:
            a, b = lens_for(tokens)
            ll_lens, d_lens = ll_lens or a, d_lens or b
        hlit = len(ll_lens) if hlit is None else hlit
        hdist = len(d_lens) if hdist is None else hdist
        seq = list(ll_lens) + list(d_lens)
        if rle is None:
            rle = plain_rle(seq)
        elif callable(rle):
            rle = rle(seq)
        if cl_lens is None:
            syms = {s for s, _ in rle if s != "bits"}
            if len(syms) < 2:
                syms.add(min({0, 1} - syms))
            cl_lens = complete_lens(syms, 19)
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[ORDER[i]]])
        self._head(final, 2)
        self.put(hlit - 257, 5)
        self.put(hdist - 1, 5)
        self.put(hclen - 4, 4)
        self.header_at = self.nbits        # where the code-length code's lengths begin
        for i in range(hclen):
            self.put(cl_lens[ORDER[i]], 3)
        self.clens_at = self.nbits         # where the lengths list begins
        cl = canonical(cl_lens)
        self.rle_at = []                   # the bit at which each (symbol, extra) begins
        for s, x in rle:
            self.rle_at.append(self.nbits)
            if s == "bits":                # raw bits: x = (value, count) -- a pattern no code has
                self.put(*x)
                continue
            self.code(*cl[s])
            if s in CL_EXTRA:
                self.put(x, CL_EXTRA[s])
        if not header_only:
            self._tokens(tokens, canonical(ll_lens), canonical(d_lens), eob)
        self.blocks.append((2, final))
        return self

    # ---- results
    def bytes(self):
        return bytes(self.w.out) + (bytes([self.w.acc & 255]) if self.w.n else b"")

    def expected(self, hist=b""):
        """what the stream decodes to behind `hist`: the token model over all blocks, or None when a distance points in front of hist"""
        buf = bytearray(hist)
        for kind, x in self.model:
            if kind == "data":
                buf += x
                continue
            for t in x:
                if t[0] == 0:
                    buf.append(t[1])
                    continue
                ln, d = t[0], t[1]
                if d > len(buf) or d > 32768:
                    return None
                if d >= ln:
                    at = len(buf) - d
                    buf += buf[at:at + ln]
                else:                      # an overlapping copy repeats its last d bytes
                    pat = bytes(buf[-d:])
                    buf += (pat * (ln // d + 1))[:ln]
        return bytes(buf[len(hist):])

    def flags(self):
        """RCX_W_EMPTY_BLOCK_MIDSTREAM (1): a block that is not the last one added nothing"""
        for (_, final), (kind, x) in zip(self.blocks, self.model):
            if not final and len(x) == 0:
                return 1
        return 0


def shifted(k, build, lit=0x61):
    """a stream whose first block is dynamic and holds k literals `lit` of ONE bit each (the code: lit 0, end of block 1; HDIST 1, no
    distance code), followed by what build(stream) appends: k moves everything behind it by k bits"""
    s = Stream()
    ll = [0] * 257
    ll[lit] = ll[256] = 1
    s.dynamic([(0, lit)] * k, ll, [0], rle=greedy_rle)
    build(s)
    return s
