"""Builds bzip2 streams bit by bit, from a chosen post-MTF symbol sequence, coding tables, selectors and origPtr -- what libbz2 never writes
included -- with a small model of the decoder's back half (the walk over L from origPtr, the run-length undo, the CRC) so that the
CRCs it fills in are the ones libbz2 checks.  Plain Python, written from the format description in DESIGN.md 3.20 (TEST INFRASTRUCTURE)."""

BLOCK_MARK = 0x314159265359
END_MARK = 0x177245385090
RUNA, RUNB = 0, 1


class Bits:
    """an MSB-first bit string"""

    def __init__(self):
        self.v = 0
        self.n = 0

    def put(self, value, width):
        assert 0 <= value < (1 << width) or width == 0
        self.v = (self.v << width) | value
        self.n += width

    def pad(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def crc_bz2(data, crc=0xFFFFFFFF, final=True):
    """polynomial 0x04C11DB7, MSB first, all-ones in and out"""
    for b in data:
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc ^ 0xFFFFFFFF if final else crc


def bitrev8(b):
    return int("{:08b}".format(b)[::-1], 2)


def bitrev32(x):
    return int("{:032b}".format(x)[::-1], 2)


def symbols_to_l(symbols, used):
    """the MTF / RUNA / RUNB stage: symbols (without the end-of-block symbol) over the sorted list of used bytes -> L"""
    mtf = sorted(used)
    out = bytearray()
    i = 0
    while i < len(symbols):
        s = symbols[i]
        if s <= RUNB:
            es, n = 0, 1
            while i < len(symbols) and symbols[i] <= RUNB:
                es += n if symbols[i] == RUNA else 2 * n
                n *= 2
                i += 1
            out += bytes([mtf[0]]) * es
            continue
        b = mtf.pop(s - 1)
        mtf.insert(0, b)
        out.append(b)
        i += 1
    return bytes(out)


def l_to_symbols(l, used):
    """the inverse: L -> symbols, runs of the front byte as RUNA / RUNB"""
    mtf = sorted(used)
    syms = []
    run = 0

    def flush():
        nonlocal run
        while run > 0:
            if run & 1:
                syms.append(RUNA)
                run = (run - 1) // 2
            else:
                syms.append(RUNB)
                run = (run - 2) // 2

    for b in l:
        j = mtf.index(b)
        if j == 0:
            run += 1
            continue
        flush()
        mtf.pop(j)
        mtf.insert(0, b)
        syms.append(j + 1)
    flush()
    return syms


def walk(l, orig):
    """libbz2's walk: tt[C[c] + rank] = i, tPos = tt[origPtr], then n times { byte = L[tPos], tPos = tt[tPos] }.
    -> (text, length of the cycle through origPtr)"""
    n = len(l)
    order = sorted(range(n), key=lambda i: (l[i], i))          # tt: sorted place -> index in L
    t = bytearray()
    p = order[orig]
    for _ in range(n):
        t.append(l[p])
        p = order[p]
    cyc, q = 1, order[orig]
    while q != orig and cyc <= n:
        q = order[q]
        cyc += 1
    return bytes(t), cyc


def unrle(t):
    """the run-length undo: after four equal bytes the next byte is a count of further copies; the state starts fresh"""
    out = bytearray()
    i, run, prev = 0, 0, -1
    while i < len(t):
        b = t[i]
        i += 1
        run = run + 1 if b == prev else 1
        prev = b
        out.append(b)
        if run == 4:
            if i < len(t):
                out += bytes([b]) * t[i]
                i += 1
            run, prev = 0, -1
    return bytes(out)


def rle1(data):
    """libbz2's first run-length step (runs of 4..255 + count)"""
    out = bytearray()
    i = 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 255:
            j += 1
        k = j - i
        if k >= 4:
            out += bytes([data[i]]) * 4 + bytes([k - 4])
        else:
            out += bytes([data[i]]) * k
        i = j
    return bytes(out)


def bwt(t):
    """rotation sort -> (L, origPtr); quadratic, for small texts"""
    n = len(t)
    d = t + t
    rot = sorted(range(n), key=lambda i: d[i:i + n])
    return bytes(d[i + n - 1] for i in rot), rot.index(0)


def canonical(lengths):
    """symbol -> (code, length): codes in order of (length, symbol), as libbz2's tables decode them (they may overflow their length when
    the lengths are over-subscribed: such symbols cannot be written)"""
    codes = {}
    code = 0
    for ln in range(min(lengths), max(lengths) + 1):
        for s, l in enumerate(lengths):
            if l == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


def block_bits(w, symbols, used, tables, selectors, orig, crc, randomised=0, n_selectors=None, n_groups=None, selector_values=None):
    """one block: the mark, the header and the symbols + end-of-block; tables: a list of lists of code lengths (alphaSize = used + 2
    each), selectors: the table of every group of 50 symbols."""
    alpha = len(used) + 2
    w.put(BLOCK_MARK, 48)
    w.put(crc, 32)
    w.put(randomised, 1)
    w.put(orig, 24)
    used = sorted(used)
    top = 0
    for b in used:
        top |= 1 << (15 - b // 16)
    w.put(top, 16)
    for i in range(16):
        if top >> (15 - i) & 1:
            m = 0
            for b in used:
                if b // 16 == i:
                    m |= 1 << (15 - b % 16)
            w.put(m, 16)
    w.put(len(tables) if n_groups is None else n_groups, 3)
    w.put(len(selectors) if n_selectors is None else n_selectors, 15)
    order = list(range(max(len(tables), 6)))
    for s in selectors:
        j = order.index(s)
        order.pop(j)
        order.insert(0, s)
        w.put((1 << (j + 1)) - 2, j + 1)                        # j ones, a zero
    for v in selector_values or []:                             # raw unary values beyond what `selectors` says (malformed streams)
        w.put((1 << (v + 1)) - 2, v + 1)
    for t in tables:
        assert len(t) == alpha
        cur = t[0]
        w.put(cur, 5)
        for ln in t:
            while cur < ln:
                w.put(0b10, 2)
                cur += 1
            while cur > ln:
                w.put(0b11, 2)
                cur -= 1
            w.put(0, 1)
    codes = [canonical(t) for t in tables]
    for i, s in enumerate(list(symbols) + [alpha - 1]):
        g = selectors[i // 50] if i // 50 < len(selectors) else selectors[-1]
        c, ln = codes[g][s]
        assert c < (1 << ln), "symbol %d has no code in table %d" % (s, g)
        w.put(c, ln)


def block(symbols, used, tables=None, selectors=None, orig=0, crc=None, **kw):
    """-> a dict for stream(): fills in flat 2-table coding, one selector per 50 symbols and the CRC libbz2 will compute"""
    alpha = len(used) + 2
    if tables is None:
        ln = max(1, (alpha - 1).bit_length())
        tables = [[ln] * alpha, [ln] * alpha]
    if selectors is None:
        selectors = [0] * ((len(symbols) + 1 + 49) // 50)
    l = symbols_to_l(symbols, used)
    text, cyc = walk(l, orig) if l and orig < len(l) else (b"", 0)
    plain = unrle(text)
    return dict(symbols=symbols, used=used, tables=tables, selectors=selectors, orig=orig, crc=crc_bz2(plain) if crc is None else crc,
                plain=plain, l=l, cycle=cyc, kw=kw)


def block_from_text(text, **kw):
    """a block whose text BEFORE the run-length undo is `text` (small: the sort is quadratic)"""
    l, orig = bwt(text)
    used = sorted(set(text))
    return block(l_to_symbols(l, used), used, orig=orig, **kw)


def stream(level, blocks, combined=None, end=True):
    """-> (bytes, what it decodes to): 'BZh' level, the blocks, the end mark with the combined CRC, padding"""
    w = Bits()
    w.put(int.from_bytes(b"BZh" + bytes([ord("0") + level]), "big"), 32)
    comb = 0
    plain = b""
    for b in blocks:
        block_bits(w, b["symbols"], b["used"], b["tables"], b["selectors"], b["orig"], b["crc"], **b["kw"])
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ b["crc"]
        plain += b["plain"]
    if end:
        w.put(END_MARK, 48)
        w.put(comb if combined is None else combined, 32)
    w.pad()
    return w.bytes(), plain
