"""The serial reference of the bzip2 ENCODER's specification, plain Python on bz2_craft: the chunk rule with the block
size as a parameter, the run-length step, the rotation order with equal rotations by DESCENDING start, MTF + RUNA/RUNB, the table fit
(libbz2's partition, four iterations, Moffat-Katajainen lengths limited to 17 as the DEFLATE encoder limits its own) and the bits.
Every stage is kept so that a test can name the stage that differs (TEST INFRASTRUCTURE)."""
import bz2_craft as K

LIMIT = 17


def chunk_size(level):
    return 100000 * level - 19


def chunks(data, c):
    """-> [(offset, length)]: chunks of s input bytes, the last one shorter.  s = q - q // 64 with q = c L // R, R the sum of the run-length
    forms of the pieces of c input bytes, each on its own (2^30 at the most); while the longest form of a chunk is over c (what a block
    holds), s becomes min(s - 1, q - q // 64) with q = s c // longest, and from the fifth such turn on at most s // 2 as well"""
    big = len(data)
    if not big:
        return []
    q = c * big // sum(len(K.rle1(data[o:o + c])) for o in range(0, big, c))
    s = min(max(q - q // 64, 1), big, 1 << 30)
    turn = 0
    while True:
        parts = [(o, min(s, big - o)) for o in range(0, big, s)]
        longest = max(len(K.rle1(data[o:o + n])) for o, n in parts)
        if longest <= c:
            return parts
        q = s * c // longest
        t = min(s - 1, q - q // 64)
        if turn >= 4:
            t = min(t, s // 2)
        s = max(t, 1)
        turn += 1


def rotations(t):
    """-> (L, origPtr): rotations in lexicographic order, equal ones by descending start"""
    n = len(t)
    d = t + t
    rot = sorted(range(n), key=lambda i: (d[i:i + n], -i))
    return bytes(d[i + n - 1] for i in rot), rot.index(0)


def mk_depths(weights):
    """Moffat & Katajainen in place, exactly as k_deflate_encode.hip's de_code_lengths runs it: weights ascending -> depths"""
    a = list(weights)
    nu = len(a)
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, nu - 1):
        if leaf >= nu or a[root] < a[leaf]:
            a[nxt] = a[root]; a[root] = nxt; root += 1
        else:
            a[nxt] = a[leaf]; leaf += 1
        if leaf >= nu or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]; a[root] = nxt; root += 1
        else:
            a[nxt] += a[leaf]; leaf += 1
    a[nu - 2] = 0
    for nxt in range(nu - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avbl, used, dpth = 1, 0, 0
    root, nxt = nu - 2, nu - 1
    while avbl > 0:
        while root >= 0 and a[root] == dpth:
            used += 1; root -= 1
        while avbl > used:
            a[nxt] = dpth; nxt -= 1; avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    return a


def code_lengths(counts, lim=LIMIT):
    """counts per symbol -> lengths: weights max(count, 1), sorted ascending by (weight, index), depths, every count above `lim` bits
    folded into `lim`, the Kraft excess pushed down, the shortest lengths to the most frequent symbols.  -> (lengths, deepest unlimited)"""
    w = [max(c, 1) for c in counts]
    order = sorted(range(len(w)), key=lambda s: (w[s], s))
    depth = mk_depths([w[s] for s in order])
    cnt = [0] * 34
    for d in depth:
        cnt[min(d, 32)] += 1
    for i in range(lim + 1, 33):
        cnt[lim] += cnt[i]; cnt[i] = 0
    total = sum(cnt[i] << (lim - i) for i in range(1, lim + 1))
    while total != 1 << lim:
        cnt[lim] -= 1
        for i in range(lim - 1, 0, -1):
            if cnt[i]:
                cnt[i] -= 1; cnt[i + 1] += 2
                break
        total -= 1
    lens = [0] * len(w)
    j = len(w)
    for i in range(1, lim + 1):
        for _ in range(cnt[i]):
            j -= 1
            lens[order[j]] = i
    return lens, max(depth)


def n_groups(nmtf):
    return 2 if nmtf < 200 else 3 if nmtf < 600 else 4 if nmtf < 1200 else 5 if nmtf < 2400 else 6


def fit(syms, alpha):
    """syms: the block's symbols with the end symbol -> dict(tables, selectors, unchosen: tables no group chose in the last iteration,
    deepest: the deepest unlimited code of any table computed)"""
    nmtf = len(syms)
    ng = n_groups(nmtf)
    freq = [0] * alpha
    for s in syms:
        freq[s] += 1
    tables = [None] * ng
    rem, gs = nmtf, 0
    for part in range(ng, 0, -1):
        target = rem // part
        ge, acc = gs - 1, 0
        while acc < target and ge < alpha - 1:
            ge += 1
            acc += freq[ge]
        if ge > gs and part != ng and part != 1 and (ng - part) % 2 == 1:
            acc -= freq[ge]
            ge -= 1
        tables[part - 1] = [0 if gs <= v <= ge else 15 for v in range(alpha)]
        gs = ge + 1
        rem -= acc
    deepest, sels, counts = 0, [], []
    for _ in range(4):
        counts = [[0] * alpha for _ in range(ng)]
        sels = []
        for g in range(0, nmtf, 50):
            grp = syms[g:g + 50]
            costs = [sum(t[s] for s in grp) for t in tables]
            b = costs.index(min(costs))
            sels.append(b)
            for s in grp:
                counts[b][s] += 1
        tables = []
        for t in range(ng):
            lens, d = code_lengths(counts[t])
            tables.append(lens)
            deepest = max(deepest, d)
    return dict(tables=tables, selectors=sels, unchosen=[t for t in range(ng) if t not in sels], deepest=deepest)


def encode_block(piece):
    """one chunk -> the stages of its block"""
    t = K.rle1(piece)
    l, orig = rotations(t)
    used = sorted(set(t))
    alpha = len(used) + 2
    syms = K.l_to_symbols(l, used) + [alpha - 1]
    f = fit(syms, alpha)
    return dict(t=t, l=l, orig=orig, used=used, symbols=syms, tables=f["tables"], selectors=f["selectors"], unchosen=f["unchosen"],
                deepest=f["deepest"], crc=K.crc_bz2(piece), plain=piece)


def encode(data, level=9, c=None):
    """-> (the stream, the blocks' stages)"""
    assert 1 <= level <= 9
    c = chunk_size(level) if c is None else c
    blocks = [encode_block(data[o:o + n]) for o, n in chunks(data, c)]
    s, plain = K.stream(level, [dict(symbols=b["symbols"][:-1], used=b["used"], tables=b["tables"], selectors=b["selectors"], orig=b["orig"],
                                     crc=b["crc"], plain=b["plain"], kw={}) for b in blocks])
    assert plain == data
    return s, blocks
