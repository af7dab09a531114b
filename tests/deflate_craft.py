"""Crafted DEFLATE streams for the specialised symbol loops of the Huffman lane pass (inflate_tok.h
tok_symbols): a small RFC 1951 writer that emits dynamic-Huffman blocks from chosen code-length
vectors and a token list, plus fixed and stored blocks, and the cases of tests/test_tok_spec_*.py.

Every code-length vector is a complete code unless a case says otherwise (a single distance code,
an empty distance table).  Every stream is checked against zlib.decompress(raw, -15) when it is
built: zlib vouches for the inputs, not the decoder under test."""
import random
import struct
import zlib

ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
         131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
         2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, x, k):  # k bits of x, LSB first
        self.v |= (x & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, c, k):  # a Huffman code: MSB first
        for i in range(k - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canon(lengths):
    """canonical codes of a code-length vector: {symbol: (code, length)}"""
    cnt = [0] * 16
    for L in lengths:
        cnt[L] += 1
    cnt[0] = 0
    code, nxt = 0, [0] * 16
    for L in range(1, 16):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    out = {}
    for s, L in enumerate(lengths):
        if L:
            out[s] = (nxt[L], L)
            nxt[L] += 1
    return out


def kraft_left(lengths):
    left = 1
    for L in range(1, 16):
        left = 2 * left - sum(1 for x in lengths if x == L)
    return left


def complete_counts(nsym, minl, maxl):
    """Codes per length of a complete code with exactly nsym symbols, shortest minl, longest maxl:
    2^minl - 1 codes of length minl, the last slot split down to two codes of length maxl, then
    codes split in two (longest first, so the short ones stay) until there are nsym."""
    cnt = [0] * 16
    if minl == maxl:
        cnt[minl] = 1 << minl
    else:
        cnt[minl] = (1 << minl) - 1
        for L in range(minl + 1, maxl):
            cnt[L] = 1
        cnt[maxl] = 2
    while sum(cnt) < nsym:
        for L in range(maxl - 1, minl - 1, -1):
            if cnt[L] >= (2 if L == minl else 1):
                cnt[L] -= 1
                cnt[L + 1] += 2
                break
        else:
            raise ValueError("no complete code with %d symbols in %d..%d" % (nsym, minl, maxl))
    assert sum(cnt) == nsym and cnt[minl] and cnt[maxl], (cnt, nsym, minl, maxl)
    return cnt


def lengths_for(symbols, minl, maxl, size):
    """A code-length vector of `size` entries: the given symbols (most frequent first) get a
    complete code with lengths minl..maxl, shortest codes first; every other symbol length 0."""
    cnt = complete_counts(len(symbols), minl, maxl)
    ls = [L for L in range(1, 16) for _ in range(cnt[L])]
    out = [0] * size
    for s, L in zip(symbols, ls):
        out[s] = L
    assert kraft_left(out) == 0
    return out


LITS = [0x41 + i for i in range(58)]  # 'A'..'z'
LENSYMS = [257, 258, 261, 265, 270, 277, 284, 285]


def ll_lengths(minl, maxl, nlit=40):
    """lit/len lengths: literals first (the first one is the dominant literal), then 256, then length symbols"""
    syms = LITS[:nlit] + [256] + LENSYMS
    n = len(syms)
    lo = (1 << minl) if minl == maxl else (1 << minl) + maxl - minl
    if n < lo:
        raise ValueError("too few symbols")
    return lengths_for(syms, minl, maxl, 286)


def d_lengths(minl, maxl, nd):
    return lengths_for(list(range(nd)), minl, maxl, nd)


def tokens(rng, ll, dl, out_target, op0=0):
    """Random tokens over the symbols that have codes: literals and matches (dist <= output so far),
    until about out_target bytes; every symbol of both alphabets is a candidate each time."""
    lits = [s for s in range(256) if ll[s]]
    lens = [s for s in range(257, 286) if s < len(ll) and ll[s]]
    dists = [s for s in range(len(dl)) if dl[s]]
    toks, op, end = [], op0, op0 + out_target
    while op < end:
        pick = rng.randrange(len(lits) + len(lens))
        if pick >= len(lits) and dists and op > 0:
            ls = lens[pick - len(lits)]
            ds = rng.choice(dists)
            if DBASE[ds] <= op:
                ln = LBASE[ls - 257] + rng.randrange(1 << LEXT[ls - 257])
                dist = min(op, DBASE[ds] + rng.randrange(1 << DEXT[ds]))
                toks.append(("match", ls, ln - LBASE[ls - 257], ds, dist - DBASE[ds], ln, dist))
                op += ln
                continue
        toks.append(("lit", rng.choice(lits)))
        op += 1
    return toks, op


def put_tokens(w, toks, lc, dc):
    for t in toks:
        if t[0] == "lit":
            w.code(*lc[t[1]])
        else:
            _, ls, lx, ds, dx, _, _ = t
            w.code(*lc[ls])
            w.put(lx, LEXT[ls - 257])
            w.code(*dc[ds])
            w.put(dx, DEXT[ds])
    w.code(*lc[256])


def dynamic_block(w, ll, dl, toks, final):
    """One dynamic-Huffman block.  The code-length code gives lengths 0..15 four bits each (a
    complete code; no repeat symbols), so the header states every length literally."""
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(ll) - 257, 5)
    w.put(len(dl) - 1, 5)
    w.put(19 - 4, 4)
    cl = [4] * 16 + [0, 0, 0]
    for s in ORDER:
        w.put(cl[s], 3)
    cc = canon(cl)
    for L in list(ll) + list(dl):
        w.code(*cc[L])
    put_tokens(w, toks, canon(ll), canon(dl))


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def fixed_block(w, toks, final):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, toks, canon(FIXED_LL), canon(FIXED_D))


def stored_block(w, data, final):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xffff, 16)
    for b in data:
        w.put(b, 8)


def fits(ll, dl):
    """What tok_build's fit bits must say, restated from the lengths: both codes complete, neither
    has a length 1 or 2, no distance code is longer than 11 bits."""
    lu, du = [x for x in ll if x], [x for x in dl if x]
    return bool(lu and du and kraft_left(ll) == 0 and kraft_left(dl) == 0 and min(lu) >= 3 and min(du) >= 3
                and max(du) <= 11)


def make(seed, parts, out_each=1500):
    """One raw DEFLATE stream of the given parts: ("dyn", ll, dl) | ("fixed",) | ("stored",).
    Returns (raw, inflated bytes, [True / False per Huffman-coded part: the specialised body fits])."""
    rng = random.Random(seed)
    w, op, bodies = BitWriter(), 0, []
    for i, p in enumerate(parts):
        final = i + 1 == len(parts)
        if p[0] == "dyn":
            toks, op = tokens(rng, p[1], p[2], out_each, op)
            dynamic_block(w, p[1], p[2], toks, final)
            bodies.append(fits(p[1], p[2]))
        elif p[0] == "fixed":
            toks, op = tokens(rng, [8 if s in LITS or s in LENSYMS else 0 for s in range(286)], [5] * 30, out_each, op)
            fixed_block(w, toks, final)
            bodies.append(True)  # 7..9 and 5..5, both complete
        else:
            data = bytes(rng.choice(LITS) for _ in range(300))
            stored_block(w, data, final)
            op += len(data)
    raw = w.bytes()
    u = zlib.decompress(raw, -15)
    assert len(u) == op and len(raw) >= 200, (len(u), op, len(raw))
    return raw, u, bodies


def cases():
    """name -> (raw, inflated, bodies): every case of the issue, built once."""
    ll3, d3 = ll_lengths(3, 14), d_lengths(3, 9, 20)
    out = {}

    def add(name, *parts):
        out[name] = make(len(out) + 1, parts)

    add("ll_min1", ("dyn", ll_lengths(1, 14), d3))            # one dominant literal
    add("ll_min2", ("dyn", ll_lengths(2, 14), d3))
    add("ll_min3", ("dyn", ll3, d3))                           # the boundary of the folded pair
    add("ll_min4", ("dyn", ll_lengths(4, 12), d3))
    add("ll_max14", ("dyn", ll_lengths(3, 14), d_lengths(3, 11, 20)))
    add("ll_max15", ("dyn", ll_lengths(3, 15), d3))            # no high trimming for lit/len: still fits
    add("d_max9", ("dyn", ll3, d_lengths(3, 9, 20)))
    add("d_max10", ("dyn", ll3, d_lengths(3, 10, 20)))
    add("d_max11", ("dyn", ll3, d_lengths(3, 11, 20)))
    add("d_max12", ("dyn", ll3, d_lengths(3, 12, 20)))
    add("d_max15", ("dyn", ll3, d_lengths(3, 15, 20)))
    add("d_min1", ("dyn", ll3, d_lengths(1, 9, 20)))
    add("d_min2", ("dyn", ll3, d_lengths(2, 9, 20)))
    add("d_single", ("dyn", ll3, [1]))                          # incomplete, legal, never fits
    add("d_empty", ("dyn", lengths_for(LITS[:40] + [256], 3, 14, 286)[:257], [0]))  # no matches at all
    add("fit_then_not", ("dyn", ll3, d3), ("dyn", ll_lengths(2, 14), d3))
    add("not_then_fit", ("dyn", ll3, d_lengths(3, 12, 20)), ("dyn", ll3, d3))
    add("dyn_then_fixed", ("dyn", ll3, d3), ("fixed",))
    add("dyn_then_stored", ("dyn", ll3, d3), ("stored",))
    return out


def flipped(raw, want_error):
    """raw with one bit of its symbol region flipped (second half of the stream): the first flip after
    which zlib still inflates to as many bytes but different ones (want_error False), or after which zlib
    raises (True).  Returns (raw', zlib's bytes or None)."""
    ref = zlib.decompress(raw, -15)
    for bit in range(8 * (len(raw) // 2), 8 * len(raw) - 64):
        b = bytearray(raw)
        b[bit >> 3] ^= 1 << (bit & 7)
        try:
            u = zlib.decompress(bytes(b), -15)
        except zlib.error:
            if want_error:
                return bytes(b), None
            continue
        if not want_error and len(u) == len(ref) and u != ref:
            return bytes(b), u
    raise AssertionError("no such flip")


def bgzf(raw, u, crc=None):
    """One BGZF member around a raw stream (crc: the CRC to state, default that of u)."""
    bsize = 18 + len(raw) + 8
    head = b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + raw + struct.pack("<II", zlib.crc32(u) if crc is None else crc, len(u))
