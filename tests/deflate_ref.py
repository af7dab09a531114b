"""Plain references for the device BGZF compressor (csrc/hbam_deflate.hip, csrc/deflate_enc.h).

  RFC 1951 tables, symbol codes, canonical codes             len_code, dist_code, canonical
  optimal and length-limited optimal Huffman costs           huffman_cost, package_merge
  a byte-cursor stream parser down to the tokens             parse_deflate, parse_member, members
  the tokenizer exactly as hbam_deflate.hip's header states   tokens

The restatement pins the algorithm as documented; the compressed bytes stay the device's own.
A tuning change of the compressor edits one of the named parameters below, and says so."""
import heapq
import struct
import zlib

import numpy as np

# ---- the tokenizer's parameters (hbam_deflate.hip / deflate_enc.h) ----------------------------
CHUNK = 256        # positions probed in parallel; heads come from earlier chunks only
HBITS = 11         # hash heads: 2^HBITS entries, the most recent position of each hash
PROBE = 16         # bytes verified per candidate; a match the probe caps is extended
WINDOW = 32768     # a hash candidate is used if 4 < distance <= WINDOW
PERIODS = (1, 2, 3, 4)   # the short-period candidates, in this order, strict improvement
MAX_MATCH = 258
HASH_MUL = 2654435761


def accept(length, dist):
    """The accept rule of a probed match (ints or numpy arrays)."""
    return (length >= 4) | ((length == 3) & (dist <= 64))


# ---- RFC 1951 tables ---------------------------------------------------------------------------
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
         131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
         2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def len_code(length):
    """(symbol, extra bits, extra value) of a match length 3..258, from the tables."""
    if length == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LBASE[k] <= length)
    return 257 + i, LEXT[i], length - LBASE[i]


def dist_code(d):
    i = max(k for k in range(30) if DBASE[k] <= d)
    return i, DEXT[i], d - DBASE[i]


def df_hash(w, hbits=HBITS):
    """One-line restatement of the match hash of the little-endian dword w."""
    return ((w * HASH_MUL) & 0xffffffff) >> (32 - hbits)


def rev(code, nbits):
    r = 0
    for _ in range(nbits):
        r = r << 1 | (code & 1)
        code >>= 1
    return r


def canonical(lengths):
    """RFC 1951 3.2.2 canonical codes (MSB first) of the code lengths; 0 for unused symbols."""
    cnt = [0] * 17
    for L in lengths:
        cnt[L] += 1
    cnt[0] = 0
    code, nxt = 0, [0] * 17
    for L in range(1, 17):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    out = []
    for L in lengths:
        if L:
            out.append(nxt[L])
            nxt[L] += 1
        else:
            out.append(0)
    return out


def kraft(lengths, limit):
    """Kraft sum in units of 2^-limit."""
    return sum(1 << (limit - L) for L in lengths if L)


# ---- Huffman costs -----------------------------------------------------------------------------
def huffman_cost(f):
    """sum f * len of an optimal prefix code over the used symbols (one used symbol: 1 bit each)."""
    h = [w for w in f if w]
    if len(h) == 0:
        return 0
    if len(h) == 1:
        return h[0]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def huffman_depth(f):
    """Depth of one optimal tree (ties: lower weight first, then shallower first)."""
    h = [(w, 0) for w in f if w]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def package_merge(f, limit):
    """Optimal code lengths with no length above limit (Larmore & Hirschberg's package-merge)."""
    n = len(f)
    used = sorted((w, i) for i, w in enumerate(f) if w)
    m = len(used)
    out = [0] * n
    if m == 0:
        return out
    if m == 1:
        out[used[0][1]] = 1
        return out
    assert m <= 1 << limit
    leaves = []
    for w, i in used:
        v = np.zeros(n, np.int32)
        v[i] = 1
        leaves.append((w, v))
    prev = leaves
    for _ in range(limit - 1):
        pk = [(prev[2 * k][0] + prev[2 * k + 1][0], prev[2 * k][1] + prev[2 * k + 1][1])
              for k in range(len(prev) // 2)]
        prev = sorted(leaves + pk, key=lambda x: x[0])
    tot = np.zeros(n, np.int32)
    for _, v in prev[:2 * m - 2]:
        tot += v
    return [int(x) for x in tot]


def cost(f, lengths):
    return sum(w * L for w, L in zip(f, lengths))


# ---- stream parser -----------------------------------------------------------------------------
class Bits:
    """LSB-first bit reader with a byte cursor and a small accumulator."""

    def __init__(self, data):
        self.d = bytes(data) + bytes(16)
        self.total = 8 * len(data)
        self.bp = 0      # next byte to load
        self.acc = 0
        self.n = 0       # bits in acc

    def need(self, k):
        while self.n < k:
            self.acc |= int.from_bytes(self.d[self.bp:self.bp + 8], "little") << self.n
            self.bp += 8
            self.n += 64

    def get(self, k):
        if k == 0:
            return 0
        self.need(k)
        x = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return x

    @property
    def pos(self):
        return 8 * self.bp - self.n

    def align(self):
        self.get((-self.pos) % 8)


def _table(lengths, what):
    """Flat decode table indexed by the next maxlen bits (LSB first) -> symbol << 4 | length.
    An over-subscribed code, or an incomplete one of more than one symbol, is an error, as in
    zlib's inflate."""
    mx = max(lengths) if lengths else 0
    used = [L for L in lengths if L]
    if not used:
        return [], 0
    k = kraft(lengths, mx)
    if k > 1 << mx:
        raise ValueError("%s code is over-subscribed" % what)
    if k < 1 << mx and len(used) > 1:
        raise ValueError("%s code is incomplete" % what)
    t = np.full(1 << mx, -1, np.int32)
    for s, (L, c) in enumerate(zip(lengths, canonical(lengths))):
        if L:
            t[rev(c, L)::1 << L] = s << 4 | L
    return t.tolist(), mx


def _sym(bits, table, mx):
    bits.need(mx)
    e = table[bits.acc & ((1 << mx) - 1)]
    if e < 0:
        raise ValueError("invalid code at bit %d" % bits.pos)
    L = e & 15
    bits.acc >>= L
    bits.n -= L
    return e >> 4


def parse_header(bits, strict=True):
    """The dynamic block header after BTYPE -> dict(hlit, hdist, hclen, cl, cl_syms, ll, dl);
    cl_syms are the code-length symbols as sent.  strict=False accepts a set with no
    end-of-block code (a header writer can be asked for one; no inflater takes it)."""
    hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
    if hlit > 286 or hdist > 30:
        raise ValueError("too many length or distance symbols")
    cl = [0] * 19
    for i in range(hclen):
        cl[ORDER[i]] = bits.get(3)
    ct, cm = _table(cl, "code-length")
    if not ct:
        raise ValueError("empty code-length code")
    lens, syms = [], []
    while len(lens) < hlit + hdist:
        s = _sym(bits, ct, cm)
        syms.append(s)
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                raise ValueError("repeat with no previous length")
            lens += [lens[-1]] * (3 + bits.get(2))
        elif s == 17:
            lens += [0] * (3 + bits.get(3))
        else:
            lens += [0] * (11 + bits.get(7))
    if len(lens) != hlit + hdist:
        raise ValueError("a run passes the end of the lengths")
    if strict and lens[256] == 0:
        raise ValueError("no end-of-block code")
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, cl_syms=syms, ll=lens[:hlit], dl=lens[hlit:])


def check_dynamic_header(b):
    """What every dynamic header of the compressor must satisfy: the length limits, complete
    codes (a distance set of fewer than two codes is one code of length 1), and HLIT / HDIST /
    HCLEN with no trailing zero length sent."""
    ll, dl, cl = b["ll"], b["dl"], b["cl"]
    assert len(ll) == b["hlit"] and len(dl) == b["hdist"]
    assert max(ll) <= 15 and max(dl) <= 15 and max(cl) <= 7
    assert ll[256] > 0
    assert kraft(ll, 15) == 1 << 15, "lit/len code not complete"
    if sum(1 for x in dl if x) >= 2:
        assert kraft(dl, 15) == 1 << 15, "distance code not complete"
    else:
        assert sorted(dl)[-1] == 1 and sum(dl) == 1
    assert kraft(cl, 7) == 1 << 7, "code-length code not complete"
    assert b["hlit"] == 257 or ll[-1] != 0
    assert b["hdist"] == 1 or dl[-1] != 0
    assert b["hclen"] == 4 or cl[ORDER[b["hclen"] - 1]] != 0


def parse_deflate(raw):
    """Raw DEFLATE stream -> list of blocks, each a dict with btype, tokens (an int literal or a
    (length, distance) pair), for dynamic blocks hlit / hdist / hclen / cl / ll / dl, hdr_bits;
    plus the rebuilt bytes and the bits used.  Returns (blocks, data, bits)."""
    bits = Bits(raw)
    out = bytearray()
    blocks = []
    while True:
        start = bits.pos
        last, typ = bits.get(1), bits.get(2)
        b = dict(btype=typ, bit=start, tokens=[])
        toks = b["tokens"]
        if typ == 0:
            bits.align()
            ln, nln = bits.get(16), bits.get(16)
            if ln ^ nln != 0xffff:
                raise ValueError("stored block: LEN / NLEN mismatch")
            p = bits.pos // 8
            if p + ln > len(raw):
                raise ValueError("stored block passes the end")
            chunk = raw[p:p + ln]
            toks.extend(chunk)
            out += chunk
            bits = _skip(bits, raw, p + ln)
        elif typ == 3:
            raise ValueError("reserved block type")
        else:
            if typ == 1:
                ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
            else:
                b.update(parse_header(bits))
                ll, dl = b["ll"], b["dl"]
            b["hdr_bits"] = bits.pos - start
            lt, lm = _table(ll, "lit/len")
            dt, dm = _table(dl, "distance")
            while True:
                s = _sym(bits, lt, lm)
                if s < 256:
                    toks.append(s)
                    out.append(s)
                elif s == 256:
                    break
                else:
                    i = s - 257
                    if i >= 29:
                        raise ValueError("length symbol %d" % s)
                    ln = LBASE[i] + bits.get(LEXT[i])
                    if not dt:
                        raise ValueError("a match with no distance code")
                    ds = _sym(bits, dt, dm)
                    if ds >= 30:
                        raise ValueError("distance symbol %d" % ds)
                    dist = DBASE[ds] + bits.get(DEXT[ds])
                    if dist > len(out):
                        raise ValueError("distance %d before the start" % dist)
                    toks.append((ln, dist))
                    if dist >= ln:
                        out += out[len(out) - dist:len(out) - dist + ln]
                    else:
                        for _ in range(ln):
                            out.append(out[-dist])
            if bits.pos > bits.total:
                raise ValueError("stream ends inside a block")
        blocks.append(b)
        if last:
            break
    return blocks, bytes(out), bits.pos


def _skip(bits, raw, byte):
    nb = Bits(raw)
    nb.bp = byte
    return nb


def split_members(comp):
    """BGZF stream -> list of member byte strings (header checked)."""
    comp = bytes(comp)
    out, p = [], 0
    while p < len(comp):
        assert comp[p:p + 4] == b"\x1f\x8b\x08\x04", p
        assert comp[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        bs = struct.unpack_from("<H", comp, p + 16)[0] + 1
        out.append(comp[p:p + bs])
        p += bs
    assert p == len(comp)
    return out


def parse_member(member):
    """One BGZF member -> its single DEFLATE block (parse_deflate's dict) plus data, isize, crc_ok,
    size.  The rebuilt bytes must be zlib's inflate of the same member, every time."""
    member = bytes(member)
    raw = member[18:-8]
    crc, isz = struct.unpack_from("<II", member, len(member) - 8)
    d = zlib.decompressobj(-15)
    u = d.decompress(raw)
    assert d.eof and not d.unused_data
    blocks, data, nbits = parse_deflate(raw)
    assert data == u, "the parser's bytes are not zlib's"
    assert (nbits + 7) // 8 == len(raw)
    b = blocks[0]   # the device writes one block per member; zlib may write several
    b.update(nblocks=len(blocks), tokens=[t for x in blocks for t in x["tokens"]], data=data, isize=isz,
             crc_ok=zlib.crc32(u) == crc, size=len(member))
    return b


# ---- the tokenizer, serially ------------------------------------------------------------------
def _prefix(s, a, p, lim, width):
    """Common prefix of s[a..] and s[p..] for index arrays a, p, at most lim (array) <= width."""
    k = np.arange(width)
    eq = (s[a[:, None] + k] == s[p[:, None] + k]) & (k[None, :] < lim[:, None])
    stop = np.concatenate([~eq, np.ones((len(a), 1), bool)], axis=1)
    return stop.argmax(axis=1)


def probe(block, hbits=HBITS, probe_len=PROBE, window=WINDOW, chunk=CHUNK, periods=PERIODS):
    """Per position: (length, distance) of the match the device's probe takes, 0 where none."""
    n = len(block)
    s = np.zeros(n + MAX_MATCH + 64, np.uint8)
    s[:n] = np.frombuffer(bytes(block), np.uint8)
    bl = np.zeros(n, np.int64)
    bd = np.zeros(n, np.int64)
    if n < 4:
        return bl, bd
    P = np.arange(n - 3)                       # positions with four bytes
    lim = np.minimum(n - P, probe_len)
    for d in periods:
        q = P[P >= d]
        m = _prefix(s, q - d, q, lim[q], probe_len)
        better = m > bl[q]
        bl[q[better]] = m[better]
        bd[q[better]] = d
    # the most recent position of the same hash in an earlier chunk
    s32 = s.astype(np.uint64)
    w = s32[P] | s32[P + 1] << 8 | s32[P + 2] << 16 | s32[P + 3] << 24
    h = ((w * HASH_MUL) & 0xffffffff) >> (32 - hbits)
    key = np.sort((h << 20 | P.astype(np.uint64)).astype(np.int64))
    c0 = (P // chunk) * chunk
    i = np.searchsorted(key, (h.astype(np.int64) << 20 | c0), side="left") - 1
    ok = i >= 0
    cand = key[np.maximum(i, 0)]
    ok &= (cand >> 20) == h.astype(np.int64)
    a = cand & ((1 << 20) - 1)
    dist = P - a
    ok &= (dist > 4) & (dist <= window)
    q = P[ok]
    m = _prefix(s, a[ok], q, lim[q], probe_len)
    better = m > bl[q]
    bl[q[better]] = m[better]
    bd[q[better]] = dist[ok][better]
    # accept, then extend what the probe capped
    acc = accept(bl, bd)
    bl[~acc] = 0
    bd[~acc] = 0
    capped = np.nonzero(bl == probe_len)[0]
    for i0 in range(0, len(capped), 4096):
        q = capped[i0:i0 + 4096]
        full = np.minimum(n - q, MAX_MATCH)
        bl[q] += _prefix(s, q - bd[q] + probe_len, q + probe_len, full - probe_len, MAX_MATCH - probe_len)
    return bl, bd


def tokens(block, **kw):
    """The device's token list of one block: greedy over the probed matches, carried over the
    chunk boundaries.  A literal is an int, a match a (length, distance) pair."""
    bl, bd = probe(block, **kw)
    bl, bd = bl.tolist(), bd.tolist()
    out, p, n = [], 0, len(block)
    data = bytes(block)
    while p < n:
        if bl[p]:
            out.append((bl[p], bd[p]))
            p += bl[p]
        else:
            out.append(data[p])
            p += 1
    return out


def detokenize(toks):
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            ln, d = t
            for _ in range(ln):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out)
