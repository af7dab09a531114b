"""Crafted token blocks for the LZ77 resolve pass (k_resolve_units, csrc/resolve_units.h; contract
in csrc/resolve_dev.h): builders, the reference and a model of the kernel's bookkeeping.

A token list holds literals as ints and matches as (len, dist), as `_tokens` of test_gpu_parity.py.
A last token (n, dist) with n of 1 or 2 is a tail: the final match the output cut short.

  expand(tokens)       the byte-by-byte sequential expansion: the reference of every comparison
  token_block(tokens)  (io, bitmap, tail_token, tail_dist) as Context.resolve_tokens takes them
  deflate(tokens)      a raw DEFLATE stream of the same tokens (deflate_craft's block writers)
  model(tokens, a0)    the kernel's per-stretch bookkeeping restated from its comments and rules
                       (cutting rules, pre / ordered split, the readiness rule, 16-byte reads), the
                       units replayed on a byte buffer

The model follows the kernel's arithmetic, not its instructions: what it pins is the algorithm and
which path every case reaches; the masks, shifts, scans and wait counts are the device tests' part."""
import bisect
import random
import zlib

import numpy as np

import deflate_craft as dc

RS_W, RS_S = 512, 1024                     # resolve_dev.h
RS_BUF = RS_W + 2 * RS_S + 48
RS_MAXM = RS_S // 3 + 2
RU_CAP = 360                                # resolve_units.h
REL_MAX = 2047                              # 11-bit destination field of a unit record


# ---- reference ---------------------------------------------------------------------------------
def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 1 <= d <= len(out), (n, d, len(out))
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def size(tokens):
    return sum(1 if isinstance(t, int) else t[0] for t in tokens)


def split_tail(tokens):
    """(tokens without the tail, tail or None); a match shorter than 3 bytes is legal only last"""
    for t in tokens[:-1]:
        assert isinstance(t, int) or t[0] >= 3, t
    last = tokens[-1] if tokens else 0
    if not isinstance(last, int) and last[0] < 3:
        return tokens[:-1], last
    return tokens, None


def token_block(tokens):
    """(io, bitmap, tail_token, tail_dist): literals at their offsets, a 3-byte descriptor at every
    match start, one bitmap bit per match start, the tail as the Huffman pass states it"""
    isize = size(tokens)
    body, tail = split_tail(tokens)
    io = bytearray(isize)
    bm = np.zeros((isize + 31) // 32, np.uint32)
    op = 0
    for t in body:
        if isinstance(t, int):
            io[op] = t
            op += 1
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= min(op, 32768), (n, d, op)
            io[op:op + 3] = bytes([n - 3, (d - 1) & 0xff, (d - 1) >> 8])
            bm[op >> 5] |= np.uint32(1 << (op & 31))
            op += n
    tt = td = 0
    if tail is not None:
        tt, td = op | tail[0] << 16 | 0x80000000, tail[1]
        op += tail[0]
    assert op == isize
    return bytes(io), bm, tt, td


# ---- DEFLATE -----------------------------------------------------------------------------------
class Writer(dc.BitWriter):
    """deflate_craft's BitWriter with whole bytes moved out of the accumulator as they fill (the
    plain one shifts the whole stream on every put: quadratic on a 60 KB member)"""
    REV = [[int(format(c, "0%db" % k)[::-1], 2) if k else 0 for c in range(1 << k)] for k in range(10)]

    def __init__(self):
        super().__init__()
        self.done = bytearray()

    def put(self, x, k):
        self.v |= (x & ((1 << k) - 1)) << self.n
        self.n += k
        if self.n >= 64:
            nb = self.n >> 3
            self.done += (self.v & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self.v >>= 8 * nb
            self.n -= 8 * nb

    def code(self, c, k):
        self.put(self.REV[k][c], k)

    def bytes(self):
        return bytes(self.done) + super().bytes()


def match_token(n, d):
    """(len, dist) -> deflate_craft's match token: symbol and extra bits of both"""
    assert 3 <= n <= 258 and 1 <= d <= 32768
    ls = 285 if n == 258 else 257 + max(i for i in range(28) if dc.LBASE[i] <= n)
    ds = max(i for i in range(30) if dc.DBASE[i] <= d)
    lx, dx = n - dc.LBASE[ls - 257], d - dc.DBASE[ds]
    assert lx < 1 << dc.LEXT[ls - 257] and dx < 1 << dc.DEXT[ds]
    return ("match", ls, lx, ds, dx, n, d)


_MT = {}
STORED_MIN = 48  # literal runs at least this long go into stored sub-blocks


def deflate(tokens):
    """Raw DEFLATE of the tokens: fixed-Huffman blocks, stored sub-blocks for long literal runs.
    A tail (n, dist) is written as the 3-byte match the output cuts short: the stream then inflates
    to 3 - n bytes more than the tokens, and a member states ISIZE = size(tokens)."""
    body, tail = split_tail(tokens)
    if tail is not None:
        body = body + [(3, tail[1])]
    parts, run, cur = [], [], []

    def close_run():
        if len(run) >= STORED_MIN:
            if cur:
                parts.append(("fixed", list(cur)))
                cur.clear()
            for i in range(0, len(run), 65535):
                parts.append(("stored", bytes(run[i:i + 65535])))
        else:
            cur.extend(("lit", b) for b in run)
        run.clear()

    for t in body:
        if isinstance(t, int):
            run.append(t)
        else:
            close_run()
            if t not in _MT:
                _MT[t] = match_token(*t)
            cur.append(_MT[t])
    close_run()
    if cur or not parts:
        parts.append(("fixed", cur))
    w = Writer()
    for i, (kind, x) in enumerate(parts):
        (dc.fixed_block if kind == "fixed" else dc.stored_block)(w, x, i + 1 == len(parts))
    return w.bytes()


def deflate_literals(data):
    """Raw DEFLATE of an all-literal block over a small alphabet as one dynamic-Huffman block (a
    stored or fixed-Huffman 65536-byte member would pass the BSIZE limit)"""
    syms = sorted(set(data))
    assert 4 <= len(syms) <= 6
    ll = dc.lengths_for(syms + [256], 2, 3, 286)[:257]
    w = Writer()
    dc.dynamic_block(w, ll, [0], [("lit", b) for b in data], True)
    return w.bytes()


def member(tokens, literal_code=False):
    """(BGZF member, its bytes): ISIZE and CRC of expand(tokens)"""
    u = expand(tokens)
    raw = deflate_literals(u) if literal_code else deflate(tokens)
    m = dc.bgzf(raw, u)
    assert len(m) <= 65536, len(m)  # BSIZE is 16 bits
    return m, u


# ---- the model ---------------------------------------------------------------------------------
def cut(p, n, dist):
    """Units of one match -> (rule, h, [(q, bytes, distance, periodic)]), as the kernel cuts them."""
    if dist >= n or dist >= 16:
        rule, h, D = "plain", 0, dist
    elif dist < 8:
        rule, h, D = "periodic", min(n, 16), dist * -(-16 // dist)
    else:
        rule, h, D = "mid", dist, 2 * dist
    units = [(p, h, dist, rule == "periodic")] if h else []
    q = p + h
    while q < p + n:
        units.append((q, min(16, p + n - q), D, False))
        q += 16
    assert len(units) == (1 if h else 0) + (n - h + 15) // 16
    return rule, h, units


def _read16(buf, x):
    assert x >= 0
    v = bytes(buf[x:x + 16])
    return v + b"\0" * (16 - len(v))


def model(tokens, a0):
    """-> (bytes, stretches, seen).  stretches: one dict per stretch with starts, npre, nord, sched
    ("none" / "index" / "bitmap"), rounds, far (pre units whose source is read from global memory),
    maxrel, maxdeps (most earlier units one unit waits for), straddle (ordered units that wait and
    whose source begins before the stretch).  seen: what the block reached as a whole:
      rules     cutting rules used;  per, mid: the distances of periodic / 8..15 head units
      far_prev  far sources inside the stretch written back one iteration earlier;  far_old: older
      put       (path, destination & 3, bytes, source & 3) of every unit copied through LDS reads,
                path in "pre" / "index" / "bitmap" (LDS addresses, so they move with a0)."""
    io, bm, tt, td = token_block(tokens)
    isize = len(io)
    buf = bytearray(io)
    starts_all = np.nonzero(np.unpackbits(bm.view(np.uint8), bitorder="little")[:isize])[0].tolist()
    nstr = (a0 + isize + RS_S - 1) // RS_S
    stretches = []
    seen = dict(rules=set(), per=set(), mid=set(), far_prev=0, far_old=0, put=set())
    for k in range(nstr):
        s0 = k * RS_S
        lbase = RS_W + a0 - s0
        st = dict(starts=0, npre=0, nord=0, sched="none", rounds=0, far=0, maxrel=0, maxdeps=0, straddle=0)
        pre, ordered = [], []
        lo_i = bisect.bisect_left(starts_all, s0)
        hi_i = bisect.bisect_left(starts_all, s0 + RS_S)
        st["starts"] = hi_i - lo_i
        for p in starts_all[lo_i:hi_i]:
            n, dist = buf[p] + 3, (buf[p + 1] | buf[p + 2] << 8) + 1
            assert dist <= p and p + n <= isize and dist <= 32768
            e = p - dist + min(n, dist)
            rule, h, units = cut(p, n, dist)
            seen["rules"].add(rule)
            if dist >= n and e <= s0:
                assert rule == "plain"
                pre += units
            else:
                ordered += units
                if rule == "periodic":
                    seen["per"].add(dist)
                elif rule == "mid":
                    seen["mid"].add(dist)
        st["npre"], st["nord"] = len(pre), len(ordered)
        for q, n, dist, per in pre + ordered:
            st["maxrel"] = max(st["maxrel"], q - s0)
            assert lbase + q + 20 <= RS_BUF  # five dwords from the destination's dword
        # pre units: every source final; all reads of a step before its writes
        got = []
        for q, n, dist, per in pre:
            src = q - dist
            if src + RS_W + a0 < s0:
                st["far"] += 1
                age = (s0 - 1 - (src + a0)) // RS_S  # 0: the stretch written back last iteration
                seen["far_prev" if age == 0 else "far_old"] += 1
                assert src + a0 + 16 <= s0  # the 16 bytes read are written back
            else:
                seen["put"].add(("pre", (lbase + q) & 3, n, (lbase + src) & 3))
            got.append(_read16(buf, src))
        for (q, n, dist, per), v in zip(pre, got):
            buf[q:q + n] = v[:n]
        # ordered units: a unit runs in the round after the last earlier unit that writes its source
        vp = [u[0] for u in ordered]
        ve = [u[0] + u[1] for u in ordered]
        rnd = []
        for i, (q, n, dist, per) in enumerate(ordered):
            a = q - dist
            e = q if per else a + n
            assert e <= q and lbase + a >= 0  # never its own destination; inside the LDS window
            lo, hi = bisect.bisect_right(ve, a), bisect.bisect_left(vp, e)
            assert hi <= i
            deps = range(lo, hi)
            rnd.append(1 + max((rnd[j] for j in deps), default=0))
            st["maxdeps"] = max(st["maxdeps"], len(deps))
            if len(deps) and a < s0:
                st["straddle"] += 1
        if ordered:
            st["sched"] = "index" if len(ordered) <= 64 else "bitmap"
            st["rounds"] = max(rnd)
            for r in range(1, st["rounds"] + 1):
                idx = [i for i in range(len(ordered)) if rnd[i] == r]
                got = []
                for i in idx:
                    q, n, dist, per = ordered[i]
                    v = _read16(buf, q - dist)
                    if per:
                        v = bytes(v[j % dist] for j in range(16))
                    seen["put"].add((st["sched"], (lbase + q) & 3, n, (lbase + q - dist) & 3))
                    got.append(v)
                for i, v in zip(idx, got):
                    q, n, dist, per = ordered[i]
                    buf[q:q + n] = v[:n]
        if tt & 0x80000000 and (tt & 0xffff) // RS_S == k:
            p, n = tt & 0xffff, tt >> 16 & 0x7fff
            assert 0 < td <= p and p + n <= isize
            for t in range(n):
                buf[p + t] = buf[p - td + t % td]
        stretches.append(st)
    return bytes(buf), stretches, seen


# ---- block builder -----------------------------------------------------------------------------
class Block:
    """A token list under construction: literals from a seeded small alphabet, the output offset"""

    def __init__(self, seed, alphabet=b"ACGT"):
        self.rng = random.Random(seed)
        self.alphabet = alphabet
        self.toks, self.op = [], 0

    def lit(self, k=1):
        assert k >= 0
        self.toks += [self.rng.choice(self.alphabet) for _ in range(k)]
        self.op += k
        return self

    def to(self, pos):
        return self.lit(pos - self.op)

    def m(self, n, d):
        assert 1 <= d <= self.op and d <= 32768, (n, d, self.op)
        self.toks.append((n, d))
        self.op += n
        return self


# ---- BGZF streams for Context.inflate --------------------------------------------------------------
def table(members):
    """(file bytes, block table as Context.inflate takes it) of [(member, its bytes)]"""
    data, t = bytearray(), {"coff": [], "clen": [], "isize": [], "crc": []}
    for m, u in members:
        t["coff"].append(len(data))
        t["clen"].append(len(m))
        t["isize"].append(len(u))
        t["crc"].append(zlib.crc32(u))
        data += m
    return (np.frombuffer(bytes(data), np.uint8),
            {k: np.array(v, np.uint64 if k == "coff" else np.uint32) for k, v in t.items()})


def stream(members, lead, seed=9):
    """The members behind a lead member of `lead` literal bytes, a literal member between two of them
    wherever the next would not start at `lead` mod 16 again: every member's output then starts at
    lead mod 16 and has literal neighbours that nobody rewrites.  -> [(member, its bytes)]"""
    rng = random.Random(seed)
    out, pos = [], 0
    for m, u in members:
        k = (lead - pos) % 16
        if k:
            out.append(member([rng.randrange(256) for _ in range(k)]))
            pos += k
        out.append((m, u))
        pos += len(u)
    return out
