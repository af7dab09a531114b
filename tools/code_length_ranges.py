"""Huffman code-length ranges of the DEFLATE blocks of a BAM / BGZF file or of a generated body:
what the specialised symbol loops of the Huffman lane pass (inflate_tok.h) may rely on.

Per DEFLATE block: its type, the lit/len and distance code lengths in use (min..max) and whether
each code is complete.  Per 64 consecutive BGZF blocks (what one wave of k_inflate_tokens holds, a
lane per BGZF block): the union of those ranges and the loop body every DEFLATE-block round of that
wave would select.  Only the headers are decoded into tables; the symbols of a block are skipped
with a table walk (no token list, no output), which is what finding the next header needs.

    python tools/code_length_ranges.py FILE.bam ... [--gen SEED ...] [--blocks N] [--per-block]
"""
import argparse
import os
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflate_trace import DEXT, LEXT, ORDER  # noqa: E402

FAST = 10  # first-level table bits of the symbol skipper


def rev(c, n):
    return int("{:0{w}b}".format(c, w=n)[::-1], 2)


def tables(lengths):
    """code lengths -> (fast table of 2^FAST entries sym << 4 | len, {(code, len): sym} for longer codes)."""
    cnt = [0] * 16
    for L in lengths:
        cnt[L] += 1
    cnt[0] = 0
    code, nxt = 0, [0] * 16
    for L in range(1, 16):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    fast, slow = [0] * (1 << FAST), {}
    for s, L in enumerate(lengths):
        if not L:
            continue
        r = rev(nxt[L], L)
        nxt[L] += 1
        if L <= FAST:
            fast[r::1 << L] = [s << 4 | L] * (1 << (FAST - L))
        else:
            slow[(r, L)] = s
    return fast, slow


def shape(lengths):
    """(min, max, complete) of a code-length vector; (0, 0, False) for an empty table."""
    used = [L for L in lengths if L]
    if not used:
        return 0, 0, False
    left = 1
    for L in range(1, 16):
        left = 2 * left - sum(1 for x in used if x == L)
    return min(used), max(used), left == 0


class Reader:
    def __init__(self, raw):
        self.raw, self.pos, self.buf, self.n, self.used = raw, 0, 0, 0, 0

    def need(self, k):
        while self.n < k:
            self.buf |= int.from_bytes(self.raw[self.pos:self.pos + 4], "little") << self.n
            self.pos += 4
            self.n += 32

    def get(self, k):
        self.need(k)
        x = self.buf & ((1 << k) - 1)
        self.buf >>= k
        self.n -= k
        self.used += k
        return x

    def sym(self, fast, slow):
        self.need(15)
        e = fast[self.buf & ((1 << FAST) - 1)]
        if e:
            self.get(e & 15)
            return e >> 4
        for L in range(FAST + 1, 16):
            s = slow.get((self.buf & ((1 << L) - 1), L))
            if s is not None:
                self.get(L)
                return s
        raise ValueError("invalid code at bit %d" % self.used)


def deflate_blocks(raw):
    """raw DEFLATE -> [{type, ll: (min, max, complete), d: (...)}], every block of the stream."""
    rd, out = Reader(raw), []
    while True:
        last, typ = rd.get(1), rd.get(2)
        if typ == 0:
            rd.get((8 - rd.used % 8) % 8)
            ln = rd.get(16)
            rd.get(16)
            for _ in range(ln):
                rd.get(8)
            out.append({"type": 0})
        else:
            if typ == 1:
                ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
            else:
                hlit, hdist, hclen = rd.get(5) + 257, rd.get(5) + 1, rd.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[ORDER[i]] = rd.get(3)
                ct = tables(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = rd.sym(*ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + rd.get(2))
                    elif s == 17:
                        lens += [0] * (3 + rd.get(3))
                    else:
                        lens += [0] * (11 + rd.get(7))
                ll, dl = lens[:hlit], lens[hlit:]
            out.append({"type": typ, "ll": shape(ll), "d": shape(dl)})
            lt, dt = tables(ll), tables(dl)
            while True:  # skip the symbols
                s = rd.sym(*lt)
                if s < 256:
                    continue
                if s == 256:
                    break
                rd.get(LEXT[s - 257])
                ds = rd.sym(*dt)
                rd.get(DEXT[ds])
        if last:
            break
    assert rd.used <= 8 * len(raw) and 8 * len(raw) - rd.used < 8,(rd.used, 8 * len(raw))
    return out


def bgzf_members(data):
    o = 0
    while o + 18 <= len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04", o
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        yield bytes(data[o + 18:o + bsize - 8]), struct.unpack_from("<I", data, o + bsize - 4)[0]
        o += bsize


def body_of(d):
    """The loop body a table pair fits, as tok_build's fit bits decide it: both codes complete and
    without lengths 1 and 2; distance lengths <= 11 -> 'd4' (the specialised body: lit/len pairs
    1..6, distance pairs 1..4); <= 13 -> 'd5' (what a "distance pairs 1..5" body would take; not
    instantiated, it runs the generic body: the ranges file shows one such block and no such wave);
    anything else 'generic'.  Stored blocks run no symbol loop."""
    if d["type"] == 0:
        return None
    (lmin, _, lc), (dmin, dmax, dc) = d["ll"], d["d"]
    if not (lc and dc and lmin >= 3 and dmin >= 3):
        return "generic"
    return "d4" if dmax <= 11 else "d5" if dmax <= 13 else "generic"


ORDERING = {"d4": 0, "d5": 1, "generic": 2}


def fmt(r):
    return "%d..%d%s" % (r[0], r[1], "" if r[2] else " (incomplete)") if r[1] else "empty"


def report(name, data, limit, per_block):
    print("== %s" % name)
    rows = []
    for i, (raw, isize) in enumerate(bgzf_members(data)):
        if limit and i >= limit:
            break
        if isize == 0 and len(raw) <= 2:
            rows.append([{"type": 1, "ll": (7, 9, True), "d": (5, 5, True)}])  # the empty member: one fixed block
            continue
        assert len(zlib.decompress(raw, -15)) == isize
        rows.append(deflate_blocks(raw))
    nd = sum(len(r) for r in rows)
    types = [sum(1 for r in rows for d in r if d["type"] == t) for t in range(3)]
    print("BGZF blocks %d, DEFLATE blocks %d (stored %d, fixed %d, dynamic %d), DEFLATE blocks per BGZF block %s"
          % (len(rows), nd, types[0], types[1], types[2], sorted(set(len(r) for r in rows))))
    hist = {}
    for r in rows:
        for d in r:
            if d["type"]:
                k = (fmt(d["ll"]), fmt(d["d"]), body_of(d))
                hist[k] = hist.get(k, 0) + 1
    print("per DEFLATE block: lit/len lengths | distance lengths | loop body | blocks")
    for k in sorted(hist):
        print("  %-22s | %-22s | %-7s | %d" % (k + (hist[k],)))
    if per_block:
        for i, r in enumerate(rows):
            print("  block %5d: %s" % (i, "; ".join("stored" if not d["type"] else "%s / %s" % (fmt(d["ll"]), fmt(d["d"]))
                                                       for d in r)))
    print("per wave (64 consecutive BGZF blocks), per DEFLATE-block round: union lit/len | union distance | body")
    wh = {}
    for w in range(0, len(rows), 64):
        lanes = rows[w:w + 64]
        for k in range(max(len(r) for r in lanes)):
            ds = [r[k] for r in lanes if k < len(r) and r[k]["type"]]
            if not ds:
                continue
            lu = (min(d["ll"][0] for d in ds), max(d["ll"][1] for d in ds), all(d["ll"][2] for d in ds))
            dne = [d["d"] for d in ds if d["d"][1]]
            du = (min(x[0] for x in dne), max(x[1] for x in dne), all(d["d"][2] for d in ds)) if dne else (0, 0, False)
            body = max((body_of(d) for d in ds), key=lambda b: ORDERING[b])
            print("  wave %4d round %d: %-8s | %-8s | %s" % (w // 64, k, fmt(lu), fmt(du), body))
            wh[body] = wh.get(body, 0) + 1
    print("wave rounds by body: %s" % ", ".join("%s %d" % (b, wh[b]) for b in sorted(wh, key=lambda b: ORDERING[b])))
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--gen", type=int, action="append", default=[], metavar="SEED",
                    help="the benchmark generator's body for this seed (genbam.generate_range(1, 0, 1, seed=SEED))")
    ap.add_argument("--blocks", type=int, default=0, help="only the first N BGZF blocks of each input")
    ap.add_argument("--per-block", action="store_true")
    a = ap.parse_args()
    for seed in a.gen:
        import genbam
        report("generated body, seed %d" % seed, bytes(genbam.generate_range(1, 0, 1, seed=seed, threads=4)),
               a.blocks, a.per_block)
    for p in a.paths:
        report(os.path.relpath(p), open(p, "rb").read(), a.blocks, a.per_block)


if __name__ == "__main__":
    main()
