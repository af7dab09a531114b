"""Crafted DEFLATE streams for the bit-cursor reader of the Huffman lane pass (inflate_tok.h EIn,
ein_window): the smallest shapes at which a reader that holds a cursor over a 256-bit ring of two
128-bit banks can go wrong.  Streams are written with tests/deflate_craft.py and zlib on the CPU
vouches for each when it is built (bytes for the good ones; "incomplete" or an error for the two
bad ones).

A case is (raw, inflated bytes or None, ISIZE, kind, phase): kind "ok" / "short" (zlib runs out of
input: INF_SHORT) / "data" (zlib raises: INF_DATA); phase is the address mod 16 the stream's first
byte must have, or None where any will do.  place() orders cases and fillers so that each phase
holds, for the CPU model (which puts block b at address b mod 16) and for a BGZF file (where a
member's stream starts 18 bytes into it)."""
import random
import zlib

import deflate_craft as craft

LL3, D3 = craft.ll_lengths(3, 14), craft.d_lengths(3, 9, 20)
A, Z = 0x41, 0x7a


def lit(s):
    return ("lit", s)


def match(ls, lx, ds, dx):
    return ("match", ls, lx, ds, dx, craft.LBASE[ls - 257] + lx, craft.DBASE[ds] + dx)


def out_len(toks):
    return sum(1 if t[0] == "lit" else t[5] for t in toks)


def _vouched(raw):
    u = zlib.decompress(raw, -15)
    return raw, u, len(u), "ok", None


def _dyn(ll, dl, toks):
    w = craft.BitWriter()
    craft.dynamic_block(w, ll, dl, toks, True)
    return w


def _fixed_lits(k):
    """a fixed-Huffman block of k literals 'A': 3 + 8k + 7 bits = k + 2 bytes"""
    w = craft.BitWriter()
    craft.fixed_block(w, [lit(A)] * k, True)
    raw = w.bytes()
    assert len(raw) == k + 2
    return raw


def _start_stream():
    """a dynamic block of exactly 300 bytes"""
    for seed in range(1, 200):
        for target in range(300, 520, 4):
            toks, _ = craft.tokens(random.Random(seed), LL3, D3, target)
            raw = _dyn(LL3, D3, toks).bytes()
            if len(raw) == 300:
                return raw
    raise AssertionError("no 300-byte stream")


def _wide(spec):
    """>= 64 iterations in a row of a literal and a match at the widest codes: generic loop
    15 + 15 + 5 + 15 + 13 = 63 bits, specialised loop 14 + 14 + 5 + 10 + 13 = 56 bits.  The stream
    first builds 16,513 bytes of output with cheap matches (3-bit or 2-bit codes), since distance
    codes 28 / 29 need 16,385 bytes behind them."""
    minl, maxl, dmax = (3, 14, 10) if spec else (2, 15, 15)
    nshort = (1 << minl) - 1
    nsyms = nshort + (maxl - minl - 1) + 2
    fill = [0x30 + i for i in range(nsyms - 5)]
    ll = craft.lengths_for([285, 0x61, 256] + fill + [Z, 284], minl, maxl, 286)
    dl = craft.lengths_for([0] + list(range(1, 28)) + [28, 29], minl, dmax, 30)
    assert ll[Z] == ll[284] == maxl and dl[28] == dl[29] == dmax and ll[285] == minl and dl[0] == minl
    assert craft.fits(ll, dl) == spec
    rng = random.Random(7 if spec else 8)
    toks = [lit(0x61)] + [match(285, 0, 0, 0)] * 64
    op = out_len(toks)
    for _ in range(70):
        toks.append(lit(Z))
        op += 1
        ds = rng.choice([d for d in (28, 29) if craft.DBASE[d] <= op])
        dx = rng.randrange(min(1 << 13, op - craft.DBASE[ds] + 1))
        lx = rng.randrange(32)
        toks.append(match(284, lx, ds, dx))
        op += 227 + lx
    assert op < 65536
    return _vouched(_dyn(ll, dl, toks).bytes())


def _stored_after_dyn():
    """name -> case: a stored block after a dynamic one with the stored header at each of the 8 bit
    phases, and two of them placed so that LEN/NLEN straddles a dword and a quad edge"""
    out, seed = {}, 100
    while sum(1 for k in out if k.startswith("stored_ph")) < 8:
        seed += 1
        rng = random.Random(seed)
        toks, _ = craft.tokens(rng, LL3, D3, 300)
        w = craft.BitWriter()
        craft.dynamic_block(w, LL3, D3, toks, False)
        ph = w.n & 7
        if "stored_ph%d" % ph in out:
            continue
        lenoff = (w.n + 3 + 7) // 8  # byte offset of LEN in the stream
        craft.stored_block(w, bytes(rng.choice(craft.LITS) for _ in range(40)), True)
        c = _vouched(w.bytes())
        out["stored_ph%d" % ph] = c
        if ph == 5:
            out["lennlen_dword"] = c[:4] + ((6 - lenoff) % 16,)  # LEN at 6 mod 16: dwords 1 and 2
            out["lennlen_quad"] = c[:4] + ((14 - lenoff) % 16,)  # LEN at 14 mod 16: two quads
    return out


def _pads():
    """name -> case: the final code ends on the last bit of the last byte (pad0) or 1..7 bits before it"""
    out, seed = {}, 200
    while len(out) < 8:
        seed += 1
        toks, _ = craft.tokens(random.Random(seed), LL3, D3, 300)
        w = _dyn(LL3, D3, toks)
        out.setdefault("pad%d" % (-w.n & 7), _vouched(w.bytes()))
    return out


def cases():
    """name -> (raw, inflated bytes or None, ISIZE, kind, phase), built once per process"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    start = _start_stream()
    for a in range(16):  # the initial cursor and the first window at every address mod 16
        out["start%d" % a] = _vouched(start)[:4] + (a,)
    for k in range(39):  # 2..40 bytes: fewer than two quads are fetched, fp clamps to fend
        out["short%d" % (k + 2)] = _vouched(_fixed_lits(k))
    for name, end in (("end_before", 15), ("end_on", 0), ("end_after", 1)):  # stream end against a quad edge
        k = 40 + ((end - 5 - 42) % 16)
        c = _vouched(_fixed_lits(k))
        assert (5 + len(c[0])) % 16 == end
        out[name] = c[:4] + (5,)
    # every value of cursor & 31 and the ring wrapped more than once at 2-3 bits an iteration:
    # two symbols with 1-bit codes (generic loop)
    ll = [0] * 257
    ll[A] = ll[256] = 1
    out["bits1"] = _vouched(_dyn(ll, [1], [lit(A)] * 640).bytes())
    out["wide_generic"] = _wide(False)
    out["wide_spec"] = _wide(True)
    out.update(_stored_after_dyn())
    raw, u, _ = craft.make(31, [("stored",), ("fixed",)], out_each=400)
    out["fixed_after_stored"] = _vouched(raw)
    raw, u, _ = craft.make(32, [("dyn", LL3, D3)] * 3, out_each=500)
    out["three_dynamic"] = _vouched(raw)
    pads = _pads()
    out.update(pads)
    # the stream cut by a byte and by four: zlib consumes it all and wants more.  One byte takes the
    # end-of-block code only, so every byte of the output is there (one inflate call with avail_out
    # = ISIZE succeeds: INF_OK); four bytes take data symbols as well (INF_SHORT)
    raw, u = pads["pad0"][:2]
    for name, cut in (("cut1", 1), ("cut4", 4)):
        d = zlib.decompressobj(-15)
        part = d.decompress(raw[:-cut])
        assert not d.eof and u.startswith(part)
        whole = len(part) == len(u)
        out[name] = (raw[:-cut], u if whole else None, len(u), "ok" if whole else "short", None)
    assert out["cut1"][3] == "ok" and out["cut4"][3] == "short"
    # a distance past the start of the output in the last symbol
    toks = [lit(A)] * 10 + [match(257, 0, 7, 0)]  # distance 13 behind 10 bytes of output
    raw = _dyn(LL3, D3, toks).bytes()
    try:
        zlib.decompress(raw, -15)
        raise AssertionError("zlib accepts the bad distance")
    except zlib.error:
        pass
    out["bad_dist"] = (raw, None, 13, "data", None)
    _CASES = out
    return out


_CASES = None
_LONG = None


def long_member():
    """a 4 KiB block for the other lanes of a one-wave call: (raw, inflated bytes)"""
    global _LONG
    if _LONG is None:
        toks, _ = craft.tokens(random.Random(5), LL3, D3, 4096)
        raw = _dyn(LL3, D3, toks).bytes()
        _LONG = (raw, zlib.decompress(raw, -15))
    return _LONG


def filler(n):
    """a stored block of n >= 1 bytes: 5 + n bytes of stream"""
    w = craft.BitWriter()
    data = bytes(0x2e for _ in range(n))
    craft.stored_block(w, data, True)
    raw = w.bytes()
    assert len(raw) == 5 + n
    return raw, data


def place(names, at, step):
    """Order cases for a container that puts item i's stream at address at(i, bytes before it) mod 16
    and grows by step(stream length) per item.  Returns [(name or None, raw, bytes)]: None marks a
    filler put in front of a case to reach its phase."""
    cs, out, pos = cases(), [], 0
    for name in names:
        raw, u, isize, kind, phase = cs[name]
        while phase is not None and at(len(out), pos) % 16 != phase:
            # a filler of n data bytes moves what follows by step(5 + n) bytes and one item: where
            # the bytes count one filler reaches the phase, where the items count n does not matter
            n = next((n for n in range(1, 17) if at(len(out) + 1, pos + step(5 + n)) % 16 == phase), 1)
            fr, fu = filler(n)
            out.append((None, fr, fu))
            pos += step(5 + n)
        out.append((name, raw, u))
        pos += step(len(raw))
    return out
