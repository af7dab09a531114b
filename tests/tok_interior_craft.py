"""Crafted DEFLATE streams for the interior body of the specialised symbol loop (inflate_tok.h
tok_symbols), built with the RFC 1951 writer of tests/deflate_craft.py: the cases of
tests/test_tok_interior_*.py.  Every block uses code lengths that fit the specialised loop (lit/len
3..14, distances 3..9), so what varies is where a lane leaves the interior body: within
TOK_ITER_OUT = 260 bytes of the end of its output, or within TOK_FAST_BITS = 64 bits of the end
of its stream.

The token list of every case is explicit, so the iteration in which the hand-over happens follows
from the format alone: one iteration of the fast path takes a literal and then a second literal or a
match, or a match alone (iteration_tops below restates that, it is not derived from the decoder).
zlib vouches for every stream when it is built (inflated with the output capped at ISIZE, as the
decoder's contract says)."""
import random
import zlib

import deflate_craft as craft

LL, DL = craft.ll_lengths(3, 14), craft.d_lengths(3, 9, 20)
LC, DC = craft.canon(LL), craft.canon(DL)
LITS = [s for s in range(256) if LL[s]]
LENSYMS = [s for s in range(257, 286) if LL[s]]
ITER_OUT, FAST_BITS = 260, 64


def lit(rng):
    return ("lit", rng.choice(LITS))


def match(ln, dist):
    """the token of a match (ln, dist) over the symbols that have codes"""
    ls = max(s for s in LENSYMS if craft.LBASE[s - 257] <= ln)
    ds = max(d for d in range(len(DL)) if craft.DBASE[d] <= dist)
    lx, dx = ln - craft.LBASE[ls - 257], dist - craft.DBASE[ds]
    assert lx < (1 << craft.LEXT[ls - 257]) and dx < (1 << craft.DEXT[ds]), (ln, dist)
    return ("match", ls, lx, ds, dx, ln, dist)


MATCH_LENS = [3, 4, 7, 11, 12, 23, 26, 67, 82, 227, 257, 258]


def body(rng, n, op0=0):
    """random literals and matches giving exactly n bytes, the output so far being op0 bytes"""
    toks, op = [], op0
    while op < op0 + n:
        left = op0 + n - op
        lens = [x for x in MATCH_LENS if x <= left]
        if op > 0 and lens and rng.random() < 0.3:
            ln = rng.choice(lens)
            toks.append(match(ln, rng.randrange(1, min(op, 1024) + 1)))
            op += ln
        else:
            toks.append(lit(rng))
            op += 1
    return toks


def out_len(toks):
    return sum(1 if t[0] == "lit" else t[5] for t in toks)


def tok_bits(t):
    if t[0] == "lit":
        return LC[t[1]][1]
    return LC[t[1]][1] + craft.LEXT[t[1] - 257] + DC[t[3]][1] + craft.DEXT[t[3]]


def header_bits():
    w = craft.BitWriter()
    craft.dynamic_block(w, LL, DL, [], True)
    return w.n - LC[256][1]


def iteration_tops(toks):
    """[(tokens before, output bytes before, stream bits of those tokens)] at the top of every
    iteration of a fast path that takes literal + literal, literal + match, or a match alone"""
    tops, i, op, bits = [], 0, 0, 0
    while i <= len(toks):
        tops.append((i, op, bits))
        k = 1
        if i < len(toks) and toks[i][0] == "lit":
            k = 2  # the second lookup's symbol belongs to this iteration: literal, match or end of block
        for t in toks[i:i + k]:
            op += 1 if t[0] == "lit" else t[5]
            bits += tok_bits(t)
        i += k
    return tops


def stream(parts, isize=None):
    """raw DEFLATE of parts, each ("dyn", tokens) or ("stored", bytes); returns (raw, the first
    isize bytes zlib gives for it with its output capped there: all of them by default)"""
    w = craft.BitWriter()
    for i, p in enumerate(parts):
        final = i + 1 == len(parts)
        if p[0] == "dyn":
            craft.dynamic_block(w, LL, DL, p[1], final)
        else:
            craft.stored_block(w, p[1], final)
    raw = w.bytes()
    whole = zlib.decompress(raw, -15)
    if isize is None:
        return raw, whole
    u = zlib.decompressobj(-15).decompress(raw, isize)
    assert len(u) == isize and u == whole[:isize]
    return raw, u


SIZES = [1, 259, 260, 261, 262, 263, 520, 4096]


def _bits_case(target):
    """A block ending in four 258-byte matches whose stream has exactly `target` bits left at the top
    of an iteration at which the output is still more than 260 bytes from its end."""
    hb = header_bits()
    for seed in range(4000):
        rng = random.Random(7000 + seed)
        toks = body(rng, 400 + seed % 7) + [match(258, 1 + seed % 300)] * 4
        used = hb + sum(tok_bits(t) for t in toks) + LC[256][1]
        total = 8 * ((used + 7) // 8)
        isize = out_len(toks)
        for _, op, bits in iteration_tops(toks):
            if total - (hb + bits) == target and op + ITER_OUT <= isize:
                return toks
    raise AssertionError("no stream with %d bits left at an iteration top" % target)


TWO = {"two_blocks": 259, "two_long": 600}  # name -> output bytes of the second block


def two_block_parts(name):
    """(first, second): the tokens of two Huffman blocks of one stream whose first block ends in an
    iteration of the interior body and whose second re-enters tok_symbols.
    two_blocks: the first block's last iteration is a literal and the end-of-block symbol, at a top
    with op = ISIZE - 260, the last op that still qualifies (op + 260 <= ISIZE), and the second
    block has the 259 bytes that are left, so it never qualifies: the only length under 260 bytes
    for which the first block can end in the interior body (its end-of-block symbol is decoded in an
    iteration that starts at op <= ISIZE - 260 and takes one literal before it at the most).
    two_long: the second block is long enough to go back into the interior body itself."""
    rng = random.Random(31000 + TWO[name])
    first = body(rng, 999)
    if iteration_tops(first)[-1][0] == len(first):  # the end-of-block symbol alone at a top
        first.append(lit(rng))
    second = body(rng, TWO[name], out_len(first))
    i, op, _ = iteration_tops(first)[-1]
    isize = out_len(first) + TWO[name]
    assert i == len(first) - 1 and first[-1][0] == "lit" and op == out_len(first) - 1
    assert op + ITER_OUT <= isize and (name != "two_blocks" or op + ITER_OUT == isize)
    return first, second


def two_block_interior_iterations(name):
    """(iterations of the first block, iterations of the second block that start at least
    FAST_BITS from the stream's end and ITER_OUT from the output's): what a lane spends in the
    interior body, from the token lists alone"""
    first, second = two_block_parts(name)
    hb, eob = header_bits(), LC[256][1]
    t1, t2 = iteration_tops(first), iteration_tops(second)
    n1, isize = out_len(first), out_len(first) + out_len(second)
    before = hb + sum(tok_bits(t) for t in first) + eob + hb  # stream bits ahead of the second block's tokens
    total = 8 * ((before + sum(tok_bits(t) for t in second) + eob + 7) // 8)
    inner2 = sum(1 for _, op, bits in t2 if n1 + op + ITER_OUT <= isize and total - (before + bits) >= FAST_BITS)
    return len(t1), inner2


def cases():
    """name -> (raw, expected bytes); isize is the length of the expected bytes"""
    out = {}
    rng = random.Random(20250)
    for n in SIZES:  # 520: two iterations from the end of the interior body at the least
        out["n%d" % n] = stream([("dyn", body(rng, n))])
    # the last token is a 258-byte match that starts 1, 2 and 3 bytes before ISIZE (the n < 3 tail
    # token and the shortest cut match with a descriptor); the stream itself goes on
    for k in (1, 2, 3):
        toks = body(rng, 600 - k) + [match(258, 5)]
        out["tail%d" % k] = stream([("dyn", toks)], isize=600)
    # the hand-over with a pending packet: 150 iterations of two literals, then the last interior
    # iteration (literal + match of 23: a packet with a match mark; two literals: one without),
    # then a match in the first iteration after it
    pairs = [lit(rng) for _ in range(300)]
    t_mark = pairs + [lit(rng), match(23, 9), match(26, 40)]
    t_mark += [lit(rng) for _ in range(570 - out_len(t_mark))]
    t_plain = pairs + [lit(rng), lit(rng), match(26, 40)]
    t_plain += [lit(rng) for _ in range(561 - out_len(t_plain))]
    for name, toks, last in (("hand_mark", t_mark, 150), ("hand_plain", t_plain, 150)):
        tops = iteration_tops(toks)
        isize = out_len(toks)
        assert tops[last][1] + ITER_OUT <= isize < tops[last + 1][1] + ITER_OUT, name
        assert toks[tops[last + 1][0]][0] == "match", name
        out[name] = stream([("dyn", toks)])
    # the stream's last 64 bits begin at an iteration top, one bit before it and one bit after it
    for target in (FAST_BITS - 1, FAST_BITS, FAST_BITS + 1):
        out["bits%d" % target] = stream([("dyn", _bits_case(target))])
    # two Huffman blocks (two_block_parts below): the first ends inside the interior body
    for name in TWO:
        first, second = two_block_parts(name)
        out[name] = stream([("dyn", first), ("dyn", second)])
    out["dyn_stored"] = stream([("dyn", body(rng, 1500)), ("stored", bytes(rng.choice(LITS) for _ in range(300)))])
    # every match reaches back to the block's first byte: a flipped distance bit is "too far back"
    far, op = [lit(rng) for _ in range(300)], 300
    while op < 900:
        ln = rng.choice([3, 4, 7, 11])
        far += [match(ln, op), lit(rng)]
        op += ln + 1
    out["far"] = stream([("dyn", far)])
    return out


def corrupted(raw):
    """(a flip zlib still inflates, zlib's bytes for it), (a flip zlib rejects, None)"""
    return craft.flipped(raw, want_error=False), craft.flipped(raw, want_error=True)
