"""Crafted input blocks for the device BGZF compressor's tests: planted repeats at chosen lengths
and distances, chunk and block edges, and blocks whose tokens drive the Huffman builder to its
limits.  Everything is generated from fixed seeds; deflate_ref.tokens (the serial restatement of
the tokenizer) says what each block's tokens are, and the coverage each block exists for is
asserted on those tokens (tests/test_deflate_enc.py on the CPU, tests/test_deflate_gpu.py again
before it compares with the device).

A repeat is found through the hash heads only if no later position of an earlier chunk lands in
its bucket, so a planted string is redrawn until deflate_ref.df_hash says its bucket is free."""
import functools

import numpy as np

import deflate_ref as R

CHUNK = R.CHUNK


def hashes(buf):
    """df_hash of every position of buf that has four bytes."""
    s = np.frombuffer(bytes(buf), np.uint8).astype(np.uint64)
    if len(s) < 4:
        return np.zeros(0, np.uint64)
    w = s[:-3] | s[1:-2] << 8 | s[2:-1] << 16 | s[3:] << 24
    return ((w * R.HASH_MUL) & 0xffffffff) >> (32 - R.HBITS)


def plant(buf, a, p, L, rng, end_sep=True):
    """The same L fresh bytes (128..255) at a and at p (p's chunk later than a's), closed by two
    different bytes, drawn until the most recent earlier-chunk position in the string's bucket,
    seen from p, is a.  buf must be final in [a, chunk start of p)."""
    c0 = p // CHUNK * CHUNK
    assert a < c0 and p - a > 4 and a + L < p and L >= 4
    for _ in range(200):
        x = rng.integers(128, 256, L, dtype=np.uint8).tobytes()
        sa = int(rng.integers(0, 128))
        sp = (sa + 1 + int(rng.integers(0, 127))) % 128
        buf[a:a + L] = x
        buf[a + L] = sa
        buf[p:p + L] = x
        if end_sep:
            if len(buf) <= p + L:
                buf.extend(bytes(p + L + 1 - len(buf)))
            buf[p + L] = sp
        h = hashes(buf[a:c0 + 3])
        if a and p - 1 == a + L and buf[a - 1] == sa:
            continue    # the bytes before the two strings must differ, or the repeat is longer
        if not np.any(h[1:c0 - a] == h[0]):
            return
    raise AssertionError("no free bucket for a planted string")


def filler(rng, n):
    """n random bytes 0..127: no 4-gram is likely to repeat."""
    return bytearray(rng.integers(0, 128, n, dtype=np.uint8).tobytes())


# ---- length ladder ---------------------------------------------------------------------------
LENGTH_RANGES = [(4, 130), (131, 200), (201, 258)]


@functools.lru_cache(maxsize=None)
def length_ladder():
    """Blocks holding, for every L in 3..258, a repeat of exactly L bytes ended by a differing
    byte.  L = 3 comes from a period of 4 ("abcXabcY": a hash candidate needs four equal bytes).
    Returns [(block, [(L, distance), ...])]."""
    out = []
    for k, (lo, hi) in enumerate(LENGTH_RANGES):
        rng = np.random.default_rng(100 + k)
        buf = filler(rng, 300)
        want = []
        if k == 0:
            buf += bytes([200, 201, 202, 1, 200, 201, 202, 2])
            want.append((3, 4))
            buf += filler(rng, 40)
        for L in range(lo, hi + 1):
            a = len(buf)
            p = max(a + L + 1, (a // CHUNK + 1) * CHUNK)
            buf += filler(rng, p + L + 1 - a)
            plant(buf, a, p, L, rng)
            want.append((L, p - a))
        buf += filler(rng, 300)
        assert len(buf) <= 65280
        out.append((bytes(buf), want))
    return out


# ---- distance ladder -------------------------------------------------------------------------
def distance_block(D, seed, L=None):
    """A block with one repeat at distance D after low-entropy filler (period 2 over {0, 1}: two
    buckets), the planted string over 128..255."""
    rng = np.random.default_rng(seed)
    if D <= 4:   # a period: the short-period probes find it
        unit = bytes(200 + i for i in range(D))
        return bytes(filler(rng, 300)) + unit * (40 // D) + bytes(filler(rng, 300))
    L = L or (4 if D < 16 else 9)
    B = -(-(300 + D) // CHUNK) * CHUNK
    p = B + min(D - 1, 7)
    a = p - D
    buf = bytearray(bytes([0, 1]) * ((p + L + 1 + 300) // 2))
    if a + L + 1 > p:    # D == L + 1 at the least
        raise AssertionError("planted strings overlap")
    buf[a - 1] = 100
    plant(buf, a, p, L, rng)
    return bytes(buf)


@functools.lru_cache(maxsize=None)
def distance_ladder():
    """[(block, distance)]: for every distance code its base and its last distance."""
    ds = sorted({R.DBASE[c] for c in range(30)} | {R.DBASE[c] + (1 << R.DEXT[c]) - 1 for c in range(30)})
    assert {1, 4, 5, 24577, 32768} <= set(ds)
    return [(distance_block(D, 200 + i), D) for i, D in enumerate(ds)]


def beyond_window_block():
    """A repeat at distance 32769: one past the window."""
    return distance_block(32769, 333)


# ---- chunk and block edges -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_blocks():
    """[(label, block, wanted (length, distance) or None)]."""
    out = []
    rng = np.random.default_rng(400)
    # a 258-byte match that starts at chunk position 255 and crosses two chunk boundaries
    buf = filler(rng, 3 * CHUNK + 255 + 258 + 1 + 100)
    plant(buf, 10, 3 * CHUNK + 255, 258, rng)
    out.append(("crosses_two_chunks", bytes(buf), (258, 3 * CHUNK + 245)))
    # a match whose end is a chunk end
    buf = filler(rng, 4 * CHUNK + 50)
    plant(buf, 100, 4 * CHUNK - 40, 40, rng)
    out.append(("ends_on_chunk_end", bytes(buf), (40, 4 * CHUNK - 140)))
    # a match that ends on the block's last byte
    for L in (4, 5, 21, 258):
        buf = filler(rng, 2 * CHUNK + 17 + L)
        plant(buf, 50, 2 * CHUNK + 17, L, rng, end_sep=False)
        assert len(buf) == 2 * CHUNK + 17 + L
        out.append(("ends_on_block_end_%d" % L, bytes(buf), (L, 2 * CHUNK - 33)))
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 259, 511, 512, 513, 65279, 65280):
        out.append(("len_%d" % n, rng.integers(0, 4, n, dtype=np.uint8).tobytes(), None))
    return out


# ---- Huffman extremes ------------------------------------------------------------------------
# matches wanted per distance code: Fibonacci-like over 17 codes (the Huffman tree of the counts
# is 16 deep).  Periods 4, 3 and 2 carry the three largest counts (a period of 1 has only 256
# different units, and a unit seen before is found through the hash at a far distance instead);
# the other codes are planted over chunk boundaries, nested: targets to the right of the boundary,
# sources to its left, every next pair at least 10 further apart.
DEEP_DIST_COUNTS = {3: 1730, 2: 1060, 1: 640, 12: 400, 0: 233, 4: 144, 8: 89, 9: 55, 10: 34, 11: 21, 13: 13,
                    5: 8, 6: 5, 7: 3, 14: 2, 15: 1, 16: 1}


@functools.lru_cache(maxsize=None)
def deep_distance_block():
    rng = np.random.default_rng(500)
    nb = 254                                  # chunk boundaries used: 256, 512, ...
    per = [[] for _ in range(nb)]
    k = 0
    for c in (4, 5, 6, 7):                    # distances 5..16: one per boundary
        for _ in range(DEEP_DIST_COUNTS[c]):
            per[k].append(c)
            k += 1
    for c in (8, 9, 10, 11, 13):
        for i in range(DEEP_DIST_COUNTS[c]):
            per[i].append(c)
    for i in range(DEEP_DIST_COUNTS[12]):     # distances 65..96: two per boundary
        per[i // 2].append(12)
    far = [14, 14, 15, 16]
    for i, c in enumerate(far):               # distances 129..: alone on their boundaries
        assert not per[nb - 1 - i]
        per[nb - 1 - i] = [c]
    # positions: targets go right from the boundary, sources left
    n = (nb + 1) * CHUNK
    buf = filler(rng, n)
    used = np.zeros(n, bool)
    plan = []
    for i, codes in enumerate(per):
        B = (i + 1) * CHUNK
        p, last_a = B, B + 5
        for c in sorted(codes):
            D = max(R.DBASE[c] + (40 if c >= 14 else 0), p - (last_a - 5))
            assert D < R.DBASE[c] + (1 << R.DEXT[c])
            a = p - D
            plan.append((a, p))
            used[a - 1:a + 5] = True
            used[p:p + 5] = True
            p, last_a = p + 5, a
    # period units (d literals, then a match of 4 at distance d, then a separator) in the gaps,
    # no 4-gram of a unit used twice
    todo = [d for d in (4, 3, 2, 1) for _ in range(DEEP_DIST_COUNTS[d - 1])]
    rng.shuffle(todo)
    grams = set()
    q = 8
    for d in todo:
        size = d + 4 + 1
        while used[q:q + size].any():
            q += 1
        assert q + size < n
        while True:
            unit = rng.choice(np.arange(128, 256) if d > 1 else np.arange(256), d, replace=False)
            body = (unit.astype(np.uint8).tobytes() * 8)[:d + 4]
            g = {body[i:i + 4] for i in range(d + 1)}
            if not g & grams:
                grams |= g
                break
        buf[q:q + d + 4] = body
        buf[q + d + 4] = int(rng.choice([v for v in range(128) if v != body[0]]))
        if d == 1 and buf[q - 1] == body[0]:
            buf[q - 1] = (body[0] + 1) % 128
        used[q:q + size] = True
        q += size
    for a, p in sorted(plan, key=lambda ap: (ap[1] // CHUNK, ap[1])):
        plant(buf, a, p, 4, rng)
    return bytes(buf)


@functools.lru_cache(maxsize=None)
def deep_code_length_block():
    """Literal counts in powers of two that add up, with the end-of-block code, to 2^14, so the
    lit/len code lengths are known: 129 of 9, 65 of 8, 33 of 7, 9 of 6, 3 of 5 and one each of
    10..13, two of 14.  Byte values are ordered so that no length stands more than twice in a row
    (no repeat symbol), and the code-length symbols' own Huffman tree is 8 deep."""
    rng = np.random.default_rng(600)
    others = [8] * 65 + [7] * 33 + [6] * 9 + [5] * 3 + [10, 11, 12, 13, 14]
    others = [others[i] for i in rng.permutation(len(others))]
    order = []
    for i, o in enumerate(others):
        order += [9, 9, o] if i < 129 - len(others) else [9, o]
    assert order.count(9) == 129 and len(order) == 244
    data = np.concatenate([np.full(1 << (14 - L), byte, np.uint8) for byte, L in enumerate(order)])
    assert len(data) == (1 << 14) - 1
    rng.shuffle(data)
    return data.tobytes()


def one_distance_code_block():
    """Matches at distance 1 only: runs of 200 different bytes (a run byte seen before would be
    found through the hash at a far distance)."""
    rng = np.random.default_rng(700)
    out = bytearray()
    for v in rng.permutation(256)[:200]:
        out += bytes([int(v)]) * int(rng.integers(5, 12)) + bytes((int(v) + 1 + int(x)) % 256 for x in rng.integers(0, 100, 3))
    return bytes(out)


def no_match_block():
    """A de Bruijn-like sequence over four symbols: no 4-gram twice and no three bytes equal to
    the three bytes 1..4 positions before them, so the probe finds no match at all; two bits a
    byte."""
    seq, seen = [0, 1, 2, 3], {(0, 1, 2, 3)}
    while True:
        for k in range(4):
            t = seq + [(seq[-1] + 1 + k) % 4]
            if tuple(t[-4:]) in seen:
                continue
            if any(len(t) >= d + 3 and t[-3:] == t[-3 - d:-d] for d in (1, 2, 3, 4)):
                continue
            seen.add(tuple(t[-4:]))
            seq = t
            break
        else:
            break
    return bytes(65 + s for s in seq)


def dist_code_counts(toks):
    f = [0] * 30
    for t in toks:
        if isinstance(t, tuple):
            f[R.dist_code(t[1])[0]] += 1
    return f


# ---- what the restatement says of every crafted block, and the coverage each exists for --------
@functools.lru_cache(maxsize=None)
def reference():
    """{group: [(label, block, tokens of deflate_ref.tokens)]}, computed once."""
    groups = {
        "length": [("ladder%d" % i, b) for i, (b, _) in enumerate(length_ladder())],
        "distance": [("d%d" % D, b) for b, D in distance_ladder()] + [("d32769", beyond_window_block())],
        "edges": [(label, b) for label, b, _ in edge_blocks()],
        "huffman": [("deep_distance", deep_distance_block()), ("deep_code_length", deep_code_length_block()),
                    ("one_distance_code", one_distance_code_block()), ("no_match", no_match_block())],
    }
    return {g: [(label, b, R.tokens(b)) for label, b in v] for g, v in groups.items()}


def matches(toks):
    return [t for t in toks if isinstance(t, tuple)]


@functools.lru_cache(maxsize=None)
def assert_coverage():
    """Every crafted block still exercises its case (on the restatement's tokens): an input that
    stopped doing so fails here instead of passing vacuously.  (Checked once per process; a
    failure is not cached.)"""
    ref = reference()
    for v in ref.values():
        for label, b, toks in v:
            assert R.detokenize(toks) == b, label
            assert all(3 <= L <= 258 and 1 <= D <= R.WINDOW for L, D in matches(toks)), label
    # lengths: every length 3..258, hence every length symbol and both ends of every range
    got = set()
    for (label, b, toks), (_, want) in zip(ref["length"], length_ladder()):
        ms = set(matches(toks))
        assert all(w in ms for w in want), (label, [w for w in want if w not in ms])
        got |= {L for L, _ in ms}
    assert got >= set(range(3, 259))
    assert {R.len_code(L)[0] for L in got} == set(range(257, 286))
    # distances: every distance symbol with extra value 0 and with its maximum
    seen = set()
    for (label, b, toks), (_, D) in zip(ref["distance"], distance_ladder()):
        assert any(d == D for _, d in matches(toks)), label
        seen |= {R.dist_code(d) for _, d in matches(toks)}
    for c in range(30):
        assert (c, R.DEXT[c], 0) in seen and (c, R.DEXT[c], (1 << R.DEXT[c]) - 1) in seen, c
    label, b, toks = ref["distance"][-1]
    assert label == "d32769" and all(d <= 32768 for _, d in matches(toks))
    assert not any(L == 9 for L, _ in matches(toks)), "the repeat one past the window was taken"
    # edges
    for (label, b, toks), (_, _, want) in zip(ref["edges"], edge_blocks()):
        if want:
            assert want in toks, label
            pos = 0
            for t in toks:
                if t == want:
                    break
                pos += t[0] if isinstance(t, tuple) else 1
            if label == "crosses_two_chunks":
                assert pos % CHUNK == 255 and pos // CHUNK + 2 == (pos + 258) // CHUNK
            if label == "ends_on_chunk_end":
                assert (pos + want[0]) % CHUNK == 0
            if label.startswith("ends_on_block_end"):
                assert pos + want[0] == len(b) and toks[-1] == want
    # Huffman extremes
    h = {label: toks for label, b, toks in ref["huffman"]}
    f = dist_code_counts(h["deep_distance"])
    assert sum(1 for x in f if x) >= 17 and R.huffman_depth(f) > 15
    assert R.cost(f, R.package_merge(f, 15)) > R.huffman_cost(f)
    assert not matches(h["deep_code_length"])
    f = dist_code_counts(h["one_distance_code"])
    assert sum(1 for x in f if x) == 1 and sum(f) >= 100
    assert not matches(h["no_match"]) and len(set(h["no_match"])) == 4
