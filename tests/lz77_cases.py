"""The crafted token blocks of the LZ77 resolve pass (k_resolve_units): every case says what it is
there for, and `check` asserts on the model's report (lz77_craft.model) that it gets there, so a
case that stops reaching its path fails instead of passing vacuously.

cases() -> {name: Case}.  A Case has blocks (name, tokens, literal_code), the leads (output offsets
mod 16 of the members when they run through the inflater) and check(reports, a0), reports being
[(stretches, seen)] per block as model() returns them.  Literals come from fixed seeds; sizes are
the smallest that reach the path."""
import functools
import random

from lz77_craft import RS_S, Block

ALL16 = tuple(range(16))
SOME = (1, 5, 10, 15)


class Case:
    def __init__(self, blocks, leads, check, direct_only=False):
        self.blocks = [b if len(b) == 3 else b + (False,) for b in blocks]
        self.leads, self.check, self.direct_only = leads, check, direct_only


def _up(x):
    return -(-x // RS_S) * RS_S


# ---- unit_grid: every ru_put mask and ru_rd16 shift pair ----------------------------------------
GRID_LENS = list(range(3, 19)) + [33, 34]  # units of 3..16 bytes, last units of 1 and 2
GRID = [(n, dd, o) for dd in range(4) for o in range(4) for n in GRID_LENS]


def unit_grid():
    """One block, the grid (length x distance 16..19 x destination 0..3 mod 4) three times:
    dense (more than 64 ordered units a stretch: the bitmap scheduler's ru_put), with 32 literals
    between matches (at most 64: the index scheduler's ru_put5), and at distance 272..275 in the
    first bytes of a stretch (pre units read through the LDS window)."""
    b = Block(101)
    b.lit(24)
    i = 0
    while i < len(GRID) or b.op % RS_S < RS_S - 64:  # go on to the stretch's end: it stays dense
        n, dd, o = GRID[i % len(GRID)]
        b.lit((o - b.op) % 4).m(n, 16 + dd)
        i += 1
    b.to(_up(b.op))
    for n, dd, o in GRID:
        b.lit(32 + (o - b.op) % 4)
        if b.op % RS_S < 24:  # its source would end before the stretch: a pre unit
            b.lit(24)
        b.m(n, 16 + dd)
    todo = list(GRID)
    while todo:
        s0 = _up(b.op)
        b.to(s0)
        while todo and b.op - s0 < 190:
            n, dd, o = todo.pop()
            b.lit((o - b.op) % 4).m(n, 272 + dd)

    def check(reports, a0):
        (stretches, seen), = reports
        want = {(o, n, sh) for o in range(4) for n in range(1, 17) for sh in range(4)}
        for path in ("pre", "index", "bitmap"):
            got = {x[1:] for x in seen["put"] if x[0] == path}
            assert got >= want, (path, sorted(want - got)[:8])
        assert seen["rules"] == {"plain"}

    return Case([("grid", b.toks)], ALL16, check)


# ---- ladder: every length at every distance that changes a rule or a source path ----------------
LADDER_DISTS = (list(range(1, 41)) + list(range(255, 260)) + [511, 512, 513, 527, 528] +
                [1023, 1024, 1025] + [32767, 32768])


def ladder():
    """Every length 3..258 at each distance of LADDER_DISTS, len % 4 literals between matches,
    in blocks of at most 60000 bytes with filler in front that makes the distance legal: all three
    cutting rules, periodic heads of every distance 1..7, heads of every distance 8..15, far
    sources in the stretch written back one iteration earlier and far sources much older."""
    blocks, b = [], None
    for d in LADDER_DISTS:
        for n in range(3, 259):
            if b is None or max(b.op, d) + n % 4 + n > 60000:
                b = Block(200 + len(blocks), bytes(range(97, 113)))
                blocks.append(b)
            if b.op < d:
                b.lit(d - b.op)
            b.lit(n % 4).m(n, d)
    assert all(b.op <= 60000 for b in blocks)

    def check(reports, a0):
        rules, per, mid, prev, old = set(), set(), set(), 0, 0
        for stretches, seen in reports:
            rules |= seen["rules"]
            per |= seen["per"]
            mid |= seen["mid"]
            prev += seen["far_prev"]
            old += seen["far_old"]
        assert rules == {"plain", "periodic", "mid"}
        assert per == set(range(1, 8)) and mid == set(range(8, 16))
        assert prev >= 100 and old >= 100, (prev, old)

    return Case([("ladder%d" % i, b.toks) for i, b in enumerate(blocks)], SOME, check)


# ---- stretch_edges ------------------------------------------------------------------------------
def stretch_edges():
    """Matches of 258 and of 3 bytes starting at s0 + 1021 / 1022 / 1023 (the descriptor straddles
    the stretch boundary), the next stretch's first match reading the spill at distance 1, 9, 16 and
    from the spill's first byte; a match that ends exactly at isize; a match at offset 1 with
    distance 1; blocks of 1, 2, 3 (literals) and 1023, 1024, 1025 bytes."""
    b = Block(301)
    b.lit(RS_S)
    edges = []
    for n in (258, 3):
        for off in (1021, 1022, 1023):
            for d2 in (1, 9, 16, "first"):
                spill = off + n - RS_S
                if d2 == "first" and spill <= 0:
                    continue
                s0 = _up(b.op)
                b.to(s0 + off).m(n, 300)
                edges.append((s0 // RS_S, off + (n - 1) // 16 * 16))
                b.m(20, spill if d2 == "first" else d2)
    b.lit(5).m(30, 11)  # ends at isize
    blocks = [("edges", b.toks)]
    o1 = Block(302).lit(1).m(258, 1).lit(3).m(3, 1).lit(2)
    blocks.append(("offset1", o1.toks))
    for isize in (1, 2, 3):
        blocks.append(("lit%d" % isize, Block(310 + isize).lit(isize).toks))
    for isize in (1023, 1024, 1025):
        blocks.append(("size%d" % isize, Block(320).lit(100).m(258, 50).to(isize - 20).m(20, 7).toks))

    def check(reports, a0):
        stretches, seen = reports[0]
        for k, rel in edges:
            assert stretches[k]["maxrel"] == rel, (k, rel, stretches[k])
            assert stretches[k + 1]["nord"] >= 1  # the match that reads the spill waits for nothing final
        assert {rel for _, rel in edges} >= {1021, 1022, 1023, 1021 + 256, 1022 + 256, 1023 + 256}
        assert reports[1][1]["per"] == {1}
        for r in reports[2:5]:
            assert all(s["starts"] == 0 for s in r[0])

    return Case(blocks, ALL16, check)


# ---- counts: exact numbers of units and match starts in one stretch ----------------------------------
ORD_COUNTS = (63, 64, 65, 128)
PRE_COUNTS = (63, 64, 65, 127, 128, 129, 200)
START_COUNTS = (64, 65, 128, 129, 342)


def counts():
    """Exactly N ordered units (the 64-unit threshold between the two schedulers), exactly N pre
    units (the two-units-per-lane loop: 64 and 128 are its step edges; sources alternate between
    the LDS window and global memory), exactly N match starts (s_pos, the scans) in one stretch."""
    blocks, want = [], []
    for n in ORD_COUNTS:
        b = Block(400 + n).lit(RS_S)
        for _ in range(n):
            b.lit(1).m(3, 1)
        b.lit(8)
        blocks.append(("ord%d" % n, b.toks))
        want.append((1, dict(nord=n, npre=0, starts=n, sched="index" if n <= 64 else "bitmap")))
    for n in PRE_COUNTS:
        b = Block(500 + n).lit(2 * RS_S)
        for i in range(n):
            b.m(3, 400 if i % 2 and b.op - 2 * RS_S < 390 else 1100)
        b.lit(8)
        blocks.append(("pre%d" % n, b.toks))
        want.append((2, dict(nord=0, npre=n, starts=n, sched="none")))
    for n in START_COUNTS:
        b = Block(600 + n).lit(2 * RS_S)
        if n == 342:
            for i in range(341):
                b.m(3, 1100 if i % 2 == 0 else 1)
            b.m(3, 1)
            want.append((2, dict(starts=342, npre=171, nord=171)))
        else:
            for i in range(n):
                b.m(3, 1100) if i % 2 == 0 else b.m(4, 2)
            b.lit(8)
            want.append((2, dict(starts=n, npre=(n + 1) // 2, nord=n // 2)))
        blocks.append(("starts%d" % n, b.toks))

    def check(reports, a0):
        for (stretches, seen), (k, w), blk in zip(reports, want, blocks):
            for key, v in w.items():
                assert stretches[k][key] == v, (blk[0], key, stretches[k])
            for j, s in enumerate(stretches):
                assert j == k or s["starts"] == 0
        far = [r[0][2]["far"] for r in reports[len(ORD_COUNTS):len(ORD_COUNTS) + len(PRE_COUNTS)]]
        if a0 == 0:  # both source paths in one step of the pre loop
            assert all(0 < f < n for f, n in zip(far, PRE_COUNTS)), far

    return Case(blocks, SOME, check)


# ---- capacity -----------------------------------------------------------------------------------
def capacity():
    """341 matches of 3 bytes from s0 and a 258-byte match at s0 + 1023: 342 match starts and
    358 units, the most a stretch can hold (RU_CAP 360): all ordered at distance 1 (one unit a
    round, the longest chain), all pre, and mixed (the pre list from the front meets the ordered
    list from the back); and a whole 65536-byte block of (3, 1) matches."""
    chain = Block(701).lit(RS_S)
    for _ in range(341):
        chain.m(3, 1)
    chain.m(258, 1).lit(4)
    pre = Block(702).lit(2 * RS_S)
    for _ in range(341):
        pre.m(3, 1300)
    pre.m(258, 1300).lit(4)
    mixed = Block(703).lit(2 * RS_S)
    for i in range(341):
        mixed.m(3, 1300 if i % 2 == 0 else 1)
    mixed.m(258, 1).lit(4)
    whole = Block(704).lit(1)
    for _ in range(21845):
        whole.m(3, 1)
    assert whole.op == 65536

    def check(reports, a0):
        c, p, m, w = (r[0] for r in reports)
        assert (c[1]["starts"], c[1]["npre"], c[1]["nord"], c[1]["rounds"], c[1]["sched"]) == (342, 0, 358, 358, "bitmap")
        assert (p[2]["starts"], p[2]["npre"], p[2]["nord"]) == (342, 358, 0)
        assert (m[2]["starts"], m[2]["npre"], m[2]["nord"]) == (342, 171, 187)
        assert len(w) >= 64 and all(s["rounds"] == s["nord"] >= 341 for s in w[:64])

    return Case([("chain", chain.toks), ("pre", pre.toks), ("mixed", mixed.toks), ("whole", whole.toks)],
                SOME, check)


# ---- rounds: the two schedulers on units that are not one chain ---------------------------------------
def _groups(b, k):
    for _ in range(k):
        b.lit(2).m(3, 1).m(3, 1).m(4, 5)      # (4, 5): its source spans both matches before it
        b.lit(1).m(9, 2).m(20, 3).m(12, 9)    # periodic heads, an 8..15 head, each on the one before
        b.lit(1).m(6, 12)                     # a plain unit over two earlier destinations


def rounds():
    """Stretches whose ordered units form independent groups that become ready in the same round:
    a unit whose source spans two earlier units' destinations, one whose source begins before s0
    and ends inside the stretch on a unit it waits for, periodic heads among them; with more than
    64 units (the pending-byte bitmap) and with at most 64 (unit-index ranges)."""
    blocks = []
    for name, k in (("bitmap", 12), ("bitmap_full", 16), ("index", 5), ("index64", 6)):
        b = Block(800 + k).lit(RS_S)
        b.m(3, 1).m(8, 8)  # (8, 8) at s0 + 3: source [s0 - 5, s0 + 3)
        _groups(b, k)
        if name == "index64":
            for _ in range(8):  # 2 + 6 * 9 + 8: exactly 64
                b.lit(1).m(3, 1)
        b.lit(8)
        blocks.append((name, b.toks))

    def check(reports, a0):
        for (stretches, seen), blk in zip(reports, blocks):
            s = stretches[1]
            assert s["sched"] == ("bitmap" if blk[0].startswith("bitmap") else "index"), (blk[0], s)
            assert 2 < s["rounds"] and 3 * s["rounds"] < s["nord"], s  # several units a round
            assert s["maxdeps"] >= 2 and s["straddle"] >= 1, s
            assert seen["per"] >= {1, 2, 3} and seen["mid"] == {9}
        assert reports[3][0][1]["nord"] == 64 and reports[1][0][1]["nord"] > 128

    return Case(blocks, SOME, check)


# ---- max_block --------------------------------------------------------------------------------------
def max_block():
    """ISIZE 65536 (65 stretches behind a lead of 15): a 258-byte match at distance 32768 that
    starts at offset 32768, a match that ends on the last byte; an all-literal block of 65536
    bytes, which the pass leaves on its early return."""
    b = Block(901, bytes(range(256))).lit(32768).m(258, 32768).lit(2)
    ds = [32768, 1, 9, 600, 1024, 16, 5000, 3]
    for i in range(126):
        b.m(258, ds[i % len(ds)])
    assert b.op == 65536
    lit = Block(902).lit(65536)

    def check(reports, a0):
        stretches, seen = reports[0]
        assert len(stretches) == (65 if a0 else 64)
        assert stretches[32]["starts"] >= 1 and seen["far_old"] > 0
        assert all(s["starts"] == 0 for s in reports[1][0])

    return Case([("far", b.toks), ("literals", lit.toks, True)], (15,), check)


# ---- tails ------------------------------------------------------------------------------------------
def tails():
    """Valid tail tokens (a final match of 1 or 2 bytes) at distance 1, 2, greater than n, and from
    a source older than the LDS window; in the last stretch after an ordered match the tail
    copies from, and in blocks with no other match, down to ISIZE 2."""
    blocks = []
    for n, d in ((1, 1), (2, 1), (2, 2), (1, 5), (2, 5)):
        blocks.append(("after_match_%d_%d" % (n, d), Block(1000).lit(RS_S + 30).m(18, 4).toks + [(n, d)]))
    for n in (1, 2):
        for d in (1, 2, 7, 1500):  # 1500 from 2000: source 500, window of stretch 1 begins at 512
            blocks.append(("alone_%d_%d" % (n, d), Block(1001).lit(2000).toks + [(n, d)]))
    blocks.append(("isize2", Block(1002).lit(1).toks + [(1, 1)]))
    blocks.append(("isize3_2_1", Block(1003).lit(1).toks + [(2, 1)]))
    blocks.append(("isize3_1_2", Block(1004).lit(2).toks + [(1, 2)]))
    blocks.append(("isize3_1_1", Block(1005).lit(2).toks + [(1, 1)]))

    def check(reports, a0):
        assert all(r[0][-1]["nord"] == 2 for r in reports[:5])
        assert all(s["starts"] == 0 for r in reports[5:] for s in r[0])

    return Case(blocks, (5, 15), check, direct_only=True)


@functools.lru_cache(None)
def cases():
    return {f.__name__: f() for f in (unit_grid, ladder, stretch_edges, counts, capacity, rounds, max_block, tails)}


# ---- neighbours -------------------------------------------------------------------------------------
@functools.lru_cache(None)
def neighbours():
    """Small members packed back to back, alternating an all-literal member of random bytes (ISIZE
    1..33, which the pass leaves untouched) and a member of one literal and a distance-1 match to its
    end (ISIZE 4..40), the sizes chosen so that match members start and end at every residue mod 16.
    -> [(tokens, start offset)], the match members at the odd indices."""
    rng = random.Random(77)
    out, pos = [], 0
    pairs = [(s, e) for s in range(16) for e in range(16)]
    rng.shuffle(pairs)
    for i, (s, e) in enumerate(pairs):
        nl = (s - pos) % 16 or 16
        nl += 16 if i % 3 == 0 else 0
        out.append(([rng.randrange(256) for _ in range(nl)], pos))
        pos += nl
        sizes = [m for m in range(4, 41) if (s + m) % 16 == e]
        m = sizes[i % len(sizes)]
        out.append(([rng.randrange(256), (m - 1, 1)], pos))
        pos += m
    out.append(([rng.randrange(256) for _ in range(21)], pos))
    return out
