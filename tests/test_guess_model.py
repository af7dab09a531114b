"""The crafted guess windows (tests/guess_cases.py) on the CPU: every case has the structure it claims
(describe(): bytes, zlib and numpy only) and the oracle's outcome class it names, and the catalogue
is not degenerate.  test_guess_gpu.py runs the same guesses on the device."""
import collections

import pytest

import guess_cases as GC
import guess_craft as gc

CASES = GC.cases()
IDS = [repr(c) for c in CASES]


def outcome(case, g, res):
    """the oracle's (out, err) as the catalogue's outcome class"""
    out, err = res
    if err:
        return err
    return "end" if out == g["end"] else "rec"


@pytest.fixture(scope="module")
def oracle_results(oracle_mod):
    return {(repr(c), i): oracle_mod.guess_bam_record_start(c.np(), g["beg"], g["end"], c.n_ref)
            for c in CASES for i, g in enumerate(c.guesses)}


def test_catalogue_size():
    assert len(GC.guesses()) <= 150
    assert all(len(c.data) <= 300 << 10 for c in CASES)
    assert set(c.family for c in CASES) == set(GC.FAMILIES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_structure(case):
    for g in case.guesses:
        d = gc.describe(case.data, g["beg"], g["end"], case.n_ref)
        assert d["cached"] == g["cached"], (g, d)
        assert d["listed"] == g["listed"], (g, d)
        if g["n_window"] is not None:
            assert d["n_window"] == g["n_window"], (g, d)
        if g["n_first"] is not None:
            assert d["n_first"] == g["n_first"], (g, d)
        if g["listed"]:
            assert g["end"] - g["beg"] > 0xffff and len(case.data) - g["beg"] >= 65539
    if case.block is not None:
        g = case.guesses[0]
        d = gc.describe(case.data, g["beg"], g["end"], case.n_ref, block=case.block, up=case.up,
                        chain_from=case.chain_from)
        assert (d["accepted"][0] if d["accepted"] else None) == case.accepted0, d["accepted"][:8]
        if case.n_accepted is not None:
            assert len(d["accepted"]) == case.n_accepted
        if case.chain is not None:
            op, n = case.chain
            assert (d["chain"] > n) if op == ">" else (d["chain"] <= n), d["chain"]


def test_capacities_from_both_sides():
    """both sides of 256, 512 and 65539, and of 1024 through the G cases' chains"""
    D = [(c, g, gc.describe(c.data, g["beg"], g["end"])) for c, g in GC.guesses()]
    nw = set(d["n_window"] for _, _, d in D)
    assert {255, 256, 257, 600} <= nw
    nf = set(d["n_first"] for c, _, d in D if c.family == "B")
    assert nf == {511, 512, 513}
    assert all(not d["cached"] for c, _, d in D if c.family == "B")
    av = set(min(len(c.data) - g["beg"], g["end"] - g["beg"]) for c, g, _ in D if c.family == "C")
    assert {65538, 65539} <= av
    assert {d["listed"] for c, _, d in D if c.family == "D"} == {True, False}
    for fam in "EG":
        assert {d["cached"] for c, _, d in D if c.family == fam} == {True, False}
    # a chain that joins the remembered one behind its 1024th start: 1700 starts in one member
    long = next(c for c in CASES if c.name == "join")
    assert gc.chain_starts(long.data, long.block, 0) == 1700


def test_d_cut_reads():
    """The scan of the cut windows, restated: every guess ends in a short read whose buf keeps
    bytes of the read before; in exactly one phase a full read is aa aa aa 04 (it ends in
    04) and the next read starts one byte before the magic."""
    ends_in_04 = []
    for c in [c for c in CASES if c.name.startswith("cut/")]:
        hit = set()
        for k, g in zip((1, 2, 3), c.guesses):
            w = c.data[g["beg"]:g["end"]]
            m = c.magic_at - g["beg"]
            assert len(w) == m + k
            reads = gc.scan_reads(w, 0, gc.describe(c.data, g["beg"], g["end"])["first_end"])
            # the last read is short, and buf behind its bytes is what the read before left there
            (q, n, buf), before = reads[-1], reads[-2]
            assert n < 4 and q + n == len(w) and buf[n:] == before[2][n:], reads[-3:]
            full04 = [i for i, r in enumerate(reads) if r[1] == 4 and r[2] == b"\xaa\xaa\xaa\x04"]
            hit.add(bool(full04) and reads[full04[0] + 1][0] == m - 1)
        assert len(hit) == 1
        ends_in_04.append(hit.pop())
    assert sorted(ends_in_04) == [False, False, True]


def test_f_accepted_offsets():
    """the edge of every field of guessNextBAMPos' test, as the Python statement of it sees it"""
    by = {c.name: c for c in CASES if c.family == "F"}
    assert by["last40"].accepted0 == 200 and by["last39"].accepted0 is None
    assert [by["lane%d" % k].accepted0 for k in (63, 64, 65)] == [63, 64, 65]
    for name, accept, _ in GC.F_PROBES:
        assert (by[name].accepted0 == 0) == accept, name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_outcome(case, oracle_results):
    for i, g in enumerate(case.guesses):
        res = oracle_results[(repr(case), i)]
        assert outcome(case, g, res) == g["out"], (g, res)
        if g["out"] == "rec":
            v = res[0]
            assert v in case.starts, (g, hex(v))
            assert gc.walks_to_block_end(case.data, v)
            if g["at"] is not None:
                assert v >> 16 == g["at"], (g, v >> 16)
            if g["uoff"] is not None:
                assert v & 0xffff == g["uoff"], (g, v & 0xffff)


def test_non_degenerate(oracle_results):
    fam = collections.defaultdict(collections.Counter)
    for c in CASES:
        for i, g in enumerate(c.guesses):
            fam[c.family][outcome(c, g, oracle_results[(repr(c), i)])] += 1
    for f in GC.FAMILIES:
        assert fam[f]["rec"] >= 1, f
    total = sum(sum(v.values()) for v in fam.values())
    assert 3 * sum(v["end"] for v in fam.values()) <= total
    e = fam["E"]
    assert e["rec"] and e["end"] and any(isinstance(k, int) for k in e)
    # family E per damage kind: the outcomes the catalogue's table names are all there are
    where = {k: (0, 1, 2) for k in GC.E_KINDS}
    where.update({k: (w,) for k, w in GC.E_EXTRA})
    for kind, ws in where.items():
        seen = set(outcome(c, c.guesses[0], oracle_results[(repr(c), 0)])
                   for c in CASES if c.family == "E" and c.name.startswith(kind + "@"))
        assert seen == set(GC.E_OUTCOME[kind][w][0] for w in ws), (kind, seen)
    # BSIZE + 1 < 26 with a non-negative ISIZE escapes (EDATA); with a negative one it is skipped
    assert [o for o, _ in GC.E_OUTCOME["bsize_small"][1:]] == [GC.EDATA, GC.EDATA]
    assert GC.E_OUTCOME["bsize_neg"][1][0] == "rec"
