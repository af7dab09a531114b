"""The crafted BAM field cases (tests/bam_field_cases.py) on the CPU: every case has the structure
it claims (which loop of k_decode_pools each tile of 64 takes, the unit-count boundary hit exactly,
every (segment, residue) cell and every hash length present), and the oracle reads exactly what the
builder wrote, so the device test (test_bam_fields_gpu.py) compares against references that agree
with each other and are independent: the builder's pieces and the oracle's decode."""
import numpy as np
import pytest

import bam_field_cases as B
from helpers import FIELDS, oracle_pools
from sam_ref import murmur_bytes

# k_decode_pools (csrc/hbam_kernels.hip), the tile's path, at "if (__ballot(big || R >= (1u << 16)) == 0ull)":
#   R += (L[f] + 15u) >> 4;  big |= L[f] >= (1u << 20);   with L = {nl, 4 nc, ls, ls, na} and all five 0
#   for a record whose layout_ok is 0.  The record-major path (pools_tile_rm) packs a record's
#   cumulative unit counts as cu[1] | cu[2] << 16 and cu[3] | cu[4] << 16.
UNIT_LIMIT = 1 << 16
FIELD_LIMIT = 1 << 20
TILE = 64


def tiles(case):
    """per tile of 64 records: dict(path, R list, T, first lane with units)"""
    out = []
    for t0 in range(0, len(case.recs), TILE):
        recs = case.recs[t0:t0 + TILE]
        R = [sum(r.units()) for r in recs]
        big = [any(n >= FIELD_LIMIT for n in r.field_lens()) for r in recs]
        fm = any(b or n >= UNIT_LIMIT for b, n in zip(big, R))
        first = next((i for i, n in enumerate(R) if n), None)
        out.append(dict(path="field" if fm else "record", R=R, big=big, T=sum(R), first=first, recs=recs))
    return out


def test_key_arithmetic():
    """java_key against hand-worked values of BAMRecordReader.getKey (Java int / long wrap)."""
    var = b"abc\0"
    h = murmur_bytes(var, 0) & 0xffffffff
    hk = (0x7fffffff << 32 | (h | 0xffffffff00000000 if h >> 31 else h)) & (1 << 64) - 1
    hk = hk - (1 << 64) if hk >> 63 else hk
    assert B.hash_key(var) == hk
    assert B.java_key(1, -1, 0, var) == -1                      # start 0: ref << 32 | (long)-1
    assert B.java_key(3, 0, 0, var) == 3 << 32
    assert B.java_key(2, 0x7ffffffe, 0, var) == (2 << 32 | 0x7ffffffe)
    assert B.java_key(1, -2, 0, var) == hk                      # start -1
    assert B.java_key(1, 0x7fffffff, 0, var) == hk              # start wraps to Integer.MIN_VALUE
    assert B.java_key(2, 100, 4, var) == hk and B.java_key(-1, 100, 0, var) == hk
    assert B.java_key(0, 5, 0x4d, b"") == B.hash_key(b"")


# ---- which loop each tile takes -------------------------------------------------------------------------------
def test_field_limit_is_implied_by_the_unit_limit():
    """A field of 2^20 bytes is 2^16 units, so no record can be over the field limit and under the
    unit limit: the smallest record that leaves the record-major path has exactly 2^16 units
    (field_major-three_empty holds one)."""
    assert (FIELD_LIMIT + 15) >> 4 == UNIT_LIMIT
    t = tiles(B.field_major("three_empty"))[0]
    assert t["R"][63] == UNIT_LIMIT and t["big"][63] and t["path"] == "field"


@pytest.mark.parametrize("case_id", ["length_grid", "key_edges", "murmur_lengths-tail0", "murmur_lengths-tail15"] +
                         ["prefixes-%d" % n for n in B.PREFIXES])
def test_small_cases_are_record_major(case_id):
    case = B.get(case_id)
    ts = tiles(case)
    assert all(t["path"] == "record" for t in ts)
    assert len(case.data) < 1 << 18


def test_prefix_tiles():
    assert [[len(t["recs"]) for t in tiles(B.prefixes(n))] for n in B.PREFIXES] == \
        [[1], [63], [64], [64, 1], [64, 64, 1]]
    assert all(t["T"] > 0 for n in B.PREFIXES for t in tiles(B.prefixes(n)))


@pytest.mark.parametrize("R,lane", B.UNIT_VARIANTS)
def test_unit_boundary_tiles(R, lane):
    case = B.unit_boundary(R, lane)
    (t,) = tiles(case)
    assert len(t["recs"]) == 64 and t["R"][lane] == R and case.notes["big"] == lane
    assert max(n for i, n in enumerate(t["R"]) if i != lane) < 64 and not any(t["big"])
    big = case.recs[lane]
    u = big.units()
    cu = [sum(u[:f]) for f in range(5)]
    assert len(big.name) == 16 and not big.cigar and not big.aux and big.l_seq == 16 * ((R - 1) // 2)
    if R == 65535:
        assert t["path"] == "record" and cu[4] == 0xffff and cu[3] == 1 + 32767 and max(cu) <= 0xffff
    else:
        assert t["path"] == "field" and cu[4] == 0x10001
    assert len(case.data) < 1 << 20


@pytest.mark.parametrize("which", B.FIELD_MAJOR_VARIANTS)
def test_field_major_tiles(which):
    case = B.field_major(which)
    t0, t1 = tiles(case)
    assert t0["path"] == "field" and t1["path"] == "record" and len(t1["recs"]) == 64
    over = [i for i, (b, n) in enumerate(zip(t0["big"], t0["R"])) if b or n >= UNIT_LIMIT]
    rest = [r for i, r in enumerate(t0["recs"]) if i not in over]
    if which == "one_aux":
        assert over == [17] and t0["big"][17] and len(t0["recs"][17].aux) == FIELD_LIMIT + 11
    elif which == "two_over":
        assert over == [5, 40]
        assert not t0["big"][5] and t0["R"][5] == 65537          # over by the unit count alone
        assert t0["big"][40] and len(t0["recs"][40].aux) >= FIELD_LIMIT
    else:
        assert over == [63] and t0["R"][63] == UNIT_LIMIT
        fu = [sum(r.units()[f] for r in t0["recs"]) for f in range(5)]
        assert fu[1] == fu[2] == fu[3] == 0 and fu[0] > 0 and fu[4] > 0    # three fields without units
    if which != "three_empty":
        # the field-major loop's partial stores and seq4 see the grid too
        ls = [len(r.qual) for r in rest]
        assert 0 in ls and any(n % 2 for n in ls) and any(n and n % 2 == 0 for n in ls)
        assert any(not r.cigar for r in rest) and any(not r.aux for r in rest) and any(not r.name for r in rest)
        assert {n % 16 for n in ls} == set(range(16))
    assert len(case.data) < 5 << 19


@pytest.mark.parametrize("which", B.EMPTY_VARIANTS)
def test_empty_tiles(which):
    case = B.empty_tiles(which)
    t0, t1 = tiles(case)
    assert t1["path"] == "record" and t1["T"] > 0 and t1["first"] == 0 and len(t1["recs"]) == 64
    if which == "no_units":
        assert t0["T"] == 0 and all(r.block_size == 32 and r.layout_ok for r in t0["recs"])
    elif which == "leading_empty":
        assert t0["first"] == 10 and all(r.block_size == 32 for r in t0["recs"][:10]) and t0["T"] > 0
    else:
        assert t0["T"] == 0 and not any(r.layout_ok for r in t0["recs"])
        assert all(r.block_size > 32 for r in t0["recs"])
        nc = sum(1 for r in t0["recs"] if r.n_cigar != len(r.cigar))
        assert nc == 16 and {r.l_seq for r in t0["recs"]} >= {-1, 0x7fffffff}
        # one byte too long: the claim's packed bytes are the pieces', its QUAL one byte more
        one = [r for r in t0["recs"] if r.l_seq == len(r.qual) + 1]
        assert len(one) == 16
        for r in one:
            need = len(r.name) + 4 * r.n_cigar + (r.l_seq + 1) // 2 + r.l_seq
            assert need == len(r.var) + 1
        assert sum(1 for r in t0["recs"] if r.flag & 4) == 32


# ---- coverage -------------------------------------------------------------------------------------------------
def test_length_grid_coverage():
    recs, what = B.grid_records()
    assert len(recs) == 52 + 14 + 50 + 50 + 50
    for seg, lens in B.GRID_LENGTHS.items():
        assert sorted(n for s, n in what if s == seg) == lens
    field = dict(name=lambda r: len(r.name), cigar=lambda r: 4 * len(r.cigar), seq=lambda r: len(r.qual),
                 qual=lambda r: len(r.qual), aux=lambda r: len(r.aux))
    for seg in B.GRID_SEGMENTS:
        mine = [field[seg](r) for r, (s, _) in zip(recs, what) if s == seg]
        # a CIGAR is whole words: its residues are the multiples of 4
        want = set(range(0, 16, 4)) if seg == "cigar" else set(range(16))
        assert {n % 16 for n in mine if n < 16} == want, seg
        assert {n % 16 for n in mine if n >= 16} == want, seg
    # SEQ: the last unit's character count n = l_seq mod 16 fixes its own parity (the slide-back
    # store runs for even n only); of the packed bytes every residue mod 8 occurs with an odd and an
    # even l_seq, below 16 bases and from 16 on
    ls = [len(r.qual) for r, (s, _) in zip(recs, what) if s == "seq"]
    for lo, hi in ((0, 16), (16, 50)):
        assert {(((n + 1) // 2) % 8, n % 2) for n in ls if lo <= n < hi} == {(p, q) for p in range(8) for q in (0, 1)}
    assert all(r.layout_ok and not (r.flag & 4) and r.ref >= 0 and r.pos >= 0 for r in recs)
    assert any(len(r.name) == 0 for r in recs)
    # neighbouring lanes differ
    assert sum(1 for a, b in zip(what, what[1:]) if a[0] != b[0]) > len(what) // 2


def test_length_grid_bytes():
    """SEQ uses all 16 nibble values in both positions, QUAL and aux hold bytes >= 0x80"""
    recs, _ = B.grid_records()
    seq = np.frombuffer(b"".join(r.seq for r in recs), np.uint8)
    assert set(seq >> 4) == set(range(16)) and set(seq & 15) == set(range(16))
    assert max(b"".join(r.qual for r in recs)) >= 0x80 and max(b"".join(r.aux for r in recs)) >= 0x80
    e = B.length_grid().expect
    assert set(e["seq"].tolist()) == set(B.SEQ_ALPHA.encode())
    # the expectation's SEQ, written out plainly for one record
    r = next(r for r in recs if len(r.qual) == 49)
    plain = "".join(B.SEQ_ALPHA[(r.seq[i // 2] >> 4) if i % 2 == 0 else (r.seq[i // 2] & 15)] for i in range(49))
    assert bytes(r.bases()) == plain.encode()


@pytest.mark.parametrize("tail", [0, 15])
def test_murmur_lengths_coverage(tail):
    case = B.murmur_lengths(tail)
    lens = [len(r.var) for r in case.recs]
    assert sorted(lens) == list(range(288)) and B.MURMUR_MAX == 287
    assert lens[-1] == 16 * 17 + tail and case.u.endswith(case.recs[-1].bytes)
    assert all((r.flag & 4) and r.ref == -1 and r.layout_ok for r in case.recs)
    assert all(r.key == B.hash_key(r.var) for r in case.recs)
    assert {(n // 16, n % 16) for n in lens} == {(b, t) for b in range(18) for t in range(16)}
    assert len({r.key for r in case.recs}) == 288
    # both signs of the hash: a negative one's sign extension covers the key's upper word
    assert {r.key >> 32 for r in case.recs} == {0x7fffffff, -1}
    assert next(r for r in case.recs if not r.var).block_size == 32


def test_key_edges_spelled_out():
    case = B.key_edges()
    e = case.notes["edges"]
    assert len(e) == 9
    for label, (i, want) in e.items():
        r = case.recs[i]
        assert r.key == want == B.java_key(r.ref, r.pos, r.flag, r.var), label
    rec = lambda label: case.recs[e[label][0]]
    assert e["pos_m1"][1] == -1 and rec("pos_m1").pos == -1 and not rec("pos_m1").flag & 4
    assert e["pos_max_m1"][1] == 0x27ffffffe and e["last_ref"][1] == 3 << 32 | 77777
    for label in ("pos_m2", "pos_max", "flag4_placed", "mapped_unplaced", "twin_a", "twin_b"):
        # Integer.MAX_VALUE << 32 | (long)hash: a negative hash's sign extension fills the upper word
        h = B._i32(murmur_bytes(rec(label).var, 0))
        assert e[label][1] == (0x7fffffff << 32 | h if h >= 0 else h), label
    assert (rec("pos_m2").pos, rec("pos_max").pos, rec("pos_max_m1").pos) == (-2, 0x7fffffff, 0x7ffffffe)
    assert rec("flag4_placed").flag & 4 and (rec("flag4_placed").ref, rec("flag4_placed").pos) == (2, 100)
    assert not rec("mapped_unplaced").flag & 4 and (rec("mapped_unplaced").ref, rec("mapped_unplaced").pos) == (-1, 100)
    a, b = rec("twin_a"), rec("twin_b")
    assert a.var == b.var and a.bytes[4:36] != b.bytes[4:36] and a.key == b.key
    # among ordinary records
    edge_idx = {i for i, _ in e.values()}
    assert all(i - 1 not in edge_idx and i + 1 not in edge_idx and 0 < i < len(case.recs) - 1 for i in edge_idx)


# ---- the oracle reads what the builder wrote ------------------------------------------------------------------
@pytest.mark.parametrize("case_id", B.ALL_IDS)
def test_oracle_agrees_with_the_builder(oracle_mod, case_id):
    case = B.get(case_id)
    e = case.expect
    ref = oracle_mod.read_split(case.data, case.v_start, case.v_end)
    assert (ref["n"], ref["status"]) == (len(case.recs), 0)
    for k in FIELDS[2:]:
        assert np.array_equal(ref[k], e[k]), k
    assert np.array_equal(ref["key"], e["key"])
    assert bytes(ref["var"]) == b"".join(r.var for r in case.recs)
    op = oracle_pools(ref)
    assert np.array_equal(op["layout_ok"], e["layout_ok"])
    for k, dt in B.POOLS:
        assert op[k].dtype == e[k].dtype == dt and np.array_equal(op[k], e[k]), k
    # the offset columns are the running sums of the pieces
    assert int(e["name_off"][-1]) == len(e["names"]) and int(e["cigar_off"][-1]) == len(e["cigars"])
    assert int(e["seq_off"][-1]) == len(e["seq"]) == len(e["qual"]) and int(e["aux_off"][-1]) == len(e["aux"])
    # the first record's voffset is where the case says the split starts
    assert int(ref["voffset"][0]) == case.v_start
