"""The crafted merge-correction cases (tests/merge_cases.py) on the CPU: the oracle's
correct_payloads and rewrite_group_tags return, or raise, exactly what each case declares; the cases
reach every branch they are there for (computed from the case data); and a dozen single records with
hand-written bytes pin the oracle to something other than the case builder.  test_merge_gpu.py then
holds hbam_merge_remap and hbam_rewrite_groups to the oracle."""
import struct

import numpy as np
import pytest

import f4_records as F
import merge_cases as M

REMAP = M.cached(M.remap_cases)
GROUP = M.cached(M.group_cases)
PRODUCT = M.cached(M.product_cases)


def by_id(cases, cid):
    return next(c for c in cases if c.id == cid)


# ---- the oracle does what the cases declare -----------------------------------------------------------------
def check_remap(o, case):
    pay, off = F.pack(case.recs)
    got_pay, got_keys, bad = o.correct_payloads(pay, off, case.keys, case.ref_map)
    n = case.n_expected
    assert bad == case.bad, case.id
    assert n == (len(case.recs) if bad < 0 else bad)
    assert bytes(got_pay[:int(off[n])]) == b"".join(case.out_recs), case.id
    assert bytes(got_pay[int(off[n]):]) == bytes(pay[int(off[n]):]), case.id  # the oracle stops there
    assert got_keys[:n].tolist() == case.out_keys and got_keys[n:].tolist() == case.keys[n:].tolist(), case.id


@pytest.mark.parametrize("cid", [c.id for c in REMAP])
def test_remap_oracle(oracle_mod, cid):
    check_remap(oracle_mod, by_id(REMAP, cid))


@pytest.mark.parametrize("name", list(M.MAPS))
def test_remap_refused_oracle(oracle_mod, name):
    cases = M.remap_refused(name)
    assert len(cases) > 20
    for case in cases:
        assert 0 <= case.bad == len(case.recs) - 2
        check_remap(oracle_mod, case)


def test_remap_int_max_position_wraps(oracle_mod):
    """pos + 1 at Integer.MAX_VALUE wraps below zero: the key stays, nothing raises"""
    case = M.RemapCase("max", [(0, -1, 0, M.I32_MAX), (0, -1, 0, M.I32_MAX - 1)], [1, 1])
    assert case.out_keys == [M.sentinel(0), (1 << 32) | (M.I32_MAX - 1)]
    check_remap(oracle_mod, case)


def run_groups(o, case):
    pay, off = F.pack(case.inputs())
    return o.rewrite_group_tags(pay, off.astype(np.int64), case.groups, case.inp)


def check_groups(o, case):
    want = case.outputs()
    if case.err is None:
        pay, off = run_groups(o, case)
        assert bytes(pay) == b"".join(want), case.id
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want])]).tolist()
    else:
        with pytest.raises(o.GroupRewriteError) as ei:
            run_groups(o, case)
        assert (ei.value.kind, ei.value.record) == case.err, case.id
        # the records before it stand
        head = M.GroupCase(case.id, case.recs[:case.err[1]], case.pg, case.rg)
        pay, off = run_groups(o, head)
        assert bytes(pay) == b"".join(want), case.id


@pytest.mark.parametrize("cid", [c.id for c in GROUP])
def test_groups_oracle(oracle_mod, cid):
    case = by_id(GROUP, cid)
    if not case.noop:  # what is declared per record agrees with what is declared for the case
        first = next(((r.error, i) for i, r in enumerate(case.recs) if r.error), None)
        assert first == case.err
    check_groups(oracle_mod, case)


@pytest.mark.parametrize("cid", [c.id for c in PRODUCT])
def test_product_oracle(oracle_mod, cid):
    """sort_merged's order: correct_payloads, then rewrite_group_tags over the records before the
    refused one"""
    o, case = oracle_mod, by_id(PRODUCT, cid)
    pay, off = F.pack(case.inputs())
    pay, keys, bad = o.correct_payloads(pay, off, case.keys, case.ref_map)
    assert bad == case.bad
    n = len(case.recs) if bad < 0 else bad
    assert keys[:n].tolist() == case.out_keys
    off = off.astype(np.int64)[:n + 1]
    if case.err is None:
        got, _ = o.rewrite_group_tags(pay, off, case.groups.groups, case.groups.inp)
        assert bytes(got) == b"".join(case.out_recs)
    else:
        with pytest.raises(o.GroupRewriteError) as ei:
            o.rewrite_group_tags(pay, off, case.groups.groups, case.groups.inp)
        assert (ei.value.kind, ei.value.record) == case.err
        got, _ = o.rewrite_group_tags(pay, off[:case.err[1] + 1], case.groups.groups, case.groups.inp)
        assert bytes(got) == b"".join(case.out_recs)


# ---- the cases reach the branches they are there for ----------------------------------------------------------
def test_remap_cases_exercise_the_rules():
    up = by_id(REMAP, "grid-up")
    n_in = 4
    edge = {-1, 0, n_in - 1, n_in, n_in + 5, -2, M.I32_MIN, M.I32_MAX}
    refused = [c.fields[c.bad] for c in M.remap_refused("up")]
    seen = up.fields + refused
    for paired in (0, 1):
        for unmapped in (0, 4):
            mine = [f for f in seen if f[2] & 1 == paired and f[2] & 4 == unmapped]
            assert {(f[0], f[1]) for f in mine} >= {(a, b) for a in edge for b in edge}
    # the unpaired read whose mate refID is out of range is not refused and keeps bytes 24..27
    stale = [i for i, f in enumerate(up.fields) if not f[2] & 1 and (f[1] >= n_in or f[1] < -1)]
    assert {up.fields[i][1] for i in stale} == {n_in, n_in + 5, -2, M.I32_MIN, M.I32_MAX}
    assert all(up.out_fields[i][1] == up.fields[i][1] and up.out_recs[i][24:28] == up.recs[i][24:28] for i in stale)
    # every refused combination is refused for a paired mate or for the refID itself
    assert all(M.RemapCase._moved(up, f[0]) is None or (f[2] & 1 and M.RemapCase._moved(up, f[1]) is None) for f in refused)
    # the key at every position, for a record whose refID moves, mapped and unmapped
    for pos, key in ((-2, None), (-1, -1), (0, 1 << 32), (M.I32_MAX, None)):
        i = next(i for i, f in enumerate(up.fields) if f[0] == 0 and f[3] == pos and not f[2] & 4)
        assert up.out_fields[i][0] == 1 and up.out_keys[i] == (M.sentinel(i) if key is None else key)
        j = next(i for i, f in enumerate(up.fields) if f[0] == 0 and f[3] == pos and f[2] & 4)
        assert up.out_fields[j][0] == 1 and up.out_keys[j] == M.sentinel(j)
    # an index that stays: its key stays whatever the position
    assert all(k == M.sentinel(i) for i, (f, k) in enumerate(zip(up.fields, up.out_keys)) if f[0] in (-1, 3))
    # map[x] == x everywhere: no byte and no key changes
    ident = by_id(REMAP, "grid-identity")
    assert ident.out_recs == ident.recs and ident.out_keys == ident.keys.tolist() and len(ident.recs) == len(up.recs)
    assert up.out_recs != up.recs
    # only the mate index moves: the key and bytes 4..7 stay
    mate = by_id(REMAP, "grid-mate_only")
    only = [i for i, f in enumerate(mate.fields) if f[:2] == (0, 1) and f[2] & 1]
    assert only and all(mate.out_fields[i] == (0, 2) and mate.out_keys[i] == M.sentinel(i) and
                        mate.out_recs[i][4:8] == mate.recs[i][4:8] and mate.out_recs[i][24:28] == struct.pack("<i", 2)
                        for i in only)
    assert by_id(REMAP, "grid-one").n_in == 1 and {f[0] for f in by_id(REMAP, "grid-one").fields} == {-1, 0}
    none = by_id(REMAP, "grid-none")
    assert none.ref_map is None and {f[0] for f in none.fields} == {-1} and len(none.fields) > 20
    # a merged index past the input's own dictionary
    assert any(c.fields[c.bad][0] == 1 for c in M.remap_refused("past"))
    # atomicMin across workgroups
    for want, case in zip(M.WIDE, REMAP[-2:]):
        ref = [i for i, f in enumerate(case.fields) if not M._accepted("up", f)]
        assert sorted(want) == ref and case.bad == min(want) and len(case.recs) >= 700
        assert len({i // M.WG for i in ref}) == len(want)
    assert list(M.WIDE[0]) != sorted(M.WIDE[0])


def _group_items(rec):
    return [(k, it) for k, it in enumerate(rec.items) if it.kind == "group"]


def test_group_tables():
    for tab in (M.TABLE_PG, M.TABLE_RG):
        olds = [o for o, _ in tab]
        assert len(tab) >= 5 and len(set(olds)) == len(olds)
        assert {b"a", b"ab", b"abc", b""} <= set(olds)
        news = [n for _, n in tab]
        assert b"" in news and None in news and any(n and len(n) == 300 for n in news)
    assert dict(M.TABLE_PG) != dict(M.TABLE_RG)
    # the bytes, spelled out for a small table
    assert M.table_bytes((1, [(b"ab", b"x"), (b"", None)]), (2, ())) == b"\1\2\0" b"\2\0ab\1\0x" b"\0\0\xff\xff" b"\2\0\0"


def test_group_cases_exercise_the_rules():
    assert {c.modes for c in GROUP} == {(p, r) for p in range(3) for r in range(3)}
    assert by_id(GROUP, "modes-00").noop and by_id(GROUP, "modes-00").outputs() == by_id(GROUP, "modes-00").inputs()
    edited = [(c, r) for c in GROUP if not c.noop for r in c.recs[:c.n_keep] if r.edited]
    plain = [(c, r) for c in GROUP if not c.noop for r in c.recs[:c.n_keep] if not r.edited and not r.error]
    place = by_id(GROUP, "placement")
    tabs = {"PG": [o for o, _ in M.TABLE_PG], "RG": [o for o, _ in M.TABLE_RG]}
    # where the edited tag stands, per tag and outcome; which table entry it hits
    spots, hits = set(), {"PG": set(), "RG": set()}
    for r in place.recs:
        gi = [(k, it) for k, it in _group_items(r) if it.info["new"] is not M.KEEP]
        for k, it in gi:
            where = "only" if len(r.items) == 1 else "first" if k == 0 else "last" if k == len(r.items) - 1 else "middle"
            new = it.info["new"]
            spots.add((it.info["tag"], where, "remove" if new is None else "empty" if new == b"" else "replace"))
            hits[it.info["tag"]].add(tabs[it.info["tag"]].index(it.info["old"]) if it.info["old"] in tabs[it.info["tag"]] else -1)
    for tag in ("PG", "RG"):
        for where in ("only", "first", "middle", "last"):
            assert {(tag, where, "remove"), (tag, where, "empty"), (tag, where, "replace")} <= spots
        assert {-1, 0, 1, 2, 3} <= hits[tag]                     # absent, and grp_lookup past its first entry
    # two edits in one record, in both orders, adjacent and apart
    orders = set()
    for r in place.recs:
        gi = [(k, it.info["tag"]) for k, it in _group_items(r) if it.info["new"] is not M.KEEP]
        if len(gi) == 2:
            orders.add((gi[0][1], gi[1][0] - gi[0][0] == 1))
    assert orders == {("PG", True), ("PG", False), ("RG", True), ("RG", False)}
    # a second RG is copied, though the table holds it
    assert any([it.info["new"] is M.KEEP for _, it in _group_items(r) if it.info["tag"] == "RG"] == [False, True] and
               _group_items(r)[-1][1].info["old"] in tabs["RG"] for r in place.recs)
    # a first RG:Z and a later RG that is no string: nothing raises
    for kind in ("int", "group_nonstring"):
        assert any(r.edited and len(r.items) == 2 and r.items[0].kind == "group" and r.items[1].kind == kind and r.items[1].src[:2] == b"RG"
                   for r in place.recs)
    # a first RG that is no string and a later RG:Z: ClassCastException
    c = by_id(GROUP, "cast-first_nonstring")
    r = c.recs[c.err[1]]
    assert c.err[0] == "ClassCastException" and r.items[0].src[:3] == b"RGA" and r.items[1].src[:3] == b"RGZ"
    # a PG typed 'A' under PG mode 0
    c = by_id(GROUP, "pg_char_mode0")
    assert c.modes == (0, 1) and all(r.items and any(it.src[:3] == b"PGA" for it in r.items) for r in c.recs)
    assert [r.edited for r in c.recs] == [False, True, True] and c.err is None
    # precedence inside one record
    c = by_id(GROUP, "prec-cast_before_null")
    assert c.modes[0] == 2 and c.err[0] == "ClassCastException" and c.recs[c.err[1]].items[0].src[:3] == b"PGA"
    c = by_id(GROUP, "prec-pg_first")
    r = c.recs[c.err[1]]
    assert c.modes == (2, 1) and c.err[0] == "NullPointerException" and {it.src[:3] for it in r.items} == {b"RGA", b"PGZ"}
    c = by_id(GROUP, "neither-mode2")
    assert c.modes == (2, 2) and c.err is None and not any(_group_items(r) for r in c.recs) and c.outputs() == c.inputs()
    # integers: every listed value in every type that holds it, with and without an edit
    want = {(t, v) for v in M.INT_VALUES for t, (lo, hi) in M.HOLDS.items() if lo <= v <= hi}
    assert len(M.INT_VALUES) == 15 and len(want) == 46
    for pool in (edited, plain):
        assert {(it.info["typ"], it.info["v"]) for _, r in pool for it in r.items if it.kind == "int"} >= want
    changes = {(it.info["typ"], it.dst[2:3].decode()) for _, r in edited for it in r.items if it.kind == "int"}
    assert changes >= {("C", "c"), ("s", "c"), ("S", "c"), ("S", "C"), ("i", "c"), ("i", "C"), ("i", "s"), ("i", "S"),
                       ("I", "c"), ("I", "C"), ("I", "S"), ("I", "i"), ("s", "C"), ("i", "i"), ("I", "I"), ("s", "s")}
    # the other value types, copied
    for pool in (edited, plain):
        raws = [it.src for _, r in pool for it in r.items if it.kind in ("raw", "B")]
        assert {b[2:3] for b in raws} >= {b"A", b"f", b"Z", b"H", b"B"}
        assert any(b[2:] == b"Z\0" for b in raws) and any(b[2:] == b"H\0" for b in raws)
        assert {(b[3:4].decode(), struct.unpack_from("<I", b, 4)[0]) for b in raws if b[2:3] == b"B"} == \
            {(s, n) for s in "cCsSiIf" for n in (0, 1, 3)}
    # the fixed part
    for pool in (edited, plain):
        recs = [r for _, r in pool]
        assert {r.l_seq for r in recs} >= {0, 1, 2, 15, 16}
        assert all(any(r.l_seq == n and r.seq[-1] & 15 for r in recs) for n in (1, 15))
        assert any(r.l_seq > 2 and r.qual[0] == 0xff and set(r.qual[1:]) - {0xff} for r in recs)
        assert any(r.l_seq > 2 and r.qual[0] != 0xff and set(r.qual[1:]) == {0xff} for r in recs)
        assert any(r.l_seq == 1 and r.qual == b"\xff" for r in recs)
        assert any(r.ref == -1 and r.bin for r in recs) and any(r.ref >= 0 and r.bin & 1 for r in recs)
    # errors that stop the job
    bad = [c for c in GROUP if c.id.startswith(("malformed-", "overrun-")) and not c.noop]
    assert len(bad) == len(M.MALFORMED) + 4 and all(c.err[0] == "SAMFormatException" for c in bad)
    assert {c.err[1] for c in bad} >= {0, 1, 2} and any(c.err[1] and c.recs[0].edited for c in bad)
    assert any(not _group_items(c.recs[c.err[1]]) for c in bad)                    # neither tag, still raised
    assert by_id(GROUP, "overrun-first").err[1] == 0 and by_id(GROUP, "overrun-first").outputs() == []
    noop = by_id(GROUP, "malformed-noop")
    assert noop.noop and noop.err is None and noop.outputs() == noop.inputs()
    wide = by_id(GROUP, "wide_errors")
    at = [i for i, r in enumerate(wide.recs) if r.error]
    assert len({i // M.WG for i in at}) == 3 and wide.err[1] == min(at)
    assert len({r.error for r in wide.recs if r.error}) == 2
    # one run whose output grows and shrinks across workgroups
    mixed = by_id(GROUP, "mixed")
    delta = [len(r.output()) - len(r.input()) for r in mixed.recs]
    assert len(mixed.recs) >= 600
    for w in range(0, len(delta), M.WG):
        d = delta[w:w + M.WG]
        assert any(x > 250 for x in d) and any(x < 0 for x in d) and any(x == 0 for x in d)
    assert sum(1 for r in mixed.recs if len([1 for _, it in _group_items(r)]) == 2) > 50


# ---- known answers, written by hand ---------------------------------------------------------------------------
def H(s):
    return bytes.fromhex(s.replace(" ", ""))


# refID 1, pos 9, l_read_name 2, mapq 30, bin 4683, no CIGAR, flag 0, l_seq 3, no mate; name "q";
# SEQ 0x12 0x3f: three bases and a pad nibble of 0xf; QUAL 1 2 3
FIXED = "01000000 09000000 02 1e 4b12 0000 0000 03000000 ffffffff ffffffff 00000000 7100"
SQ_IN, SQ_OUT = "123f 010203", "1230 010203"
RG_A, RG_RA = "52475a 61 00", "52475a 722e61 00"        # RG:Z:a -> RG:Z:r.a (TABLE_RG)

KNOWN = [
    # (name, fixed in, seq+qual in, aux in, fixed out, seq+qual out, aux out)
    ("C127_to_c__C128_stays", FIXED, SQ_IN, RG_A + "585643 7f" + "585943 80", FIXED, SQ_OUT, RG_RA + "585663 7f" + "585943 80"),
    ("s_to_c__s_stays", FIXED, SQ_IN, "585673 80ff" + RG_A + "585973 7fff", FIXED, SQ_OUT, "585663 80" + RG_RA + "585973 7fff"),
    ("S_to_C_and_c__S_stays", FIXED, SQ_IN, "585653 ff00" + "585953 0001" + "585a53 7f00" + RG_A, FIXED, SQ_OUT,
     "585643 ff" + "585953 0001" + "585a63 7f" + RG_RA),
    ("i_to_S_s_c_C__i_stays", FIXED, SQ_IN,
     RG_A + "583069 ffff0000" + "583169 00000100" + "583269 0080ffff" + "583369 ff7fffff" + "583469 ffffffff" + "583569 80000000",
     FIXED, SQ_OUT, RG_RA + "583053 ffff" + "583169 00000100" + "583273 0080" + "583369 ff7fffff" + "583463 ff" + "583543 80"),
    ("I_to_i_c_S__I_stays", FIXED, SQ_IN,
     "583049 ffffff7f" + "583149 00000080" + "583249 ffffffff" + "583349 00000000" + "583449 00010000" + RG_A,
     FIXED, SQ_OUT, "583069 ffffff7f" + "583149 00000080" + "583249 ffffffff" + "583363 00" + "583453 0001" + RG_RA),
    ("absent_qualities", FIXED, "123f ff0203", RG_A, FIXED, "1230 ffffff", RG_RA),
    ("later_ff_is_kept", FIXED, "123f 01ffff", RG_A, FIXED, "1230 01ffff", RG_RA),
    ("unplaced_bin_0", "ffffffff 09000000 02 1e 4b12 0000 0000 03000000 ffffffff ffffffff 00000000 7100", SQ_IN, RG_A,
     "ffffffff 09000000 02 1e 0000 0000 0000 03000000 ffffffff ffffffff 00000000 7100", SQ_OUT, RG_RA),
    ("remove", FIXED, SQ_IN, "585643 05" + "52475a 7a 00" + "58595a 6100", FIXED, SQ_OUT, "585663 05" + "58595a 6100"),
    ("replace_with_empty", FIXED, SQ_IN, "50475a 6162 00" + "585643 05", FIXED, SQ_OUT, "50475a 00" + "585663 05"),
    ("first_of_two_RG", FIXED, SQ_IN, RG_A + "52475a 7a 00", FIXED, SQ_OUT, RG_RA + "52475a 7a 00"),
    ("no_tag_no_edit", FIXED, SQ_IN, "585643 7f" + "585969 05000000", FIXED, SQ_IN, "585643 7f" + "585969 05000000"),
    ("float_char_hex_array_copied", FIXED, SQ_IN, "584166 0000c0bf" + "584241 51" + "584348 314100" + "58444273 02000000 0100feff" + RG_A,
     FIXED, SQ_OUT, "584166 0000c0bf" + "584241 51" + "584348 314100" + "58444273 02000000 0100feff" + RG_RA),
]


def _rec(fixed, sq, aux):
    body = H(fixed) + H(sq) + H(aux)
    return struct.pack("<i", len(body)) + body


@pytest.mark.parametrize("row", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_group_answers(oracle_mod, row):
    _, f_in, sq_in, aux_in, f_out, sq_out, aux_out = row
    case = M.GroupCase("known", [], (1, M.TABLE_PG), (1, M.TABLE_RG))
    src = _rec(f_in, sq_in, aux_in)
    pay, off = F.pack([src])
    got, got_off = oracle_mod.rewrite_group_tags(pay, off.astype(np.int64), case.groups, case.inp)
    assert bytes(got) == _rec(f_out, sq_out, aux_out) and got_off.tolist() == [0, len(got)]
    assert len(src) == 4 + 32 + 2 + 5 + len(H(aux_in))


def test_known_remap_answers(oracle_mod):
    """refID 0 -> 1 at pos -1: the key is -1 (the sign-extended pos ORed in); the unpaired read's mate
    refID 7, outside the 3-entry map, stays and refuses nothing; a paired one is refused"""
    unpaired = _rec("00000000 ffffffff 02 1e 4b12 0000 1000 03000000 07000000 ffffffff 00000000 7100", SQ_IN, "")
    moved = _rec("01000000 ffffffff 02 1e 4b12 0000 1000 03000000 07000000 ffffffff 00000000 7100", SQ_IN, "")
    paired = _rec("00000000 ffffffff 02 1e 4b12 0000 1100 03000000 07000000 ffffffff 00000000 7100", SQ_IN, "")
    mate = _rec("02000000 05000000 02 1e 4b12 0000 0100 03000000 00000000 ffffffff 00000000 7100", SQ_IN, "")
    mate_moved = _rec("02000000 05000000 02 1e 4b12 0000 0100 03000000 01000000 ffffffff 00000000 7100", SQ_IN, "")
    pay, off = F.pack([unpaired, mate, paired])
    got, keys, bad = oracle_mod.correct_payloads(pay, off, [11, 22, 33], [1, 2, 2])
    assert bad == 2
    assert bytes(got) == moved + mate_moved + paired
    assert keys.tolist() == [-1, 22, 33]
