"""Crafted records for the multi-input Sort's record correction (Utils.correctSAMRecordForMerging,
cli/Utils.java:286-324): hbam_merge_remap (k_merge_remap, csrc/hbam_sort.hip) and hbam_rewrite_groups
(grp_encode / k_grp_len / k_grp_write, csrc/hbam_groups.hip), whose only other inputs are
small_pe.bam and copies of it.

Every case declares its own outcome, from pieces and not by parsing bytes: a remap case rebuilds each
record with the indices the reference's text gives it; a group case lists each aux item as (bytes in,
bytes out once the record is re-encoded) and says per record whether an edit happens, and which
record raises what.  test_merge_model.py holds the oracle to these declarations and to hand-written
literals; test_merge_gpu.py holds the device to the oracle.

The tables are built directly, not through headers and SamFileHeaderMerger: one header pair cannot
produce a table per tag with different contents, an empty id, or a mode pair such as (1, 2)."""
import struct

import numpy as np

import f4_records as F

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
WG = 256  # RS_WG (k_merge_remap) and F4_WG (k_grp_len, k_grp_write)


# ---- hbam_merge_remap ---------------------------------------------------------------------------------------
MAPS = {
    "up": [1, 2, 3, 3],        # 0, 1, 2 move up; 3 stays
    "identity": [0, 1, 2, 3],  # map[x] == x: no byte may change
    "one": [0],
    "none": None,              # n_in = 0: every accepted refID is -1
    "past": [1, 2],            # map[1] lies past the input's own dictionary
    "mate_only": [0, 2, 2],    # ref 0 stays while mate 1 moves
}
POSITIONS = [-2, -1, 0, I32_MAX]


def sentinel(i):
    """a starting key no re-key can produce: one that moves when it should not is visible"""
    return (0x5151 << 32) | i


def _record(i, f):
    ref, mref, flag, pos = f
    ls = 3 + i % 4
    return F.record(b"m%d" % i, flag=flag, ref=ref, pos=pos, nref=mref, npos=7 + i, cigar=((ls, 0),), l_seq=ls,
                    aux=F.aux_int("NM", "C", i % 200), seed=i)


class RemapCase:
    """fields: (refID, mate refID, flag, pos) per record"""

    def __init__(self, cid, fields, ref_map):
        self.id, self.fields, self.ref_map = cid, list(fields), ref_map
        self.n_in = 0 if ref_map is None else len(ref_map)
        self.recs = [_record(i, f) for i, f in enumerate(self.fields)]
        self.keys = np.array([sentinel(i) for i in range(len(self.recs))], np.int64)
        self.bad, self.out_fields, self.out_keys = self._outcome()
        # the corrected records, rebuilt from their fields (not patched)
        self.out_recs = [_record(i, (nr, nm, f[2], f[3])) for i, (f, (nr, nm)) in enumerate(zip(self.fields, self.out_fields))]

    def _moved(self, x):
        """the merged index of x, or None where setReferenceIndex / setMateReferenceIndex throw:
        an index that is not in the input's dictionary, or whose merged index is not"""
        if x == -1:
            return -1
        if x < 0 or x >= self.n_in:
            return None
        return self.ref_map[x] if self.ref_map[x] < self.n_in else None

    def _outcome(self):
        out, keys = [], []
        for i, (ref, mref, flag, pos) in enumerate(self.fields):
            nr = self._moved(ref)
            nm = self._moved(mref) if flag & 1 else mref  # cli/Utils.java:301: paired reads only
            if nr is None or nm is None:
                return i, out, keys
            key = sentinel(i)
            # the key is recomputed when refID changed; getKey takes the coordinate form for a mapped
            # record whose 1-based start (pos + 1 as a Java int) is not negative
            if nr != ref and not flag & 4 and -1 <= pos < I32_MAX:
                key = -1 if pos == -1 else nr * (1 << 32) + pos
            out.append((nr, nm))
            keys.append(key)
        return -1, out, keys

    @property
    def n_expected(self):
        return len(self.out_fields)


def _values(n_in):
    v = [-1, 0, n_in - 1, n_in, n_in + 5, -2, I32_MIN, I32_MAX] + list(range(n_in))
    return sorted(set(v), key=v.index)


def _grid(n_in, positions):
    k = 0
    for ref in _values(n_in):
        for mref in _values(n_in):
            for paired in (0, 1):
                for unmapped in (0, 4):
                    for pos in positions:
                        k += 1
                        yield (ref, mref, paired | unmapped | (0x40 if k % 3 == 0 else 0), pos)


def _accepted(name, f):
    probe = RemapCase.__new__(RemapCase)
    probe.fields, probe.ref_map, probe.n_in = [f], MAPS[name], len(MAPS[name] or ())
    return probe._outcome()[0] < 0


def remap_grid(name):
    """every accepted combination of the edge values, crossed with the positions"""
    n_in = len(MAPS[name] or ())
    return RemapCase("grid-" + name, [f for f in _grid(n_in, POSITIONS) if _accepted(name, f)], MAPS[name])


def remap_refused(name):
    """one small case per refused combination: accepted records, the refused one, an accepted one"""
    n_in = len(MAPS[name] or ())
    ok = [f for f in _grid(n_in, [5]) if _accepted(name, f)]
    out = []
    for k, f in enumerate(f for f in _grid(n_in, [100]) if not _accepted(name, f)):
        lead = [ok[(k + j) % len(ok)] for j in range(k % 3)]
        out.append(RemapCase("refused-%s-%d" % (name, k), lead + [f, ok[k % len(ok)]], MAPS[name]))
    return out


def remap_wide(refused_at):
    """more than two workgroups of accepted records with refused ones at refused_at"""
    ok = [f for f in _grid(4, POSITIONS) if _accepted("up", f)]
    no = [f for f in _grid(4, [100]) if not _accepted("up", f)]
    fields = [ok[(7 * i) % len(ok)] for i in range(800)]
    for j, i in enumerate(refused_at):
        fields[i] = no[(11 * j) % len(no)]
    return RemapCase("wide-" + "-".join(map(str, refused_at)), fields, MAPS["up"])


WIDE = [(770, 300, 520), (790,)]


def remap_cases():
    return [remap_grid(n) for n in MAPS] + [remap_wide(w) for w in WIDE]


# ---- hbam_rewrite_groups ------------------------------------------------------------------------------------
KEEP = "keep"  # a group tag the step leaves as it is
INT_RANGES = [(I32_MIN, -32769, "i"), (-32768, -129, "s"), (-128, 127, "c"), (128, 255, "C"), (256, 65535, "S"),
              (65536, I32_MAX, "i"), (1 << 31, (1 << 32) - 1, "I")]  # BinaryTagCodec.getIntegerType, as ranges
INT_VALUES = [-32769, -32768, -129, -128, -1, 0, 127, 128, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
HOLDS = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (I32_MIN, I32_MAX),
         "I": (0, (1 << 32) - 1)}
LONG = b"L" * 299 + b"!"
# ids that are prefixes of one another, an empty old id, a new id of length 0, one of 300 bytes, new_len -1
TABLE_PG = [(b"a", b"A1"), (b"abc", LONG), (b"ab", b""), (b"", b"empty"), (b"gone", None), (b"same", b"same"),
            (b"z", b"zz.1")]
TABLE_RG = [(b"z", None), (b"abc", b"r.abc"), (b"a", b"r.a"), (b"ab", LONG), (b"", b""), (b"same", b"same"),
            (b"rgonly", b"x")]


def smallest_type(v):
    return next(t for lo, hi, t in INT_RANGES if lo <= v <= hi)


class Item:
    def __init__(self, kind, src, dst, **info):
        self.kind, self.src, self.dst, self.info = kind, src, dst, info


def I(tag, typ, v):
    """an integer tag: re-typed to the smallest type when the record is re-encoded"""
    return Item("int", F.aux_int(tag, typ, v), F.aux_int(tag, smallest_type(v), v), typ=typ, v=v)


def raw(b, kind="raw"):
    """copied verbatim: A, f, Z, H, B"""
    return Item(kind, b, b)


def G(tag, old, new=KEEP):
    """a string group tag: left (KEEP), removed (None) or replaced in place (bytes)"""
    src = tag.encode() + b"Z" + old + b"\0"
    dst = src if new is KEEP else b"" if new is None else src[:3] + new + b"\0"
    return Item("group", src, dst, tag=tag, old=old, new=new)


class Rec:
    """One record: its items, whether the step edits it (so that it is re-encoded), and what it
    raises.  seq / qual default to bytes with a non-zero pad nibble and no 0xff."""

    def __init__(self, items=(), edited=False, error=None, l_seq=5, seq=None, qual=None, ref=2, pos=100,
                 bin_=4681, flag=0, mref=-1, seed=0, name=b"g"):
        rng = np.random.default_rng(1000 + seed)
        if seq is None:
            seq = bytearray(rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes())
            if l_seq & 1:
                seq[-1] |= 0x05
        if qual is None:
            qual = rng.integers(0, 94, l_seq, dtype=np.uint8).tobytes()
        self.items, self.edited, self.error = list(items), edited, error
        self.l_seq, self.seq, self.qual = l_seq, bytes(seq), bytes(qual)
        self.ref, self.pos, self.bin, self.flag, self.mref, self.name = ref, pos, bin_, flag, mref, name

    def _build(self, aux, seq, qual, bin_):
        return F.record(self.name, flag=self.flag, ref=self.ref, pos=self.pos, nref=self.mref, npos=3,
                        cigar=((self.l_seq, 0),) if self.l_seq else (), l_seq=self.l_seq, aux=aux, bin_=bin_,
                        seq=seq, qual=qual)

    def input(self):
        return self._build(b"".join(i.src for i in self.items), self.seq, self.qual, self.bin)

    def output(self):
        """BAMRecordCodec.encode of the edited record; the record's own bytes without an edit"""
        if not self.edited:
            return self.input()
        seq = bytearray(self.seq)
        if self.l_seq & 1:
            seq[-1] &= 0xF0
        qual = b"\xff" * self.l_seq if self.qual[:1] == b"\xff" else self.qual
        return self._build(b"".join(i.dst for i in self.items), seq, qual, 0 if self.ref < 0 else self.bin)

    def moved(self, ref, mref):
        r = Rec.__new__(Rec)
        r.__dict__.update(self.__dict__)
        r.ref, r.mref = ref, mref
        return r


class RawRec:
    """bytes as given (an n_cigar / l_seq overrun)"""
    items, edited, l_seq = (), False, None

    def __init__(self, data, error=None):
        self.data, self.error = data, error

    def input(self):
        return self.data

    output = input


def table_bytes(pg, rg):
    """include/hbam.h: per tag u8 mode, u16 count, entries {u16 old_len, old, i16 new_len, new}"""
    out = b""
    for mode, entries in (pg, rg):
        out += struct.pack("<BH", mode, len(entries))
        for old, new in entries:
            out += struct.pack("<H", len(old)) + old + struct.pack("<h", -1 if new is None else len(new)) + (new or b"")
    return out


class GroupCase:
    """recs, the (mode, entries) of PG and of RG, and err = (exception, record) or None"""

    def __init__(self, cid, recs, pg=(0, ()), rg=(0, ()), err=None, inp=1):
        self.id, self.recs, self.pg, self.rg, self.err, self.inp = cid, list(recs), pg, rg, err, inp
        self.table = table_bytes(pg, rg)
        self.groups = {"pg_collisions": pg[0] != 0, "rg_collisions": rg[0] != 0,
                       "pg": {inp: dict(pg[1])} if pg[0] == 1 else {},
                       "rg_lookup": {inp: dict(rg[1])} if rg[0] == 1 else {}}
        self.noop = pg[0] == 0 and rg[0] == 0

    @property
    def modes(self):
        return self.pg[0], self.rg[0]

    @property
    def n_keep(self):
        return len(self.recs) if self.err is None else self.err[1]

    def inputs(self):
        return [r.input() for r in self.recs]

    def outputs(self):
        """the records that stand: all of them, or those before the one that raises"""
        return [r.output() for r in self.recs[:self.n_keep]]


ODD = dict(l_seq=5, bin_=4683)  # an odd length (pad nibble set), an odd bin


def _plain(seed, **kw):
    """neither tag, but everything a re-encode would change"""
    return Rec([I("NM", "i", 5), I("XS", "S", 7), raw(F.aux_z("MD", "5"))], seed=seed, **dict(ODD, **kw))


def modes_case(pm, rm):
    pg, rg = (pm, TABLE_PG if pm != 2 else ()), (rm, TABLE_RG if rm != 2 else ())
    ints = [I("NM", "i", 5), I("XI", "I", 200)]
    p_new = b"A1" if pm == 1 else KEEP
    r_new = b"r.a" if rm == 1 else KEEP
    recs = [_plain(0),
            Rec(ints + [G("PG", b"a", p_new)], edited=pm == 1, error="NullPointerException" if pm == 2 else None, seed=1, **ODD),
            Rec(ints + [G("RG", b"a", r_new)], edited=rm == 1, error="NullPointerException" if rm == 2 else None, seed=2, **ODD),
            Rec([G("RG", b"a", r_new)] + ints + [G("PG", b"a", p_new)], edited=pm == 1 or rm == 1,
                error="NullPointerException" if 2 in (pm, rm) else None, seed=3, **ODD),
            _plain(4)]
    err = next((("NullPointerException", i) for i, r in enumerate(recs) if r.error), None)
    return GroupCase("modes-%d%d" % (pm, rm), recs, pg, rg, err)


def placement_case():
    """the edited tag first, in the middle, last and alone; replaced, removed, emptied, lengthened;
    PG and RG in one record in both orders, adjacent and apart; a second RG; values not in the table"""
    a, b = I("XA", "i", 1), raw(F.aux_z("XZ", "zed"))
    recs = []
    for tag, (old, new) in (("RG", (b"a", b"r.a")), ("PG", (b"a", b"A1")), ("RG", (b"z", None)), ("PG", (b"gone", None)),
                            ("RG", (b"", b"")), ("PG", (b"", b"empty")), ("RG", (b"ab", LONG)), ("PG", (b"abc", LONG)),
                            ("PG", (b"ab", b"")), ("RG", (b"abc", b"r.abc")), ("RG", (b"abcd", None)),
                            ("PG", (b"nope", None)), ("RG", (b"same", b"same")), ("RG", (b"A", None))):
        g = G(tag, old, new)
        recs += [Rec([g, a, b], True), Rec([a, g, b], True), Rec([a, b, g], True), Rec([g], True)]
    p, r = G("PG", b"a", b"A1"), G("RG", b"ab", LONG)
    recs += [Rec([p, r], True), Rec([r, p], True), Rec([p, a, r], True), Rec([r, a, b, p], True),
             Rec([a, G("PG", b"gone", None), G("RG", b"z", None), b], True),
             Rec([G("RG", b"z", None), G("PG", b"gone", None)], True)]
    # two RG: the first is edited, the second (a table id) copied
    recs += [Rec([G("RG", b"a", b"r.a"), a, G("RG", b"abc", KEEP)], True),
             Rec([G("RG", b"z", None), G("RG", b"z", KEEP)], True),
             Rec([G("PG", b"a", b"A1"), G("PG", b"a", KEEP), G("RG", b"a", b"r.a")], True)]
    # a first RG:Z and a later RG that is no string: nothing raises, the later one is re-typed or copied
    recs += [Rec([G("RG", b"a", b"r.a"), I("RG", "i", 5)], True),
             Rec([G("RG", b"a", b"r.a"), raw(F.aux_a("RG", b"x"), "group_nonstring")], True)]
    for i, rec in enumerate(recs):
        rec.name = b"p%d" % i
    return GroupCase("placement", recs, (1, TABLE_PG), (1, TABLE_RG))


def retype_case():
    """every listed value in every source type that holds it, in edited records and in twins without
    an edit, and all of them in one record"""
    recs, every = [], []
    for v in INT_VALUES:
        for typ, (lo, hi) in HOLDS.items():
            if lo <= v <= hi:
                recs.append(Rec([I("XV", typ, v), G("RG", b"a", b"r.a")], True, seed=len(recs)))
                recs.append(Rec([I("XV", typ, v)], False, seed=len(recs)))
                every.append(I("X" + typ, typ, v))
    recs.append(Rec(every[:40] + [G("RG", b"a", b"r.a")] + every[40:], True))
    recs.append(Rec(every, False))
    return GroupCase("retype", recs, (0, ()), (1, TABLE_RG))


def values_case():
    """A, f, an empty Z, H, B of each subtype with 0, 1 and 3 elements: copied, edit or not"""
    vals = [raw(F.aux_a("XA", b"Q")), raw(F.aux_f("XF", -1.5)), raw(F.aux_z("XE", "")), raw(F.aux_h("XH", b"1AE301")),
            raw(F.aux_h("XG", b""))]
    for sub in "cCsSiIf":
        for n in (0, 1, 3):
            vals.append(raw(F.aux_b("B" + sub, sub, [0, 1, 2][:n] if sub in "CSI" else [-1, 1.0 if sub == "f" else 1, -3][:n]), "B"))
    recs = []
    for k, it in enumerate(vals):
        recs += [Rec([it, G("PG", b"z", b"zz.1")], True, seed=k), Rec([G("PG", b"z", b"zz.1"), it], True, seed=k),
                 Rec([it], False, seed=k)]
    recs += [Rec(vals + [G("PG", b"z", b"zz.1")], True), Rec(vals, False)]
    # a PG typed 'A' under PG mode 0 is not looked at
    pa = raw(F.aux_a("PG", b"x"), "group_nonstring")
    case = GroupCase("values", recs, (1, TABLE_PG), (0, TABLE_RG))
    other = GroupCase("pg_char_mode0", [Rec([pa, I("NM", "i", 5)], False), Rec([pa, I("NM", "i", 5), G("RG", b"a", b"r.a")], True),
                                        Rec([G("RG", b"a", b"r.a"), pa], True)], (0, TABLE_PG), (1, TABLE_RG))
    return [case, other]


def fixed_case():
    """l_seq 0, 1, 2, 15, 16 with the pad nibble set on the odd ones; absent and present qualities;
    the bin of an unplaced and of a placed record — each edited and as a twin without an edit"""
    shapes = []
    for ls in (0, 1, 2, 15, 16):
        seq = bytes([0x12 + 3 * k & 0xff for k in range((ls + 1) // 2)])
        if ls & 1:
            seq = seq[:-1] + bytes([seq[-1] & 0xF0 | 0x0B])
        shapes.append(dict(l_seq=ls, seq=seq))
        if ls:
            shapes.append(dict(l_seq=ls, seq=seq, qual=b"\xff" + bytes(range(1, ls))))        # absent: all 0xff
            shapes.append(dict(l_seq=ls, seq=seq, qual=b"\x07" + b"\xff" * (ls - 1)))         # present: kept
            shapes.append(dict(l_seq=ls, seq=seq, qual=b"\xff" * ls))
    shapes += [dict(ref=-1, pos=-1, bin_=4681, flag=4), dict(ref=-1, pos=55, bin_=1, flag=0),
               dict(ref=3, pos=9, bin_=4683), dict(ref=0, pos=0, bin_=0xffff), dict(ref=-1, bin_=0)]
    recs = []
    for k, s in enumerate(shapes):
        recs += [Rec([G("RG", b"a", b"r.a")], True, seed=k, **s), Rec([G("RG", b"z", None)], True, seed=k, **s),
                 Rec([raw(F.aux_z("XZ", "a"))], False, seed=k, **s), Rec([], False, seed=k, **s)]
    return GroupCase("fixed", recs, (0, ()), (1, TABLE_RG))


def cast_cases():
    ok = Rec([G("RG", b"a", b"r.a"), I("NM", "i", 1)], True)
    ch = raw(F.aux_a("RG", b"x"), "group_nonstring")
    pch = raw(F.aux_a("PG", b"x"), "group_nonstring")
    cce, npe = "ClassCastException", "NullPointerException"
    return [
        # a first RG that is no string and a later RG:Z
        GroupCase("cast-first_nonstring", [ok, _plain(1), Rec([ch, G("RG", b"a")], error=cce), ok], (1, TABLE_PG), (1, TABLE_RG), (cce, 2)),
        GroupCase("cast-int_rg", [ok, Rec([I("NM", "i", 1), Item("group_nonstring", F.aux_int("RG", "C", 3), b"")], error=cce)],
                  (0, ()), (1, TABLE_RG), (cce, 1)),
        # the cast precedes the table: a PG that is no string under mode 2
        GroupCase("prec-cast_before_null", [_plain(0), Rec([pch, G("RG", b"a")], error=cce)], (2, ()), (1, TABLE_RG), (cce, 1)),
        # PG runs first: a PG:Z under mode 2 and an RG that is no string
        GroupCase("prec-pg_first", [_plain(0), Rec([ch, G("PG", b"a")], error=npe)], (2, ()), (1, TABLE_RG), (npe, 1)),
        # the PG edit is accepted and then the RG cast raises
        GroupCase("prec-pg_ok_rg_cast", [ok, Rec([G("PG", b"a"), ch], error=cce)], (1, TABLE_PG), (1, TABLE_RG), (cce, 1)),
        GroupCase("prec-rg_null_after_pg", [_plain(0), Rec([G("PG", b"a"), G("RG", b"a")], error=npe)], (1, TABLE_PG), (2, ()), (npe, 1)),
        # neither tag under mode 2: nothing raises, every record keeps its bytes
        GroupCase("neither-mode2", [_plain(k) for k in range(5)], (2, ()), (2, ())),
    ]


MALFORMED = {
    "trunc1": F.aux_int("NM", "C", 1) + b"X",
    "trunc2": F.aux_int("NM", "C", 1) + b"XY",
    "only1": b"X",
    "unknown_type": b"XYq\0" + F.aux_int("NM", "C", 1),
    "z_no_nul": F.aux_int("NM", "C", 1) + b"XZZabc",
    "h_no_nul": b"XHH1A",
    "int_cut": b"XYi\1\2",
    "b_header_cut": b"XBBc\1\0\0",
    "b_count_past": b"XBBs" + struct.pack("<I", 3) + b"\1\0\2\0\3",
    "b_count_huge": b"XBBi" + struct.pack("<I", 0xffffffff) + b"\0" * 8,
    "b_subtype": b"XBBZ" + struct.pack("<I", 1) + b"\0",
    "tag_after_bad": b"XYq\0" + F.aux_z("RG", "a"),
}
SFE = "SAMFormatException"


def malformed_cases():
    """SAMFormatException whenever a mode is on, tag or no tag; the records before it stand"""
    ok = Rec([G("RG", b"a", b"r.a"), I("NM", "i", 1)], True)
    out = []
    for k, (name, aux) in enumerate(MALFORMED.items()):
        lead = [ok, _plain(k)][:k % 3]
        bad = Rec([Item("malformed", aux, b"")], error=SFE, l_seq=k % 4)
        out.append(GroupCase("malformed-" + name, lead + [bad, ok], (0, ()), (1, TABLE_RG), (SFE, len(lead))))
    for field in ("cigar", "seq"):
        out.append(GroupCase("overrun-" + field, [ok, _plain(1), RawRec(F.overrun_record(field), SFE), ok], (1, TABLE_PG), (1, TABLE_RG), (SFE, 2)))
    # a block_size under the 32 fixed bytes
    out.append(GroupCase("overrun-block_size", [ok, RawRec(struct.pack("<i", 20) + bytes(range(20)), SFE), ok], (0, ()),
                         (1, TABLE_RG), (SFE, 1)))
    out.append(GroupCase("overrun-first", [RawRec(F.overrun_record("seq"), SFE), ok], (2, ()), (2, ()), (SFE, 0)))
    # with both modes off nothing is parsed
    out.append(GroupCase("malformed-noop", [Rec([G("RG", b"a"), I("NM", "i", 1)]), Rec([Item("malformed", b"XYq\0", b"")]),
                                            RawRec(F.overrun_record("cigar"))]))
    return out


def wide_errors_case():
    """errors in three workgroups: the smallest index is the job's"""
    recs = [Rec([G("RG", b"a", b"r.a"), I("NM", "i", i)], True, seed=i, l_seq=i % 7) if i % 3 else _plain(i, l_seq=i % 5)
            for i in range(800)]
    recs[770] = Rec([Item("malformed", b"XY", b"")], error=SFE)
    recs[300] = Rec([raw(F.aux_a("RG", b"x"), "group_nonstring")], error="ClassCastException")
    recs[520] = RawRec(F.overrun_record("cigar"), SFE)
    return GroupCase("wide_errors", recs, (0, ()), (1, TABLE_RG), ("ClassCastException", 300))


def mixed_case(n=600):
    """records that grow (an id of 300 bytes), shrink (a removed tag, integers re-typed down) and stay,
    in no order: k_grp_write's offsets cross workgroups in both directions"""
    rng = np.random.default_rng(77)
    pgs = [(b"a", b"A1"), (b"abc", LONG), (b"ab", b""), (b"", b"empty"), (b"gone", None), (b"same", b"same"),
           (b"z", b"zz.1"), (b"nope", None)]
    rgs = [(b"z", None), (b"abc", b"r.abc"), (b"a", b"r.a"), (b"ab", LONG), (b"", b""), (b"rgonly", b"x"),
           (b"abcd", None)]
    recs = []
    for i in range(n):
        items = [I("X%d" % j, "i", int(rng.integers(-200, 300))) for j in range(int(rng.integers(0, 5)))]
        items += [raw(F.aux_z("MD", "A" * int(rng.integers(0, 20))))]
        kind = int(rng.integers(0, 4))
        if kind & 1:
            items.insert(int(rng.integers(0, len(items) + 1)), G("PG", *pgs[int(rng.integers(0, len(pgs)))]))
        if kind & 2:
            items.insert(int(rng.integers(0, len(items) + 1)), G("RG", *rgs[int(rng.integers(0, len(rgs)))]))
        ref = int(rng.integers(-1, 4))
        recs.append(Rec(items, kind != 0, seed=i, l_seq=int(rng.integers(0, 40)), ref=ref, bin_=int(rng.integers(0, 40000)),
                        qual=None if rng.random() < .7 else b"\xff" * 0, name=b"x%d" % i))
        if recs[-1].qual == b"" and recs[-1].l_seq:
            recs[-1].qual = b"\xff" + bytes(rng.integers(0, 256, recs[-1].l_seq - 1, dtype=np.uint8))
    return GroupCase("mixed", recs, (1, TABLE_PG), (1, TABLE_RG))


def group_cases():
    out = [modes_case(pm, rm) for pm in (0, 1, 2) for rm in (0, 1, 2)]
    out += [placement_case(), retype_case()] + values_case() + [fixed_case()] + cast_cases() + malformed_cases()
    out += [wide_errors_case(), mixed_case()]
    return out


# ---- both steps, in the product's order -----------------------------------------------------------------------
class ProductCase:
    """sort.correct_split: the remap over every record, then the group step over the records before
    the refused one; a group error there is the job's"""

    def __init__(self, cid, recs, ref_map, pg, rg, bad, err=None):
        self.id, self.recs, self.ref_map, self.bad, self.err = cid, recs, ref_map, bad, err
        n_keep = len(recs) if bad < 0 else bad
        self.groups = GroupCase(cid, recs[:n_keep], pg, rg, err)
        self.table = self.groups.table
        m = ref_map

        def mv(x):
            return x if x < 0 else m[x]
        self.keys = np.array([sentinel(i) for i in range(len(recs))], np.int64)
        self.out_keys = [(mv(r.ref) << 32) | r.pos if mv(r.ref) != r.ref else sentinel(i)
                         for i, r in enumerate(recs[:n_keep])]
        keep = recs[:n_keep] if err is None else recs[:err[1]]
        self.out_recs = [r.moved(mv(r.ref), mv(r.mref) if r.flag & 1 else r.mref).output() for r in keep]

    def inputs(self):
        return [r.input() for r in self.recs]


def product_cases():
    def recs(n):
        out = []
        for i in range(n):
            items = [I("NM", "i", i % 300)]
            if i % 3:
                items.append(G("RG", b"a", b"r.a") if i % 2 else G("RG", b"z", None))
            if i % 4 == 1:
                items.insert(0, G("PG", b"abc", LONG))
            out.append(Rec(items, len(items) > 1, seed=i, l_seq=i % 9, ref=i % 4, mref=(i + 1) % 4 if i % 5 else -1,
                           flag=1 if i % 2 else 0, pos=10 + i, name=b"pr%d" % i))
        return out
    a = recs(700)
    b = recs(700)
    b[611] = b[611].moved(4, -1)  # refused by the remap
    c = recs(700)
    c[611] = c[611].moved(9, -1)
    c[140] = Rec([raw(F.aux_a("RG", b"x"), "group_nonstring")], error="ClassCastException", ref=1)
    up, pg, rg = MAPS["up"], (1, TABLE_PG), (1, TABLE_RG)
    return [ProductCase("product-clean", a, up, pg, rg, -1), ProductCase("product-refused", b, up, pg, rg, 611),
            ProductCase("product-group_error_first", c, up, pg, rg, 611, ("ClassCastException", 140))]


_CACHE = {}


def cached(fn):
    if fn not in _CACHE:
        _CACHE[fn] = fn()
    return _CACHE[fn]
