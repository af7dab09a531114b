"""Crafted records for the read-name / CIGAR keyed consumers (csrc/hbam_consumers.hip):
hbam_summarize_ranges (SummarizeRecordReader, Summarize.java:693-755), hbam_name_order (FixMateMapper's
shuffle, FixMate.java:209-221) and hbam_fixmate (FixMateReducer, FixMate.java:225-277, with htsjdk's
SamPairUtil.setMateInfo and BAMRecordCodec.encode behind it), whose other inputs are seeded random
records and small_pe.bam.

Every case declares its own outcome from pieces, not by running the oracle and not by parsing bytes:
  * a Summarize case lists its range tuples (key, beg, end, rev, record) and the status;
  * a name-order case lists the permutation;
  * a FixMate case lists its key groups in shuffle order; every group lists its records in input order
    and its writes (record, mate or None, role), and every mated write states the fixed fields
    (W: refID, pos, bin, flag, mate refID, mate pos, TLEN) and the MQ value it is written with; the
    expected bytes are rebuilt from these pieces (the aux items' re-typed forms, MC dropped, MQ placed).
    TLEN and the recomputed bin are literals or a formula of the generator's own parameters.
test_consumer_model.py holds the oracle, and a second reading of the rules, to these declarations and to
hand-written literals; test_consumer_gpu.py holds the device to the oracle.

What the cases cannot reach, and say so:
  * the recomputed bin's coarser levels: only an unmapped read gets its bin recomputed (setAlignmentStart
    is called on it alone), its alignment end is 0, so the span is one base and reg2bin answers at the
    finest level, 4681 + (pos >> 14).  From pos 2^29 on that number lies past the last bin of the scheme
    (37448); from pos 60855 << 14 on it no longer fits the u16 field and is cut to its low 16 bits.
  * an MQ rewritten to a wider value: MQ is written from a MAPQ byte, so as 'c' or 'C' with one value
    byte, and no aux value is shorter than one byte.  Same size (c -> C) and narrower (i, S, Z -> c) are
    placed.
  * a recomputed bin at pos INT32_MAX: pos + 1 wraps there and reg2bin's end - 1 has no defined value in
    the oracle's C; INT32_MAX positions are placed in the mapped-mapped arm only, which keeps the bin.
"""
import struct

import f4_records as F
import merge_cases as M

I32_MIN, I32_MAX = M.I32_MIN, M.I32_MAX
WG = 256  # F4_WG
EFORMAT, EREFID, EINDEX, EMORE, ETRUNC = -3, -6, -13, -12, -2  # include/hbam.h
M_, I_, D_, N_, S_, H_, P_, EQ_, X_ = range(9)  # CIGAR op codes


def cached(fn):
    return M.cached(fn)


# ---- Summarize ----------------------------------------------------------------------------------------------
class SumCase:
    """recs; ranges = (key, beg, end, rev, record) as declared; status; split_status = dv->status"""

    def __init__(self, cid, recs, ranges, status=0, split_status=0, about=""):
        self.id, self.recs, self.ranges, self.status, self.split_status, self.about = cid, list(recs), list(ranges), status, split_status, about


def _k(ref, com):
    """getKey0 for a centre that is not negative"""
    assert com >= 0
    return (ref << 32) | com


def _m(i, ref=1, pos=9, n=4, flag=0):
    """a plain mapped record: nM at pos -> one range"""
    return F.record(b"s%d" % i, flag=flag, ref=ref, pos=pos, cigar=((n, M_),), l_seq=n, seed=i)


def _m_range(i, ref=1, pos=9, n=4, flag=0):
    return (_k(ref, (2 * pos + 2 + n - 1) // 2), pos + 1, pos + n, 1 if flag & 0x10 else 0, i)


OP9 = [(4 << 4) | M_, (3 << 4) | 9]
BIG = (1 << 28) - 1


def sum_range_cases():
    out = []
    # every flushing op between two M runs; = and X accumulate like M
    r = F.record(b"fl", flag=0x10, ref=1, pos=99, l_seq=27,
                 cigar=((5, M_), (1, I_), (5, M_), (1, S_), (3, EQ_), (2, X_), (1, H_), (5, M_), (1, P_), (5, M_)))
    out.append(SumCase("flush-I-S-H-P", [r], [(_k(1, 102), 100, 104, 1, 0), (_k(1, 107), 105, 109, 1, 0), (_k(1, 112), 110, 114, 1, 0),
                                               (_k(1, 117), 115, 119, 1, 0), (_k(1, 122), 120, 124, 1, 0)]))
    # D directly followed by N: the D flushes, the N finds b == e and only moves on
    r = F.record(b"dn", ref=2, pos=99, cigar=((5, M_), (2, D_), (3, N_), (5, M_)), l_seq=10)
    out.append(SumCase("D-then-N", [r], [(_k(2, 102), 100, 104, 0, 0), (_k(2, 112), 110, 114, 0, 0)]))
    # leading D / N before the first M: nothing to flush, the range starts behind them
    r = F.record(b"ld", ref=0, pos=0, cigar=((3, D_), (2, N_), (1, M_)), l_seq=1)
    out.append(SumCase("leading-D-N", [r], [(_k(0, 6), 6, 6, 0, 0)]))
    # start 0 (pos -1) is kept; an even sum and an odd sum of a one- and a two-base range
    out.append(SumCase("start-0", [F.record(b"z", ref=3, pos=-1, cigar=((2, M_),), l_seq=2)], [(_k(3, 0), 0, 1, 0, 0)]))
    # a centre of mass whose b + ee is negative and odd: e wraps past INT32_MAX.  b = 2^31 - 10, 20M:
    # ee = b + 19 - 2^32 = -2147483639, b + ee = -1, and -1 / 2 is 0 in Java (floor would give -1)
    r = F.record(b"w", ref=5, pos=I32_MAX - 10, cigar=((20, M_),), l_seq=20)
    out.append(SumCase("centre-minus-one", [r], [(_k(5, 0), I32_MAX - 9, -2147483639, 0, 0)]))
    # a negative centre in the first range, then two more ranges.  b = 2013265920, one M of 2^27 + 2:
    # ee = -2147483647, b + ee = -134217727, centre -67108863 (floor: -67108864); the OR of getKey0
    # sign-extends it over refID 7, and the later keys keep that high word: second range
    # (-2147483644, -2147483641), sum -4294967285, centre -2147483642; eight N of 2^28 - 1 and one of 10
    # bring b to 10, third range (10, 13), centre 11 under the high word 0xffffffff
    r = F.record(b"n", ref=7, pos=2013265919, l_seq=8,
                 cigar=((134217730, M_), (2, D_), (4, M_)) + ((BIG, N_),) * 8 + ((10, N_), (4, M_)))
    out.append(SumCase("centre-negative-then-more", [r], [(-67108863, 2013265920, -2147483647, 0, 0),
                                                            (-2147483642, -2147483644, -2147483641, 0, 0),
                                                            (-(1 << 32) + 11, 10, 13, 0, 0)]))
    # records that are skipped, a bad CIGAR included: unmapped with op 9, unplaced with a CIGAR past the
    # record, start < 0 without a CIGAR
    ovr = bytearray(F.overrun_record("cigar"))
    struct.pack_into("<i", ovr, 4, -1)
    recs = [_m(0), F.record(b"u", flag=4, ref=1, pos=5, raw_ops=OP9), bytes(ovr), F.record(b"neg", ref=1, pos=-2, cigar=(), l_seq=0),
            F.record(b"u2", flag=4, ref=-1, pos=-1, cigar=(), l_seq=0), _m(5, flag=0x10)]
    out.append(SumCase("skipped-with-bad-cigar", recs, [_m_range(0), _m_range(5, flag=0x10)]))
    return out


def sum_error_cases():
    out = []
    lead = [_m(0, pos=20), _m(1, ref=2, pos=30, n=7)]
    kept = [_m_range(0, pos=20), _m_range(1, ref=2, pos=30, n=7)]
    tail = [_m(3)]
    # a mapped read without a CIGAR, 0M, and only non-range ops: ranges.get(0) on an empty list
    for cid, cig in (("no-cigar", ()), ("0M", ((0, M_),)), ("only-S-I", ((5, S_), (3, I_)))):
        out.append(SumCase("empty-" + cid, lead + [F.record(b"e", ref=1, pos=50, cigar=cig, l_seq=0)] + tail, kept, EINDEX))
    # op 9 behind a flushed range: the record's own ranges are not delivered
    out.append(SumCase("op9-after-range", lead + [F.record(b"o", ref=1, pos=50, raw_ops=[(4 << 4) | M_, (1 << 4) | I_, (3 << 4) | 9])] + tail,
                       kept, EREFID))
    out.append(SumCase("overrun", lead + [F.overrun_record("cigar")] + tail, kept, EFORMAT))
    out.append(SumCase("first-record-raises", [F.record(b"o", ref=1, pos=50, raw_ops=OP9)] + tail, [], EREFID))
    return out


RACE = {"op-first": ((300, 1), (520, 2), (770, 3)), "empty-first": ((270, 2), (520, 1), (780, 3)),
        "overrun-first": ((257, 3), (515, 1), (770, 2))}
KIND_STATUS = {1: EREFID, 2: EINDEX, 3: EFORMAT}


def sum_race_case(name):
    """kinds 1, 2 and 3 in three workgroups of k_sum_count: the first record wins whatever its kind, and
    the ranges of the records before it stand.  Skipped records with a bad CIGAR stand before it."""
    at = dict(RACE[name])
    bad = {1: F.record(b"x", ref=1, pos=50, raw_ops=OP9), 2: F.record(b"x", ref=1, pos=50, cigar=((5, S_),), l_seq=5),
           3: F.overrun_record("cigar")}
    recs, ranges = [], []
    first = min(at)
    for i in range(800):
        if i in at:
            recs.append(bad[at[i]])
        elif i % 50 == 7:
            recs.append(F.record(b"u", flag=4, ref=1, pos=5, raw_ops=OP9))
        else:
            recs.append(_m(i, ref=i % 3, pos=i, n=1 + i % 5, flag=0x10 if i % 2 else 0))
            if i < first:
                ranges.append(_m_range(i, ref=i % 3, pos=i, n=1 + i % 5, flag=0x10 if i % 2 else 0))
    return SumCase("race-" + name, recs, ranges, KIND_STATUS[at[first]])


def sum_status_cases():
    """dv->status: HBAM_EMORE (a window that is not the split's last) is no exception, another status is
    the base reader's and is carried, a raised error overrides it; n = 0"""
    ok, rg = [_m(0), _m(1, pos=40)], [_m_range(0), _m_range(1, pos=40)]
    bad = ok + [F.record(b"x", ref=1, pos=50, raw_ops=OP9)]
    return [SumCase("status-more", ok, rg, 0, EMORE), SumCase("status-trunc", ok, rg, ETRUNC, ETRUNC),
            SumCase("status-overridden", bad, rg, EREFID, ETRUNC), SumCase("status-more-raised", bad, rg, EREFID, EMORE),
            SumCase("n0", [], [], 0, 0), SumCase("n0-trunc", [], [], ETRUNC, ETRUNC), SumCase("n0-more", [], [], 0, EMORE)]


def summarize_cases():
    return sum_range_cases() + sum_error_cases() + [sum_race_case(n) for n in RACE] + sum_status_cases()


def summarize_product():
    """the range cases in one run, then a raising case, then records that are never reached"""
    parts = sum_range_cases() + [sum_error_cases()[3]] + [sum_range_cases()[0]]
    recs, ranges, status = [], [], 0
    for c in parts:
        if status == 0:
            ranges += [(k, b, e, r, i + len(recs)) for k, b, e, r, i in c.ranges]
            status = c.status
        recs += c.recs
    return [SumCase("product", recs, ranges, status)]


# ---- name order ---------------------------------------------------------------------------------------------
L0 = None  # a record with l_read_name 0


class NameCase:
    """names in input order (L0: l_read_name 0) and the declared permutation"""

    def __init__(self, cid, names, perm):
        self.id, self.names, self.perm = cid, list(names), list(perm)

    def recs(self, prefix=b""):
        out = []
        for i, nm in enumerate(self.names):
            kw = dict(flag=i % 3, ref=i % 4, pos=i, cigar=((3, M_),), l_seq=3, seed=i)
            out.append(F.record_l0(**kw) if nm is L0 else F.record(prefix + nm, **kw))
        return out


X253 = b"x" * 253


def name_cases():
    out = [
        # zero padding of the last chunk must not collide with a real zero byte
        NameCase("embedded-nul", [b"AB", b"A\0C", b"A\0", b"A"], [3, 2, 1, 0]),
        NameCase("embedded-nul-chunk-edge", [b"ABCDEFG\0", b"ABCDEFG", b"ABCDEFG\0\0", b"ABCDEFGH"], [1, 0, 2, 3]),
        # byte 7 (the last of chunk 0) against byte 8 (the first of chunk 1)
        NameCase("byte7-byte8", [b"ABCDEFGZA", b"ABCDEFGAZ", b"ABCDEFGAA", b"ABCDEFGZ"], [2, 1, 3, 0]),
        # one length only: the length sort is skipped
        NameCase("same-length", [b"bbbbb", b"aaaaa", b"bbbba", b"aaaaa"], [1, 3, 2, 0]),
        NameCase("high-bytes", [b"\xff", b"\x7f", b"\x80", b"\x80\x00", b"\x7f\xff"], [1, 4, 2, 3, 0]),
        # l_read_name 0 and 1 are both the empty name: one key, input order
        NameCase("empty-l0-l1", [b"A", L0, b"", L0, b""], [1, 2, 3, 4, 0]),
        # every name empty: no sort runs, the order is the input's (more than one workgroup)
        NameCase("all-empty", [L0 if i % 3 == 0 else b"" for i in range(300)], range(300)),
        # 254-byte names (l_read_name 255): 32 chunks, the last one 6 bytes
        NameCase("len-254", [X253 + b"b", X253 + b"a", X253, b"y", X253 + b"a"], [2, 1, 4, 0, 3]),
        NameCase("n1", [b"solo"], [0]),
        NameCase("n1-empty", [L0], [0]),
        NameCase("n0", [], []),
        # equal names keep the input order across workgroups
        NameCase("ties-wide", [(b"b", b"a", b"c")[i % 3] for i in range(600)],
                 [i for r in (1, 0, 2) for i in range(600) if i % 3 == r]),
    ]
    return out


def name_product():
    """all-empty first (the empty name sorts before every other), then every case under its own prefix,
    the input in reverse case order.  len-254 stands alone: its names take no prefix."""
    cases = [c for c in name_cases() if c.id not in ("all-empty", "len-254") and L0 not in c.names]
    empty = NameCase("e", [L0, b"", L0], [0, 1, 2])
    blocks = [(empty, b"")] + [(c, b"%02d." % k) for k, c in enumerate(cases)]
    names, base, starts = [], 0, []
    for c, pre in reversed(blocks):
        starts.append(len(names))
        names += [L0 if n is L0 else pre + n for n in c.names]
    starts.reverse()
    perm = [s + p for (c, _), s in zip(blocks, starts) for p in c.perm]
    return [NameCase("product", names, perm)]


# ---- FixMate ------------------------------------------------------------------------------------------------
class W:
    """what a mated write carries: the fixed fields setMateInfo leaves and the MQ value (None: removed)"""

    def __init__(self, ref, pos, bin_, flag, nref, npos, tlen, mq):
        self.ref, self.pos, self.bin, self.flag, self.nref, self.npos, self.tlen, self.mq = ref, pos, bin_, flag, nref, npos, tlen, mq


def MQ(typ="C", v=9):
    """an MQ the record already carries"""
    return M.Item("mq", F.aux_z("MQ", v) if typ == "Z" else F.aux_int("MQ", typ, v), None, typ=typ)


def MC(s="5M"):
    return M.Item("mc", F.aux_z("MC", s), b"")


def mq_bytes(v):
    """MQ as BinaryTagCodec writes a MAPQ: 'c' up to 127, 'C' from 128"""
    assert 0 <= v <= 255
    return b"MQ" + (b"c" if v <= 127 else b"C") + bytes([v])


SEQ5, SEQ5_OUT, QUAL5 = b"\x12\x48\x8f", b"\x12\x48\x80", b"\x01\x02\x03\x04\x05"


class Rec:
    """One record from pieces.  The default is five bases with a pad nibble of 0xf and real qualities, so
    every mated write shows whether the pad is cleared."""

    def __init__(self, flag=1, ref=0, pos=0, mapq=30, cigar=((5, M_),), l_seq=5, items=(), bin_=4681, nref=-1, npos=-1,
                 tlen=0, seq=None, qual=None, l0=False, bad=False, raw=None):
        if seq is None:
            seq = (SEQ5 * l_seq)[:(l_seq + 1) // 2 - 1] + (b"\x8f" if l_seq & 1 else b"\x84") if l_seq else b""
        if qual is None:
            qual = (QUAL5 * l_seq)[:l_seq]
        self.flag, self.ref, self.pos, self.mapq, self.cigar, self.l_seq = flag, ref, pos, mapq, tuple(cigar), l_seq
        self.items, self.bin, self.nref, self.npos, self.tlen = list(items), bin_, nref, npos, tlen
        self.seq, self.qual, self.l0, self.bad, self.raw = bytes(seq), bytes(qual), l0, bad, raw

    @property
    def unmapped(self):
        return bool(self.flag & 4)

    @property
    def neg(self):
        return bool(self.flag & 0x10)

    def _build(self, name, aux, seq, qual, ref, pos, bin_, flag, nref, npos, tlen):
        kw = dict(flag=flag, ref=ref, pos=pos, mapq=self.mapq, cigar=self.cigar, l_seq=self.l_seq, aux=aux, nref=nref, npos=npos,
                  tlen=tlen, bin_=bin_, seq=seq, qual=qual)
        return F.record_l0(**kw) if self.l0 else F.record(name, **kw)

    def input(self, name):
        if self.raw is not None:
            return self.raw
        return self._build(name, b"".join(i.src for i in self.items), self.seq, self.qual, self.ref, self.pos, self.bin, self.flag,
                           self.nref, self.npos, self.tlen)

    def aux_out(self, mq):
        out, done = b"", False
        for it in self.items:
            if it.kind == "mc":
                continue
            if it.kind == "mq":   # replaced where it stands, or taken out
                out += mq_bytes(mq) if mq is not None else b""
                done = True
            else:
                out += it.dst
        if not done and mq is not None:
            out += mq_bytes(mq)
        return out

    def mated(self, name, w):
        """BAMRecordCodec.encode after setMateInfo, as declared by w"""
        seq = bytearray(self.seq)
        if self.l_seq & 1:
            seq[-1] &= 0xF0
        qual = b"\xff" * self.l_seq if self.qual[:1] == b"\xff" else self.qual
        return self._build(name, self.aux_out(w.mq), seq, qual, w.ref, w.pos, w.bin, w.flag, w.nref, w.npos, w.tlen)


def _mate_bits(flag, mate_neg, mate_unmapped):
    return (flag & ~0x28) | (0x20 if mate_neg else 0) | (8 if mate_unmapped else 0)


def want_mm(a, b, tlen, neg_tlen=None):
    """both mapped; a is setMateInfo's rec1 (the earlier of the two in the shuffle) and gets tlen"""
    assert not a.unmapped and not b.unmapped
    if neg_tlen is None:
        neg_tlen = -tlen
    ba, bb = (a.bin if a.ref >= 0 else 0), (b.bin if b.ref >= 0 else 0)
    return (W(a.ref, a.pos, ba, _mate_bits(a.flag, b.neg, False), b.ref, b.pos, tlen, b.mapq),
            W(b.ref, b.pos, bb, _mate_bits(b.flag, a.neg, False), a.ref, a.pos, neg_tlen, a.mapq))


def want_mu(m, u, bin_u):
    """one mapped: the unmapped read moves to its mate's place and gets bin_u (0 when unplaced)"""
    assert not m.unmapped and u.unmapped
    return (W(m.ref, m.pos, m.bin if m.ref >= 0 else 0, _mate_bits(m.flag, u.neg, True), m.ref, m.pos, 0, None),
            W(m.ref, m.pos, bin_u, _mate_bits(u.flag, m.neg, False), m.ref, m.pos, 0, m.mapq))


def want_uu(a, b):
    assert a.unmapped and b.unmapped
    return (W(-1, -1, 0, _mate_bits(a.flag, b.neg, True), -1, -1, 0, None),
            W(-1, -1, 0, _mate_bits(b.flag, a.neg, True), -1, -1, 0, None))


class Group:
    """one key group: its records in input order, its writes (record, mate or None, role) in the
    reducer's order, and wants[(record, role)] = W for every mated write"""

    def __init__(self, name, recs, writes, wants):
        self.name, self.recs, self.writes, self.wants = name, list(recs), list(writes), dict(wants)
        assert {(s, ro) for s, m, ro in self.writes if m is not None} == set(self.wants)


def pair(name, a, b, wa, wb):
    return Group(name, [a, b], [(0, 1, 1), (1, 0, 2)], {(0, 1): wa, (1, 2): wb})


class FmCase:
    """groups in shuffle (name) order; `order`: the input order as (group, record) pairs, by default the
    groups reversed.  refused: a record's fields overrun its block_size, the job fails in the mapper and
    nothing is written.  A mated write of a record marked bad (aux that does not parse) fails the job
    there: the writes before it stand."""

    def __init__(self, cid, groups, order=None, refused=False, about=""):
        self.id, self.groups, self.refused, self.about = cid, list(groups), refused, about
        if order is None:
            order = [(g, k) for g in reversed(range(len(self.groups))) for k in range(len(self.groups[g].recs))]
        self.order = list(order)
        assert sorted(self.order) == [(g, k) for g in range(len(self.groups)) for k in range(len(self.groups[g].recs))]
        for g in range(len(self.groups)):  # a group's records keep their order in the input
            ks = [k for gg, k in self.order if gg == g]
            assert ks == sorted(ks)

    def build(self, prefix=b"", base=0):
        """-> (records in input order, plan [(src, mate or None, role)], expected payloads), all writes"""
        index = {gk: base + i for i, gk in enumerate(self.order)}
        recs = [self.groups[g].recs[k].input(prefix + self.groups[g].name) for g, k in self.order]
        plan, outs = [], []
        for g, grp in enumerate(self.groups):
            for s, m, ro in grp.writes:
                plan.append((index[g, s], None if m is None else index[g, m], ro))
                r = grp.recs[s]
                outs.append(r.input(prefix + grp.name) if m is None else r.mated(prefix + grp.name, grp.wants[s, ro]))
        return recs, plan, outs

    def fails_at(self):
        """the first write that fails the job, or None"""
        k = 0
        for grp in self.groups:
            for s, m, ro in grp.writes:
                if m is not None and grp.recs[s].bad:
                    return k
                k += 1
        return None

    def declared(self, prefix=b""):
        """-> dict(recs, plan, outs, status, n_groups) of the run as it ends"""
        recs, plan, outs = self.build(prefix)
        if self.refused:
            return dict(recs=recs, plan=[], outs=[], status=EFORMAT, n_groups=0)
        stop = self.fails_at()
        if stop is not None:
            return dict(recs=recs, plan=plan[:stop], outs=outs[:stop], status=EFORMAT, n_groups=len(self.groups))
        return dict(recs=recs, plan=plan, outs=outs, status=0, n_groups=len(self.groups))

    def writes(self):
        """(group, record, write, W or None) of every write that stands"""
        stop, k, out = self.fails_at(), 0, []
        for grp in self.groups:
            for s, m, ro in grp.writes:
                if self.refused or (stop is not None and k >= stop):
                    return out
                out.append((grp, grp.recs[s], (s, m, ro), grp.wants.get((s, ro))))
                k += 1
        return out


def _fwd(pos, **kw):
    return Rec(flag=kw.pop("flag", 0x41), pos=pos, **kw)


def retype_case():
    """every value of M.INT_VALUES in every type that holds it, on both records of a pair; MQ written
    from MAPQ 0, 127, 128 and 255"""
    combos = [(t, v) for v in M.INT_VALUES for t, (lo, hi) in M.HOLDS.items() if lo <= v <= hi]
    groups = []
    for k, half in enumerate((combos[::2], combos[1::2])):
        items = [M.I("%c%c" % (65 + j // 26, 97 + j % 26), t, v) for j, (t, v) in enumerate(half)]
        a, b = _fwd(100, items=items, mapq=0), Rec(0x81, pos=100, items=list(reversed(items)), mapq=127)
        groups.append(pair(b"int%d" % k, a, b, *want_mm(a, b, 1)))
    for k, (qa, qb) in enumerate(((0, 127), (128, 255), (255, 0), (127, 128))):
        a, b = _fwd(10, mapq=qa, items=[MQ("C", 77)]), Rec(0x81, pos=10, mapq=qb)
        groups.append(pair(b"mapq%d" % k, a, b, *want_mm(a, b, 1)))
    return FmCase("retype", groups)


def placement_case():
    """where MQ and MC stand among the tags, twice, alone, of another type, narrower; MQ taken out from
    between two tags; no aux at all"""
    x, y = M.I("XA", "i", 300), M.raw(F.aux_z("XZ", "str"))

    def xy():
        return M.I("XA", "i", 300), M.raw(F.aux_z("XZ", "str"))
    layouts = {
        "first": [MQ(), *xy()], "middle": [x, MQ(), y], "last": [*xy(), MQ()], "twice": [MQ("c", 1), x, MQ("C", 200)],
        "mc-twice": [MC("1M"), x, MC("22M")], "mc-only": [MC()], "mc-mq-adjacent": [MC(), MQ(), MC(), y],
        "mq-Z": [x, MQ("Z", "text"), y], "mq-Z-empty": [MQ("Z", "")], "mq-i-narrower": [x, MQ("i", 70000), y],
        "mq-S-narrower": [MQ("S", 300), y], "mq-c-to-C": [x, MQ("c", -3)], "mq-A": [M.Item("mq", F.aux_a("MQ", b"!"), None, typ="A"), y],
        "none": [], "no-mq": [x, y],
    }
    groups = []
    for k, (name, items) in enumerate(sorted(layouts.items())):
        # written with the mate's MAPQ 200 ('C'), then with 7 ('c')
        for q in (200, 7):
            a, b = _fwd(10 + k, items=items, mapq=1), Rec(0x81, pos=50, mapq=q, items=[MC("9M")] if k % 2 else [])
            groups.append(pair(b"set-%s-%d" % (name.encode(), q), a, b, *want_mm(a, b, 50 - 10 - k + 1)))
        # taken out: the mapped read of a mapped / unmapped pair
        m, u = _fwd(10 + k, items=items, ref=1), Rec(0x85, ref=-1, pos=-1, items=items)
        wm, wu = want_mu(m, u, 4681)
        groups.append(pair(b"rm-%s" % name.encode(), m, u, wm, wu))
    groups.sort(key=lambda g: g.name)
    return FmCase("placement", groups)


def tlen_case():
    groups = []

    def add(name, a, b, tlen, neg=None):
        groups.append(pair(name, a, b, *want_mm(a, b, tlen, neg)))
    rev10 = dict(cigar=((10, M_),), l_seq=10)
    # p2 == p1 in the four strand combinations: 5' end 100 on both sides, +1 for rec1
    add(b"tie-ff", _fwd(99), Rec(0x81, pos=99), 1)
    add(b"tie-fr", _fwd(99), Rec(0x91, pos=90, **rev10), 1)
    add(b"tie-rf", _fwd(90, flag=0x51, **rev10), Rec(0x81, pos=99), 1)
    add(b"tie-rr", _fwd(90, flag=0x51, **rev10), Rec(0x91, pos=95), 1)
    # one base apart, both ways
    add(b"near-up", _fwd(99), Rec(0x81, pos=100), 2)
    add(b"near-down", _fwd(100), Rec(0x81, pos=99), -2)
    # the reference length counts M D N = X and skips I S H P: 5 + 4 + 3 + 2 + 1 + 5 = 20, end 219
    ops = dict(cigar=((3, H_), (2, S_), (5, M_), (2, I_), (4, N_), (3, EQ_), (2, X_), (6, P_), (1, D_), (5, M_), (2, S_), (1, H_)), l_seq=21)
    add(b"ops-second", _fwd(99), Rec(0x91, pos=199, **ops), 120)
    add(b"ops-first", _fwd(199, flag=0x51, **ops), Rec(0x81, pos=99), -120)
    add(b"ops-both", _fwd(199, flag=0x51, **ops), Rec(0x91, pos=299, **ops), 101)
    # different references: 0, whatever the input says
    add(b"refs-differ", _fwd(99, ref=1, tlen=777), Rec(0x81, ref=2, pos=500, tlen=-777), 0)
    # a reverse read without a CIGAR ends one base before its start
    add(b"rev-no-cigar", _fwd(99), Rec(0x91, pos=99, cigar=(), l_seq=0), -2)
    add(b"rev-no-cigar-first", _fwd(99, flag=0x51, cigar=(), l_seq=0), Rec(0x81, pos=99), 2)
    # start INT32_MAX against start 1
    add(b"wrap-max-start", _fwd(I32_MAX - 1), Rec(0x81, pos=0), -I32_MAX)
    # pos INT32_MAX: the start wraps to INT32_MIN = p1, and -p1 is INT32_MIN again: 1 - p1 + 1 wraps
    add(b"wrap-p1-min", _fwd(I32_MAX), Rec(0x81, pos=0), I32_MIN + 2)
    add(b"wrap-p2-min", _fwd(0), Rec(0x81, pos=I32_MAX), I32_MAX - 1)   # p2 = INT32_MIN: p2 - 1 - 1 wraps
    # p1 = INT32_MIN, p2 = -1: TLEN 2^31 wraps to INT32_MIN, and so does its negation
    add(b"wrap-tlen-min", _fwd(I32_MAX), Rec(0x81, pos=-2), I32_MIN, I32_MIN)
    # the end of a reverse read wraps: start INT32_MAX - 4, 10M, end INT32_MIN + 4
    add(b"wrap-end", _fwd(0), Rec(0x91, pos=I32_MAX - 5, **rev10), I32_MIN + 2)
    # p2 - p1 wraps: 2000000000 - (-1999999999) + 1 = 4000000000 - 2^32
    add(b"wrap-diff", _fwd(-2000000000), Rec(0x81, pos=1999999999), -294967296)
    # the mapped-mapped arm keeps the input bin, garbage and unplaced included
    add(b"bin-kept", _fwd(99, bin_=0xBEEF), Rec(0x81, pos=99, bin_=0), 1)
    add(b"bin-unplaced", _fwd(99, ref=-1, bin_=0xBEEF), Rec(0x81, ref=-1, pos=99, bin_=7), 1)
    groups.sort(key=lambda g: g.name)
    return FmCase("tlen", groups)


BIN_AT = [(0, 4681), (16383, 4681), (16384, 4682), ((1 << 29) - 1, 37448), (1 << 29, 37449), (60855 << 14, 0),
          ((60855 << 14) - 1, 65535), (1 << 30, 4681), (-1, 4680)]


def bin_case():
    """the unmapped read placed at its mate's position: 4681 + (pos >> 14), cut to 16 bits"""
    groups = []
    for k, (pos, want) in enumerate(BIN_AT):
        for first in ("m", "u"):
            m = Rec(0x41 | (0x10 if k % 2 else 0), ref=3, pos=pos, bin_=0x1234, mapq=128 + k)
            u = Rec(0x85, ref=k % 3 - 1, pos=77, bin_=0x4321, nref=5, npos=6, tlen=9, items=[MQ("c", 5)])
            wm, wu = want_mu(m, u, want)
            groups.append(pair(b"at%d-%s" % (k, first.encode()), *((m, u, wm, wu) if first == "m" else (u, m, wu, wm))))
    # a "mapped" mate without a reference: the unmapped read is unplaced too, bin 0
    m, u = Rec(0x41, ref=-1, pos=500, bin_=0x1234), Rec(0x85, ref=2, pos=77, bin_=0x4321)
    groups.append(pair(b"unplaced", m, u, *want_mu(m, u, 0)))
    # both unmapped: refID -1, pos -1, bin 0, MQ removed, strands crossed
    a, b = Rec(0x45 | 0x10, ref=2, pos=40, bin_=0x1234, tlen=5, items=[MQ(), MC()]), Rec(0x85, ref=1, pos=77, bin_=0x4321, nref=1, npos=3)
    groups.append(pair(b"uu", a, b, *want_uu(a, b)))
    groups.sort(key=lambda g: g.name)
    return FmCase("bin", groups)


def seqqual_case():
    groups = []
    shapes = {
        "l0": dict(l_seq=0, cigar=()),
        "l1-pad": dict(l_seq=1, cigar=((1, M_),), seq=b"\x2f", qual=b"\x07"),
        "l1-ff": dict(l_seq=1, cigar=((1, M_),), seq=b"\x2f", qual=b"\xff"),
        "l2-even": dict(l_seq=2, cigar=((2, M_),), seq=b"\x2f", qual=b"\x07\x08"),   # an even length keeps its low nibble
        "l5-ff-first": dict(qual=b"\xff\x01\x02\x03\x04"),                             # all rewritten to 0xff
        "l5-ff-later": dict(qual=b"\x01\xff\xff\xff\xff"),                             # kept
        "l5-all-ff": dict(qual=b"\xff" * 5),
    }
    for name, kw in sorted(shapes.items()):
        a, b = _fwd(99, **kw), Rec(0x81, pos=99, **kw)
        groups.append(pair(name.encode(), a, b, *want_mm(a, b, 1)))
        m, u = _fwd(99, **kw), Rec(0x85, pos=5, **kw)
        groups.append(pair(name.encode() + b"-mu", m, u, *want_mu(m, u, 4681)))
    return FmCase("seq-qual", groups)


# the reducer's writes per shape of a key group (P primary, S secondary), read off FixMate.java:241-276:
# (record, mate, role).  "PS" and "PSS" are the quirk: the inner loop ends on the last secondary, which
# has been written already and is then mated and written again.
SHAPES = {
    "P": [(0, None, 0)], "S": [(0, None, 0)], "SS": [(0, None, 0), (1, None, 0)],
    "PP": [(0, 1, 1), (1, 0, 2)],
    "PS": [(1, None, 0), (0, 1, 1), (1, 0, 2)],
    "PSS": [(1, None, 0), (2, None, 0), (0, 2, 1), (2, 0, 2)],
    "SPSP": [(0, None, 0), (2, None, 0), (1, 3, 1), (3, 1, 2)],
    "PSSP": [(1, None, 0), (2, None, 0), (0, 3, 1), (3, 0, 2)],
    "PPP": [(0, 1, 1), (1, 0, 2), (2, None, 0)],
    "PPPP": [(0, 1, 1), (1, 0, 2), (2, 3, 1), (3, 2, 2)],
    "PSPSP": [(1, None, 0), (0, 2, 1), (2, 0, 2), (3, None, 0), (4, None, 0)],
    "SPPS": [(0, None, 0), (1, 2, 1), (2, 1, 2), (3, None, 0)],
}


def shape_group(name, shape, writes=None, items=None, bad_at=()):
    """records 10 bases apart on one reference, forward: a mated pair (i, j) has TLEN 10 (j - i) + 1"""
    recs = [Rec(1 | (0x100 if ch == "S" else 0), ref=1, pos=100 + 10 * j, mapq=20 + j, bad=j in bad_at,
                items=[M.Item("malformed", b"NMq\1", b"")] if j in bad_at else (items if items is not None else [M.I("NM", "S", j), MC("30M")]))
            for j, ch in enumerate(shape)]
    writes = SHAPES[shape] if writes is None else writes
    wants = {}
    for s, m, ro in writes:
        if ro == 1:
            wants[s, 1], wants[m, 2] = want_mm(recs[s], recs[m], 10 * (m - s) + (1 if m > s else -1))
    return Group(name, recs, writes, wants)


def shapes_case():
    names = sorted(SHAPES)
    return FmCase("shapes", [shape_group(b"sh-" + s.encode(), s) for s in names])


def tiny_cases():
    one = Rec(0x41, items=[M.Item("malformed", b"XYq\0", b"")], bad=True)
    return [FmCase("n0", []), FmCase("n1", [Group(b"one", [Rec(0x41)], [(0, None, 0)], {})]),
            FmCase("n1-l0", [Group(b"", [Rec(0x41, l0=True)], [(0, None, 0)], {})]),
            # l_read_name 0 and 1 are one key group: SPP -> S written, the two primaries mated
            FmCase("empty-names", [Group(b"", [Rec(0x101, l0=True), Rec(0x41, pos=5), Rec(0x81, pos=9, l0=True)],
                                         [(0, None, 0), (1, 2, 1), (2, 1, 2)],
                                         dict(zip(((1, 1), (2, 2)), want_mm(Rec(0x41, pos=5), Rec(0x81, pos=9, l0=True), 5)))),
                                   Group(b"\0", [Rec(0x41)], [(0, None, 0)], {})]),
            FmCase("n1-bad-untouched", [Group(b"one", [one], [(0, None, 0)], {})]),
            # the very first write fails: nothing stands
            FmCase("fails-at-0", [pair(b"p", one, Rec(0x81, pos=3), *want_mm(one, Rec(0x81, pos=3), 4)), shape_group(b"zz", "PP")])]


def many_groups_case(n=600):
    """more than 256 key groups (k_fm_plan's second and third workgroup), each one pair: group 128's head
    is position 256 of the shuffle, the first lane of k_fm_heads' second workgroup.  The input holds
    every first read, then every second read in reverse."""
    groups = []
    for i in range(n):
        d = i % 7
        a, b = _fwd(100 + i, ref=i % 3, mapq=i % 256, items=[M.I("NM", "i", i)]), Rec(0x81, ref=i % 3, pos=100 + i + d, mapq=(i * 7) % 256)
        groups.append(pair(b"g%04d" % i, a, b, *want_mm(a, b, d + 1)))
    order = [(g, 0) for g in range(n)] + [(g, 1) for g in reversed(range(n))]
    return FmCase("many-groups", groups, order)


def wide_group_case(n=300):
    """one key group wider than a workgroup: P P S repeated; between two small groups"""
    recs = [Rec(0x101 if j % 3 == 2 else 1, ref=2, pos=1000 + j, mapq=j % 256) for j in range(n)]
    writes, wants = [], {}
    for j in range(0, n, 3):
        writes += [(j, j + 1, 1), (j + 1, j, 2), (j + 2, None, 0)]
        wants[j, 1], wants[j + 1, 2] = want_mm(recs[j], recs[j + 1], 2)
    return FmCase("wide-group", [shape_group(b"a", "PP"), Group(b"m", recs, writes, wants), shape_group(b"z", "PSS")])


def untouched_bad_case():
    """aux that does not parse on records that are written as read: a single primary, a secondary, the
    third of three primaries.  Nothing is parsed, nothing fails."""
    return FmCase("bad-untouched", [shape_group(b"p", "P", bad_at=(0,)), shape_group(b"spp", "SPP", [(0, None, 0), (1, 2, 1), (2, 1, 2)], bad_at=(0,)),
                                    shape_group(b"three", "PPP", bad_at=(2,))])


def quirk_bad_case():
    """the quirk with a bad secondary: its first write (as read) stands, the primary's mated write stands,
    its own mated write fails the job"""
    return FmCase("bad-quirk", [shape_group(b"ok", "PP"), shape_group(b"ps", "PS", bad_at=(1,)), shape_group(b"zz", "PP")])


def malformed_cases():
    """every malformed aux shape on the second record of a pair behind a good group: the pair's first
    write stands too"""
    out = []
    for name, aux in M.MALFORMED.items():
        a = _fwd(10)
        b = Rec(0x81, pos=20, items=[M.Item("malformed", aux, b"")], bad=True)
        out.append(FmCase("malformed-" + name, [shape_group(b"ok", "PSSP"), pair(b"p", a, b, *want_mm(a, b, 11)), shape_group(b"zz", "PP")]))
    return out


RACE_AT = (770, 300, 521)


def race_case():
    """400 pairs, 800 writes, three workgroups of k_fm_encode; the writes RACE_AT fail.  The lowest write
    is the job's, and the writes before it stand."""
    groups = []
    for i in range(400):
        bad = [w % 2 for w in RACE_AT if w // 2 == i]
        a, b = _fwd(100 + i, mapq=i % 256), Rec(0x81, pos=100 + i, mapq=255 - i % 256, items=[M.I("NM", "S", i)])
        for r, k in ((a, 0), (b, 1)):
            if k in bad:
                r.items, r.bad = [M.Item("malformed", list(M.MALFORMED.values())[i % len(M.MALFORMED)], b"")], True
        groups.append(pair(b"r%04d" % i, a, b, *want_mm(a, b, 1)))
    return FmCase("race", groups)


def overrun_cases():
    out = []
    for field in ("cigar", "seq"):
        g = shape_group(b"ovr", "P")
        g.recs[0].raw = F.overrun_record(field)
        out.append(FmCase("overrun-" + field, [shape_group(b"a", "PP"), g, shape_group(b"z", "PP")], refused=True))
    g = Group(b"neg", [Rec(0x41, raw=_neg_lseq())], [(0, None, 0)], {})
    out.append(FmCase("overrun-negative-l_seq", [shape_group(b"a", "PP"), g], refused=True))
    return out


def _neg_lseq():
    b = bytearray(F.record(b"neg", flag=0x41, l_seq=4, cigar=((4, M_),)))
    struct.pack_into("<i", b, 20, -1)
    return bytes(b)


def fixmate_cases():
    out = [retype_case(), placement_case(), tlen_case(), bin_case(), seqqual_case(), shapes_case()] + tiny_cases()
    out += [many_groups_case(), wide_group_case(), untouched_bad_case(), quirk_bad_case()] + malformed_cases() + [race_case()] + overrun_cases()
    return out


class FmProduct:
    """cases under distinct name prefixes in one run: the input in reverse case order, the plan in prefix
    order.  `last` may fail: it sorts behind every other, so everything before its failing write stands."""

    def __init__(self, cid, cases, last=None):
        self.id = cid
        blocks = [(c, b"%02d." % k) for k, c in enumerate(cases)] + ([(last, b"zz.")] if last else [])
        base, bases = 0, []
        for c, _ in reversed(blocks):
            bases.append(base)
            base += len(c.order)
        bases.reverse()
        built = [c.build(pre, b0) for (c, pre), b0 in zip(blocks, bases)]
        self.recs = [r for recs, _, _ in reversed(built) for r in recs]
        self.plan = [p for _, plan, _ in built for p in plan]
        self.outs = [o for _, _, outs in built for o in outs]
        self.n_groups = sum(len(c.groups) for c, _ in blocks)
        self.status = 0
        if last is not None and last.fails_at() is not None:
            cut = len(self.plan) - len(built[-1][1]) + last.fails_at()
            self.plan, self.outs, self.status = self.plan[:cut], self.outs[:cut], EFORMAT

    def declared(self):
        return dict(recs=self.recs, plan=self.plan, outs=self.outs, status=self.status, n_groups=self.n_groups)


def fixmate_product():
    clean = [retype_case(), placement_case(), tlen_case(), bin_case(), seqqual_case(), shapes_case(), wide_group_case(), untouched_bad_case(),
             many_groups_case()]
    return [FmProduct("product-clean", clean), FmProduct("product-fails-last", clean[:6], quirk_bad_case())]
