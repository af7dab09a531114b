"""The crafted consumer cases (tests/consumer_cases.py) on the CPU.

  * oracle.summarize_ranges, oracle.name_order and oracle.fixmate return exactly what each case declares,
    alone and in the product runs;
  * a second pure-Python reading of SamPairUtil.setMateInfo, computeInsertSize, computeIndexingBin and
    BAMRecordCodec's tag re-encode (py_fixmate below, next to test_consumers.py_summarize and
    py_reduce_plan, which it imports) agrees with the oracle on every case;
  * known answers written by hand, as hex and literal numbers, pin the oracle to something other than the
    case builder;
  * the cases reach every arm they are there for, computed from the declarations alone, and the arms they
    cannot reach are asserted unreachable with the reason.
test_consumer_gpu.py then holds the three device entry points to the oracle.

What stays unpinned against htsjdk 1.131, because only this restatement exists (the reference holds
FixMate.java:225-277 and Summarize.java:693-755, not htsjdk):
  * the exception class of a layout overrun (a CIGAR or sequence past block_size): reported as
    SAMFormatException / HBAM_EFORMAT;
  * the recomputed bin from pos 2^29 on (past the scheme's last bin) and its cut to 16 bits from
    pos 60855 << 14 on; the bin 4680 of an unmapped read placed at pos -1;
  * an MQ of a non-integer type (MQ:Z, MQ:A) being overwritten in place by the integer MQ, or removed;
  * the type of a value from 256 to 32767: 'S' here (the ladder of the oracle, the kernels and
    merge_cases.INT_RANGES alike); whether htsjdk's getIntegerType answers 's' there cannot be read off
    anything in the reference;
  * a tag present twice: both MQ are rewritten where they stand, both MC are dropped;
  * whether the first write of a pair stands when the second record's attributes do not parse (here it
    does: each write parses its own record; htsjdk's setMateInfo touches both records' attributes
    before either is written);
  * setMateInfo's both-unmapped and one-unmapped arms as a whole (field by field from the published
    behaviour), the absent-quality fill and the pad nibble of an odd-length sequence.
"""
import struct

import numpy as np
import pytest

import consumer_cases as K
import f4_records as F
import merge_cases as M
from test_consumers import _fields, _i32, py_reduce_plan, py_summarize

SUM = K.cached(K.summarize_cases)
SUM_PRODUCT = K.cached(K.summarize_product)
NAME = K.cached(K.name_cases)
NAME_PRODUCT = K.cached(K.name_product)
FM = K.cached(K.fixmate_cases)
FM_PRODUCT = K.cached(K.fixmate_product)


def by_id(cases, cid):
    return next(c for c in cases if c.id == cid)


# ---- the second reading -------------------------------------------------------------------------------------
INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class AuxError(Exception):
    pass


def py_parse_aux(b):
    """-> [(tag, type, value)]: an int for the integer types, the raw value bytes otherwise"""
    out, p = [], 0
    while p < len(b):
        if len(b) - p < 3:
            raise AuxError("tag cut")
        tag, ty = b[p:p + 2], chr(b[p + 2])
        p += 3
        if ty in INT_FMT:
            n = struct.calcsize(INT_FMT[ty])
            if p + n > len(b):
                raise AuxError("value cut")
            out.append((tag, ty, struct.unpack_from(INT_FMT[ty], b, p)[0]))
        elif ty in "Af":
            n = 1 if ty == "A" else 4
            if p + n > len(b):
                raise AuxError("value cut")
            out.append((tag, ty, b[p:p + n]))
        elif ty in "ZH":
            z = b.find(b"\0", p)
            if z < 0:
                raise AuxError("no NUL")
            n = z + 1 - p
            out.append((tag, ty, b[p:p + n]))
        elif ty == "B":
            if p + 5 > len(b):
                raise AuxError("array header cut")
            es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(chr(b[p]))
            if es is None:
                raise AuxError("array subtype")
            n = 5 + es * struct.unpack_from("<I", b, p + 1)[0]
            if p + n > len(b):
                raise AuxError("array cut")
            out.append((tag, ty, b[p:p + n]))
        else:
            raise AuxError("type")
        p += n
    return out


def py_int_tag(tag, v):
    """BinaryTagCodec.getIntegerType as this project states it: by value, the unsigned type wherever the
    value is not negative and the signed type of the same width would hold it too (256 is 'S', not 's')"""
    for ty, lo, hi in (("c", -128, 127), ("C", 128, 255), ("S", 256, 65535), ("s", -32768, -129), ("i", -(1 << 31), (1 << 31) - 1),
                       ("I", 1 << 31, (1 << 32) - 1)):
        if lo <= v <= hi:
            return tag + ty.encode() + struct.pack(INT_FMT[ty], v)
    raise ValueError(v)


class SamRec:
    """a SAMRecord as setMateInfo sees it"""

    def __init__(self, b):
        (self.bs, self.ref, self.pos, self.lrn, self.mapq, self.bin, self.nc, self.flag, self.lseq, self.nref, self.npos,
         self.tlen) = struct.unpack_from("<iiiBBHHHiiii", b)
        self.b = bytes(b)
        self.cigar = struct.unpack_from("<%dI" % self.nc, b, 36 + self.lrn)
        self.bin_known = True
        self.mq = "keep"

    unmapped = property(lambda s: bool(s.flag & 4))
    neg = property(lambda s: bool(s.flag & 0x10))
    start = property(lambda s: _i32(s.pos + 1))

    @property
    def end(self):  # getAlignmentEnd
        if self.unmapped:
            return 0
        n = 0
        for c in self.cigar:
            if "MIDNSHP=X"[c & 15] in "MDN=X":
                n = _i32(n + (c >> 4))
        return _i32(_i32(self.start + n) - 1)

    def set_start(self, s):
        self.pos, self.bin_known = _i32(s - 1), False

    def set_mate(self, other_ref, other_start, other_neg, other_unmapped):
        self.nref, self.npos = other_ref, _i32(other_start - 1)
        self.flag = (self.flag & ~0x28) | (0x20 if other_neg else 0) | (8 if other_unmapped else 0)


def py_insert_size(a, b):
    if a.unmapped or b.unmapped or a.ref != b.ref:
        return 0
    p1 = a.end if a.neg else a.start
    p2 = b.end if b.neg else b.start
    return _i32(_i32(p2 - p1) + (1 if p2 >= p1 else -1))


def py_set_mate_info(a, b):
    if not a.unmapped and not b.unmapped:
        sa, sb = (a.ref, a.start, a.neg), (b.ref, b.start, b.neg)
        a.set_mate(*sb, False)
        b.set_mate(*sa, False)
        a.mq, b.mq = b.mapq, a.mapq
    elif a.unmapped and b.unmapped:
        na, nb = a.neg, b.neg
        for x, other_neg in ((a, nb), (b, na)):
            x.ref = -1
            x.set_start(0)
            x.set_mate(-1, 0, other_neg, True)
            x.mq, x.tlen = None, 0
    else:
        m, u = (b, a) if a.unmapped else (a, b)
        u.ref = m.ref
        u.set_start(m.start)
        m.set_mate(u.ref, u.start, u.neg, True)
        m.mq, m.tlen = None, 0
        u.set_mate(m.ref, m.start, m.neg, False)
        u.mq, u.tlen = m.mapq, 0
    t = py_insert_size(a, b)
    a.tlen, b.tlen = t, _i32(-t)


def py_reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def py_encode(r):
    """BAMRecordCodec.encode of a record whose mate information was set"""
    head = 36 + r.lrn + 4 * r.nc
    sq = (r.lseq + 1) // 2
    aux = py_parse_aux(r.b[head + sq + r.lseq:4 + r.bs])
    out, placed = b"", False
    for tag, ty, v in aux:
        if tag == b"MC":
            continue
        if tag == b"MQ":
            placed = True
            if r.mq is not None:
                out += py_int_tag(b"MQ", r.mq)
        elif ty in INT_FMT:
            out += py_int_tag(tag, v)
        else:
            out += tag + ty.encode() + v
    if not placed and r.mq is not None:
        out += py_int_tag(b"MQ", r.mq)
    if r.ref < 0:
        bin_ = 0
    elif r.bin_known:
        bin_ = r.bin
    else:
        e = r.end
        bin_ = py_reg2bin(r.pos, e if e > 0 else _i32(r.pos + 1)) & 0xffff
    seq = bytearray(r.b[head:head + sq])
    if r.lseq & 1:
        seq[-1] &= 0xf0
    qual = r.b[head + sq:head + sq + r.lseq]
    if qual[:1] == b"\xff":
        qual = b"\xff" * r.lseq
    body = struct.pack("<iiBBHHHiiii", r.ref, r.pos, r.lrn, r.mapq, bin_, r.nc, r.flag & 0xffff, r.lseq, r.nref, r.npos, r.tlen)
    body += r.b[36:head] + bytes(seq) + qual + out
    return struct.pack("<i", len(body)) + body


def py_layout_ok(b):
    bs, lrn, nc, ls = struct.unpack_from("<i", b)[0], b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<i", b, 20)[0]
    return bs >= 32 and ls >= 0 and 32 + lrn + 4 * nc + (ls + 1) // 2 + ls <= bs


def py_fixmate(recs):
    """-> (src, payloads, status): FixMateReducer's writes over py_reduce_plan's order"""
    if not all(py_layout_ok(r) for r in recs):
        return [], [], K.EFORMAT
    src, outs, pending = [], [], None
    for s, m in py_reduce_plan(recs):
        if m is None:
            src.append(s)
            outs.append(bytes(recs[s]))
            continue
        if pending is None:   # rec1 of the pair: the mate information of both is set here
            a, b = SamRec(recs[s]), SamRec(recs[m])
            py_set_mate_info(a, b)
            mine, pending = a, b
        else:
            mine, pending = pending, None
        try:
            outs.append(py_encode(mine))
        except AuxError:
            return src, outs, K.EFORMAT
        src.append(s)
    return src, outs, 0


# ---- the oracle and the second reading do what the cases declare ----------------------------------------------
def oracle_ranges(o, case):
    pay, off = F.pack(case.recs)
    # HBAM_EMORE is the C ABI's "this window is not the split's last", never an exception of the reader
    r = o.summarize_ranges(pay, off, 0 if case.split_status == K.EMORE else case.split_status)
    return list(zip(r["key"].tolist(), r["beg"].tolist(), r["end"].tolist(), r["rev"].tolist(), r["record"].tolist())), r["status"]


@pytest.mark.parametrize("cid", [c.id for c in SUM + SUM_PRODUCT])
def test_summarize_declared(oracle_mod, cid):
    case = by_id(SUM + SUM_PRODUCT, cid)
    got, status = oracle_ranges(oracle_mod, case)
    assert got == case.ranges
    assert status == case.status
    want, wst = py_summarize(case.recs)   # the reading of Summarize.java in test_consumers.py
    assert want == case.ranges
    assert (wst or (0 if case.split_status == K.EMORE else case.split_status)) == case.status


@pytest.mark.parametrize("cid", [c.id for c in NAME + NAME_PRODUCT])
def test_name_order_declared(oracle_mod, cid):
    case = by_id(NAME + NAME_PRODUCT, cid)
    recs = case.recs()
    assert sorted(case.perm) == list(range(len(recs)))
    pay, off = F.pack(recs)
    assert oracle_mod.name_order(pay, off).tolist() == case.perm
    # Text order read off the bytes: unsigned, a proper prefix first, ties in input order
    names = [_fields(r)["name"] for r in recs]
    assert sorted(range(len(recs)), key=lambda i: (names[i], i)) == case.perm


def check_fixmate(o, d):
    pay, off = F.pack(d["recs"])
    r = o.fixmate(pay, off)
    assert r["status"] == d["status"]
    assert r["src"].tolist() == [s for s, _, _ in d["plan"]]
    got = [bytes(r["payload"][int(r["offsets"][k]):int(r["offsets"][k + 1])]) for k in range(len(r["src"]))]
    for k, (g, w) in enumerate(zip(got, d["outs"])):
        assert g == w, "write %d %r: %s, declared %s" % (k, d["plan"][k], g.hex(), w.hex())
    assert len(got) == len(d["outs"])
    src, outs, status = py_fixmate(d["recs"])
    assert (src, status) == ([s for s, _, _ in d["plan"]], d["status"])
    assert outs == d["outs"]
    # the plan's mates and roles, by the reading in test_consumers.py
    if d["status"] == 0:
        assert [(s, m) for s, m, _ in d["plan"]] == py_reduce_plan(d["recs"])


@pytest.mark.parametrize("cid", [c.id for c in FM])
def test_fixmate_declared(oracle_mod, cid):
    check_fixmate(oracle_mod, by_id(FM, cid).declared())


# an l_read_name of 0 takes no prefix: such cases stand alone above
@pytest.mark.parametrize("cid", [c.id for c in FM if not any(r.l0 for g in c.groups for r in g.recs)])
def test_fixmate_declared_under_a_prefix(oracle_mod, cid):
    case = by_id(FM, cid)
    check_fixmate(oracle_mod, case.declared(b"\xc3\xa9."))


@pytest.mark.parametrize("cid", [c.id for c in FM_PRODUCT])
def test_fixmate_product_declared(oracle_mod, cid):
    check_fixmate(oracle_mod, by_id(FM_PRODUCT, cid).declared())


def test_group_names_are_in_shuffle_order():
    """a case lists its groups in Text order: that is part of the declaration, so hold it to the bytes"""
    for case in FM:
        names = [g.name for g in case.groups]
        assert names == sorted(names) and len(set(names)) == len(names), case.id


# ---- known answers, written by hand ---------------------------------------------------------------------------
def H(s):
    return bytes.fromhex(s.replace(" ", ""))


def rec(fixed, var):
    body = H(fixed) + H(var)
    return struct.pack("<i", len(body)) + body


def fixmate_pair(o, a, b):
    pay, off = F.pack([a, b])
    r = o.fixmate(pay, off)
    assert r["status"] == 0 and r["src"].tolist() == [0, 1]
    return [bytes(r["payload"][int(r["offsets"][k]):int(r["offsets"][k + 1])]) for k in range(2)]


# refID 0, pos 99, l_read_name 2, MAPQ, bin 4681, one CIGAR op, flag, l_seq 5, no mate, TLEN 0; name "q";
# 5M; SEQ 12 48 8f: five bases and a pad nibble of 0xf; QUAL 1 2 3 4 5
A_IN = "00000000 63000000 02 1e 4912 0100 4100 05000000 ffffffff ffffffff 00000000"
B_IN = "00000000 63000000 02 c8 4912 0100 8100 05000000 ffffffff ffffffff 00000000"
A_OUT = "00000000 63000000 02 1e 4912 0100 4100 05000000 00000000 63000000 01000000"   # mate at 0:99, TLEN 1
B_OUT = "00000000 63000000 02 c8 4912 0100 8100 05000000 00000000 63000000 ffffffff"   # TLEN -1
VAR, VAR_OUT = "7100 50000000 12488f 0102030405", "7100 50000000 124880 0102030405"
MQ200, MQ30 = "4d5143 c8", "4d5163 1e"

RETYPE = [
    ("C127_to_c__C128_stays__S255_to_C__S256_stays", "584143 7f" "584243 80" "584353 ff00" "584453 0001",
     "584163 7f" "584243 80" "584343 ff" "584453 0001" + MQ200),
    ("i65535_to_S__i65536_stays__m128_c__m129_s__m32768_s__m32769_i",
     "584169 ffff0000" "584269 00000100" "584369 80ffffff" "584469 7fffffff" "584569 0080ffff" "584669 ff7fffff",
     "584153 ffff" "584269 00000100" "584363 80" "584473 7fff" "584573 0080" "584669 ff7fffff" + MQ200),
    ("I_above_int_max_stays_I__I_int_max_to_i", "584149 00000080" "584249 ffffff7f" "584349 ffffffff",
     "584149 00000080" "584269 ffffff7f" "584349 ffffffff" + MQ200),
    ("s127_c__s128_C__s255_C__s256_S__S32768_stays", "584173 7f00" "584273 8000" "584373 ff00" "584473 0001" "584553 0080",
     "584163 7f" "584243 80" "584343 ff" "584453 0001" "584553 0080" + MQ200),
    # the three MQ placements: rewritten where it stands; and appended where there is none
    ("MQ_first", "4d5143 09" "584143 05" "58425a 6100", "4d5143 c8" "584163 05" "58425a 6100"),
    ("MQ_middle", "584143 05" "4d5143 09" "58425a 6100", "584163 05" "4d5143 c8" "58425a 6100"),
    ("MQ_last", "584143 05" "58425a 6100" "4d5143 09", "584163 05" "58425a 6100" "4d5143 c8"),
    ("MQ_absent_appended", "584143 05" "58425a 6100", "584163 05" "58425a 6100" "4d5143 c8"),
    ("MQ_i_narrower_later_tags_shift", "4d5169 70110100" "58425a 6100", "4d5143 c8" "58425a 6100"),
    ("MC_removed_float_char_hex_array_copied", "4d435a 354d00" "584166 0000c0bf" "584241 51" "584348 314100" "58444273 02000000 0100feff",
     "584166 0000c0bf" "584241 51" "584348 314100" "58444273 02000000 0100feff" "4d5143 c8"),
]


@pytest.mark.parametrize("row", RETYPE, ids=[r[0] for r in RETYPE])
def test_known_aux_answers(oracle_mod, row):
    _, aux_in, aux_out = row
    a, b = fixmate_pair(oracle_mod, rec(A_IN, VAR + aux_in), rec(B_IN, VAR))
    assert a == rec(A_OUT, VAR_OUT + aux_out)
    assert b == rec(B_OUT, VAR_OUT + MQ30)


@pytest.mark.parametrize("qa, qb, mq_a, mq_b", [("00", "ff", "4d5143 ff", "4d5163 00"), ("7f", "80", "4d5143 80", "4d5163 7f")])
def test_known_mq_from_mapq(oracle_mod, qa, qb, mq_a, mq_b):
    """MAPQ 0 and 127 are written as 'c', 128 and 255 as 'C'"""
    a, b = fixmate_pair(oracle_mod, rec(A_IN.replace(" 1e ", " %s " % qa), VAR), rec(B_IN.replace(" c8 ", " %s " % qb), VAR))
    assert a == rec(A_OUT.replace(" 1e ", " %s " % qa), VAR_OUT + mq_a)
    assert b == rec(B_OUT.replace(" c8 ", " %s " % qb), VAR_OUT + mq_b)


def lit(ref, pos, mapq, bin_, flag, nref, npos, tlen, cigar="50000000", sq="12488f 0102030405", aux="", l_seq=5):
    """a record from literal numbers: name "q", the CIGAR words, SEQ + QUAL and aux as hex"""
    n = len(H(cigar)) // 4
    body = struct.pack("<iiBBHHHiiii", ref, pos, 2, mapq, bin_, n, flag, l_seq, nref, npos, tlen) + b"q\0" + H(cigar) + H(sq) + H(aux)
    return struct.pack("<i", len(body)) + body


OUT5 = "124880 0102030405"
M10 = "a0000000"   # 10M
# 3H 2S 5M 2I 4N 3= 2X 6P 1D 5M 2S 1H: the reference length is 5 + 4 + 3 + 2 + 1 + 5 = 20
OPS = "35000000 24000000 50000000 21000000 43000000 37000000 28000000 66000000 12000000 50000000 24000000 15000000"
INT_MAX, INT_MIN = 2147483647, -2147483648

TLEN = [
    # name, (pos, flag, cigar) of rec1 and of rec2, the flags out, TLEN of rec1 and of rec2
    ("tie_forward_forward", (99, 0x41, "50000000"), (99, 0x81, "50000000"), (0x41, 0x81), 1, -1),
    ("tie_forward_reverse", (99, 0x41, "50000000"), (90, 0x91, M10), (0x61, 0x91), 1, -1),         # 91 + 10 - 1 = 100
    ("tie_reverse_forward", (90, 0x51, M10), (99, 0x81, "50000000"), (0x51, 0xa1), 1, -1),
    ("tie_reverse_reverse", (90, 0x51, M10), (95, 0x91, "50000000"), (0x71, 0xb1), 1, -1),         # 96 + 5 - 1 = 100
    ("second_below_first", (100, 0x41, "50000000"), (99, 0x81, "50000000"), (0x41, 0x81), -2, 2),
    ("reverse_through_N_eq_X_P_H", (99, 0x41, "50000000"), (199, 0x91, OPS), (0x61, 0x91), 120, -120),  # 200 + 20 - 1 = 219; 219 - 100 + 1
    ("reverse_without_cigar", (99, 0x41, "50000000"), (99, 0x91, ""), (0x61, 0x91), -2, 2),             # end 99 < 100
    ("start_wraps_to_int_min", (INT_MAX, 0x41, "50000000"), (0, 0x81, "50000000"), (0x41, 0x81), INT_MIN + 2, INT_MAX - 1),
    ("tlen_int_min_and_its_negation", (INT_MAX, 0x41, "50000000"), (-2, 0x81, "50000000"), (0x41, 0x81), INT_MIN, INT_MIN),
    ("end_wraps", (0, 0x41, "50000000"), (INT_MAX - 5, 0x91, M10), (0x61, 0x91), INT_MIN + 2, INT_MAX - 1),
    ("difference_wraps", (-2000000000, 0x41, "50000000"), (1999999999, 0x81, "50000000"), (0x41, 0x81), -294967296, 294967296),
]


@pytest.mark.parametrize("row", TLEN, ids=[r[0] for r in TLEN])
def test_known_tlen_answers(oracle_mod, row):
    _, (p1, f1, c1), (p2, f2, c2), (o1, o2), t1, t2 = row
    a, b = fixmate_pair(oracle_mod, lit(3, p1, 30, 0xBEEF, f1, -1, -1, 55, c1), lit(3, p2, 200, 7, f2, -1, -1, 66, c2))
    assert a == lit(3, p1, 30, 0xBEEF, o1, 3, p2, t1, c1, OUT5, MQ200)   # the bin, garbage included, is kept
    assert b == lit(3, p2, 200, 7, o2, 3, p1, t2, c2, OUT5, MQ30)


def test_known_tlen_different_references(oracle_mod):
    a, b = fixmate_pair(oracle_mod, lit(3, 99, 30, 4681, 0x41, -1, -1, 55), lit(4, 500, 200, 4681, 0x81, -1, -1, 66))
    assert a == lit(3, 99, 30, 4681, 0x41, 4, 500, 0, sq=OUT5, aux=MQ200)
    assert b == lit(4, 500, 200, 4681, 0x81, 3, 99, 0, sq=OUT5, aux=MQ30)


@pytest.mark.parametrize("pos, bin_", [(16383, 4681), (16384, 4682), ((1 << 29) - 1, 37448), (1 << 29, 37449), (60855 << 14, 0), (-1, 4680)])
@pytest.mark.parametrize("unmapped_first", [False, True])
def test_known_bin_answers(oracle_mod, pos, bin_, unmapped_first):
    """the unmapped read takes its mate's place and a bin recomputed over one base there; the mapped read
    loses its MQ and keeps its bin; both TLEN 0"""
    m = lit(3, pos, 30, 0x1234, 0x51, 9, 9, 55, aux="4d5143 09" "584143 05")
    u = lit(-1, -1, 0, 0x4321, 0x85, 9, 9, 66, sq="12488f ff02030405")
    got = fixmate_pair(oracle_mod, *((u, m) if unmapped_first else (m, u)))
    gm, gu = (got[1], got[0]) if unmapped_first else got
    assert gm == lit(3, pos, 30, 0x1234, 0x59, 3, pos, 0, sq=OUT5, aux="584163 05")
    assert gu == lit(3, pos, 0, bin_, 0xa5, 3, pos, 0, sq="124880 ffffffffff", aux=MQ30)   # a first quality of 0xff: all 0xff


def test_known_unplaced_and_both_unmapped(oracle_mod):
    m, u = lit(-1, 500, 30, 0x1234, 0x41, 9, 9, 55), lit(2, 77, 0, 0x4321, 0x85, 9, 9, 66, aux="4d5143 09")
    gm, gu = fixmate_pair(oracle_mod, m, u)
    assert gm == lit(-1, 500, 30, 0, 0x49, -1, 500, 0, sq=OUT5)
    assert gu == lit(-1, 500, 0, 0, 0x85, -1, 500, 0, sq=OUT5, aux=MQ30)
    a, b = lit(2, 40, 30, 0x1234, 0x55, 9, 9, 55, aux="4d5143 09" "584143 05"), lit(1, 77, 9, 0x4321, 0x85, 9, 9, 66)
    ga, gb = fixmate_pair(oracle_mod, a, b)
    assert ga == lit(-1, -1, 30, 0, 0x5d, -1, -1, 0, sq=OUT5, aux="584163 05")
    assert gb == lit(-1, -1, 9, 0, 0xad, -1, -1, 0, sq=OUT5)


def test_known_seq_and_quality_answers(oracle_mod):
    # a later 0xff is kept; l_seq 0; an even length keeps its low nibble
    a, b = fixmate_pair(oracle_mod, lit(0, 99, 30, 4681, 0x41, -1, -1, 0, sq="12488f 01ffffffff"),
                        lit(0, 99, 200, 4681, 0x81, -1, -1, 0, cigar="", sq="", l_seq=0))
    assert a == lit(0, 99, 30, 4681, 0x41, 0, 99, 1, sq="124880 01ffffffff", aux=MQ200)
    assert b == lit(0, 99, 200, 4681, 0x81, 0, 99, -1, cigar="", sq="", l_seq=0, aux=MQ30)
    a, b = fixmate_pair(oracle_mod, lit(0, 99, 30, 4681, 0x41, -1, -1, 0, sq="2f 0708", l_seq=2), lit(0, 99, 200, 4681, 0x81, -1, -1, 0, sq="2f ff", l_seq=1))
    assert a == lit(0, 99, 30, 4681, 0x41, 0, 99, 1, sq="2f 0708", l_seq=2, aux=MQ200)
    assert b == lit(0, 99, 200, 4681, 0x81, 0, 99, -1, sq="20 ff", l_seq=1, aux=MQ30)


def test_known_summarize_answers(oracle_mod):
    """b = 2^31 - 10, 20M: the end wraps to -2147483639, b + ee = -1, and the centre is 0, not -1;
    a negative centre takes the refID out of the key, and the ranges after it keep that high word"""
    one = lit(5, INT_MAX - 10, 30, 0, 0, -1, -1, 0, cigar="40010000")
    neg = lit(7, 2013265919, 30, 0, 0x10, -1, -1, 0, cigar="20000080 22000000 40000000" + " f3ffffff" * 8 + " a3000000 40000000")
    first_err = lit(1, 50, 30, 0, 0, -1, -1, 0, cigar="40000000 39000000")   # 4M, then op 9
    later = lit(1, 60, 30, 0, 0, -1, -1, 0, cigar="")                            # no range: never reached
    pay, off = F.pack([one, neg, first_err, later])
    r = oracle_mod.summarize_ranges(pay, off)
    assert r["status"] == K.EREFID
    assert list(zip(r["key"].tolist(), r["beg"].tolist(), r["end"].tolist(), r["rev"].tolist(), r["record"].tolist())) == [
        (5 << 32, 2147483638, -2147483639, 0, 0),
        (-67108863, 2013265920, -2147483647, 1, 1), (-2147483642, -2147483644, -2147483641, 1, 1), (-4294967285, 10, 13, 1, 1)]
    pay, off = F.pack([one, later, first_err])
    r = oracle_mod.summarize_ranges(pay, off)
    assert r["status"] == K.EINDEX and r["record"].tolist() == [0]      # the first record that raises, not the first kind


def test_known_name_answers(oracle_mod):
    names = [b"A", b"A\0", b"A\0C", b"AB", b"", b"ABCDEFGZA", b"ABCDEFGAZ"]
    pay, off = F.pack([F.record(n) for n in names] + [F.record_l0()])
    assert oracle_mod.name_order(pay, off).tolist() == [4, 7, 0, 1, 2, 3, 6, 5]


# ---- the cases reach the arms they are there for ----------------------------------------------------------------
def test_summarize_cases_exercise_the_rules():
    # error precedence: three kinds in three workgroups, each kind first once, a lower kind at a later record
    for name, at in K.RACE.items():
        case = by_id(SUM, "race-" + name)
        assert len({i // K.WG for i, _ in at}) == 3 and {k for _, k in at} == {1, 2, 3}
        first = min(at)
        assert case.status == K.KIND_STATUS[first[1]] and len(case.recs) > 3 * K.WG - 1
        assert case.ranges and all(r[4] < first[0] for r in case.ranges) and case.ranges[-1][4] == first[0] - 1
        skipped = [i for i in range(first[0]) if i % 50 == 7]
        assert skipped and not {r[4] for r in case.ranges} & set(skipped)
    assert {K.RACE[n][0][1] for n in K.RACE} == {1, 2, 3}
    assert any(min(at)[1] > min(k for _, k in at) for at in K.RACE.values())    # a packed (kind, record) minimum would differ
    assert {c.status for c in SUM} >= {0, K.EREFID, K.EINDEX, K.EFORMAT, K.ETRUNC}
    # the ranges before the raising record stand, and the raising record's own do not
    c = by_id(SUM, "op9-after-range")
    assert c.ranges and max(r[4] for r in c.ranges) < 2
    # skipped records that carry a bad CIGAR
    c = by_id(SUM, "skipped-with-bad-cigar")
    f = [_fields(r) for r in c.recs]
    assert any(x["flag"] & 4 and x["cigar"] and x["cigar"][1] & 15 == 9 for x in f)
    assert any(x["ref"] < 0 and x["cigar"] is None for x in f) and any(x["pos"] < -1 and not x["cigar"] for x in f)
    assert c.status == 0 and {r[4] for r in c.ranges} == {0, 5}
    # mapped reads without a range
    assert {cid for cid in ("empty-no-cigar", "empty-0M", "empty-only-S-I") if by_id(SUM, cid).status == K.EINDEX} == {"empty-no-cigar", "empty-0M", "empty-only-S-I"}
    # every flushing op between two M runs; D directly before N
    flush = _fields(by_id(SUM, "flush-I-S-H-P").recs[0])["cigar"]
    ops = [c & 15 for c in flush]
    between = {ops[j] for j in range(1, len(ops) - 1) if ops[j - 1] in (0, 7, 8) and ops[j + 1] in (0, 7, 8)}
    assert between >= {K.I_, K.S_, K.H_, K.P_} and {7, 8} <= set(ops)
    ops = [c & 15 for c in _fields(by_id(SUM, "D-then-N").recs[0])["cigar"]]
    assert (K.D_, K.N_) in zip(ops, ops[1:])
    # centres: b + ee negative and odd; a negative first centre followed by later ranges under its high word
    k, b, e, _, _ = by_id(SUM, "centre-minus-one").ranges[0]
    assert b + e == -1 and k & 0xffffffff == 0
    rr = by_id(SUM, "centre-negative-then-more").ranges
    assert (rr[0][1] + rr[0][2]) < 0 and (rr[0][1] + rr[0][2]) % 2 and rr[0][0] < 0 and len(rr) == 3
    assert rr[2][0] >> 32 == -1 and rr[2][0] & 0xffffffff == 11
    # dv->status
    st = {c.id: (c.split_status, c.status, len(c.recs)) for c in SUM}
    assert st["status-more"] == (K.EMORE, 0, 2) and st["status-trunc"][:2] == (K.ETRUNC, K.ETRUNC)
    assert st["status-overridden"][:2] == (K.ETRUNC, K.EREFID) and st["n0"] == (0, 0, 0) and st["n0-trunc"] == (K.ETRUNC, K.ETRUNC, 0)
    # the product run: ranges of several cases, then an error with records behind it
    p = SUM_PRODUCT[0]
    assert p.status == K.EREFID and max(r[4] for r in p.ranges) < len(p.recs) - 3 and len(p.ranges) > 12


def test_name_cases_exercise_the_rules():
    lens = {c.id: [0 if n is K.L0 else len(n) for n in c.names] for c in NAME}
    assert max(lens["len-254"]) == 254 and (254 + 7) // 8 == 32
    assert set(lens["all-empty"]) == {0} and len(lens["all-empty"]) > K.WG and by_id(NAME, "all-empty").perm == list(range(300))
    assert {K.L0, b""} <= set(by_id(NAME, "all-empty").names) and {K.L0, b""} <= set(by_id(NAME, "empty-l0-l1").names)
    assert len(set(lens["same-length"])) == 1 and by_id(NAME, "same-length").perm != sorted(by_id(NAME, "same-length").perm)
    n = by_id(NAME, "byte7-byte8").names
    assert n[0][:7] == n[1][:7] and n[0][7] > n[1][7] and n[0][8] < n[1][8]
    assert {b"A", b"A\0", b"A\0C", b"AB"} == set(by_id(NAME, "embedded-nul").names)
    assert lens["n1"] == [4] and lens["n0"] == [] and len(lens["ties-wide"]) > 2 * K.WG
    p = NAME_PRODUCT[0]
    assert len(p.names) > 600 and p.perm != sorted(p.perm) and p.names.count(K.L0) == 2


def _mated(cases=None):
    """(case, group, record, W) of every mated write that stands"""
    return [(c, g, r, w) for c in (FM if cases is None else cases) for g, r, _, w in c.writes() if w is not None]


def test_fixmate_cases_exercise_the_rules():
    mated = _mated()
    # the integer re-encode: every boundary value in every type that holds it, on a mated write
    want = {(t, v) for v in M.INT_VALUES for t, (lo, hi) in M.HOLDS.items() if lo <= v <= hi}
    have = {(it.info["typ"], it.info["v"]) for _, _, r, _ in mated for it in r.items if it.kind == "int"}
    assert have >= want and {127, 128, 255, 256, 65535, 65536, -128, -129, -32768, -32769, 1 << 31} <= set(M.INT_VALUES)
    assert {w.mq for _, _, _, w in mated} >= {0, 127, 128, 255, None}
    # MQ / MC placement
    place = by_id(FM, "placement")
    seen = set()
    for g in place.groups:
        r = g.recs[0]
        kinds = [it.kind for it in r.items]
        w = g.wants[0, 1]
        for k, kind in enumerate(kinds):
            if kind == "mq":
                where = "only" if len(kinds) == 1 else "first" if k == 0 else "last" if k == len(kinds) - 1 else "middle"
                seen.add(("mq", where, "set" if w.mq is not None else "removed", r.items[k].info["typ"]))
        seen.add((kinds.count("mq"), kinds.count("mc"), len(kinds), w.mq is not None))
    for where in ("first", "middle", "last"):
        assert any(s[:3] == ("mq", where, "set") for s in seen) and any(s[:3] == ("mq", where, "removed") for s in seen)
    assert {s[3] for s in seen if s[0] == "mq"} >= {"c", "C", "S", "i", "Z", "A"}
    assert {(2, 0, 3, True), (2, 0, 3, False), (0, 2, 3, True), (0, 1, 1, True), (0, 1, 1, False), (0, 0, 0, True), (0, 0, 0, False)} <= seen
    # an MQ that shrinks in place with tags behind it, one that keeps its size; none that grows (see below)
    sizes = {(len(it.src) - 3, k < len(r.items) - 1) for _, _, r, w in mated if w.mq is not None
             for k, it in enumerate(r.items) if it.kind == "mq"}
    assert (4, True) in sizes and (1, True) in sizes and (2, True) in sizes
    # TLEN
    t = {g.name: g for g in by_id(FM, "tlen").groups}
    ties = {(g.recs[0].neg, g.recs[1].neg) for n, g in t.items() if n.startswith(b"tie-")}
    assert ties == {(False, False), (False, True), (True, False), (True, True)}
    assert all(g.wants[0, 1].tlen == 1 and g.wants[1, 2].tlen == -1 for n, g in t.items() if n.startswith(b"tie-"))
    ops = {op for _, op in t[b"ops-second"].recs[1].cigar}
    assert ops == set(range(9)) and t[b"ops-second"].recs[1].neg and t[b"ops-first"].recs[0].neg
    assert t[b"refs-differ"].recs[0].ref != t[b"refs-differ"].recs[1].ref and t[b"refs-differ"].wants[0, 1].tlen == 0
    assert t[b"rev-no-cigar"].recs[1].neg and not t[b"rev-no-cigar"].recs[1].cigar
    assert t[b"wrap-p1-min"].recs[0].pos == K.I32_MAX and not t[b"wrap-p1-min"].recs[0].neg      # p1 = INT32_MIN
    assert t[b"wrap-tlen-min"].wants[0, 1].tlen == t[b"wrap-tlen-min"].wants[1, 2].tlen == K.I32_MIN
    assert t[b"wrap-end"].recs[1].neg and t[b"wrap-end"].recs[1].pos > K.I32_MAX - 10
    assert abs(t[b"wrap-diff"].recs[1].pos - t[b"wrap-diff"].recs[0].pos) > K.I32_MAX
    assert t[b"bin-kept"].wants[0, 1].bin == 0xBEEF and t[b"bin-unplaced"].wants[0, 1].bin == 0
    # the recomputed bin
    b = by_id(FM, "bin")
    at = {(g.recs[0].pos if not g.recs[0].unmapped else g.recs[1].pos): g for g in b.groups if g.name.startswith(b"at")}
    assert set(at) >= {16383, 16384, (1 << 29) - 1, 1 << 29, -1} and any(p >= 60855 << 14 for p in at)
    firsts = {g.recs[0].unmapped for g in b.groups if g.name.startswith(b"at")}
    assert firsts == {False, True}
    un = {g.name: g for g in b.groups}[b"unplaced"]
    assert un.recs[0].ref == -1 and not un.recs[0].unmapped and un.wants[1, 2].bin == 0 and un.wants[1, 2].ref == -1
    assert {g.name: g for g in b.groups}[b"uu"].wants[0, 1].ref == -1
    # sequence and quality
    sq = [r for c, _, r, _ in mated if c.id == "seq-qual"]
    assert {r.l_seq for r in sq} >= {0, 1, 2, 5}
    assert any(r.l_seq & 1 and r.seq[-1] & 15 for r in sq)
    assert any(r.l_seq > 1 and r.qual[0] == 0xff and set(r.qual[1:]) - {0xff} for r in sq)
    assert any(r.l_seq > 1 and r.qual[0] != 0xff and set(r.qual[1:]) == {0xff} for r in sq)
    assert all(r.l_seq % 2 == 0 or r.seq[-1] & 15 for _, _, r, _ in mated if r.l_seq and not r.l0)   # every odd mated write shows the pad
    # malformed aux: every shape fails a mated write; untouched writes of bad records stand
    bad = [c for c in FM if c.id.startswith("malformed-")]
    assert len(bad) == len(M.MALFORMED) >= 12 and all(c.fails_at() == 5 and c.declared()["status"] == K.EFORMAT for c in bad)
    assert {"trunc1", "trunc2", "z_no_nul", "h_no_nul", "b_header_cut", "b_subtype", "b_count_past", "int_cut", "unknown_type"} <= set(M.MALFORMED)
    u = by_id(FM, "bad-untouched")
    shapes = {"".join("S" if r.flag & 0x100 else "P" for r in g.recs): g for g in u.groups}
    assert u.fails_at() is None and set(shapes) == {"P", "SPP", "PPP"}
    assert all(any(r.bad for r in g.recs) and not any(g.recs[s].bad for s, m, _ in g.writes if m is not None) for g in u.groups)
    q = by_id(FM, "bad-quirk")
    g = q.groups[1]
    assert g.writes == K.SHAPES["PS"] and g.recs[1].bad and g.recs[1].flag & 0x100
    assert q.fails_at() == 2 + 2 and len(q.declared()["plan"]) == 4          # its first write and the primary's stand
    race = by_id(FM, "race")
    assert len({w // K.WG for w in K.RACE_AT}) == 3 and race.fails_at() == min(K.RACE_AT) and list(K.RACE_AT) != sorted(K.RACE_AT)
    assert len(race.build()[1]) >= 3 * K.WG + 1 and min(K.RACE_AT) > K.WG
    assert all(by_id(FM, "overrun-" + f).declared()["plan"] == [] for f in ("cigar", "seq", "negative-l_seq"))
    # the reducer plan
    shapes = {"".join("S" if r.flag & 0x100 else "P" for r in g.recs) for g in by_id(FM, "shapes").groups}
    assert shapes == set(K.SHAPES) and {"PS", "PSS", "SPSP", "PPP", "P", "S"} <= shapes
    many = by_id(FM, "many-groups")
    assert len(many.groups) > 2 * K.WG
    heads = np.cumsum([0] + [len(g.recs) for g in many.groups])[:-1]
    assert K.WG in heads and 2 * K.WG in heads        # a group head on the first lane of a workgroup of k_fm_heads
    wide = by_id(FM, "wide-group")
    assert max(len(g.recs) for g in wide.groups) > K.WG and len(wide.groups) == 3
    heads = np.cumsum([0] + [len(g.recs) for g in wide.groups])[:-1]
    assert K.WG not in heads                             # and a first lane that is no head
    assert by_id(FM, "n0").declared()["recs"] == [] and len(by_id(FM, "n1").declared()["recs"]) == 1
    e = by_id(FM, "empty-names").groups[0]
    assert {r.l0 for r in e.recs} == {True, False} and e.name == b"" and len(e.writes) == 3
    # the product runs hold every clean case and end on a failing one
    assert FM_PRODUCT[0].status == 0 and FM_PRODUCT[0].n_groups > 2 * K.WG and len(FM_PRODUCT[0].recs) > 1200
    assert FM_PRODUCT[1].status == K.EFORMAT and len(FM_PRODUCT[1].plan) > 100


def test_arms_no_case_can_reach():
    """asserted, not excluded: what would have to hold for these arms to be reached never does"""
    for c, g, r, w in _mated(FM):
        recomputed = r.unmapped and w.ref >= 0
        if recomputed:
            # the bin is recomputed for an unmapped read alone; its alignment end is 0, so the span handed to
            # reg2bin is [pos, pos + 1): one base, which no coarser level than 4681 + (pos >> 14) can hold
            assert w.bin == (4681 + (w.pos >> 14)) & 0xffff, (c.id, g.name)
            assert not 0 < w.bin < 4680
        else:
            assert w.bin == (r.bin if w.ref >= 0 else 0)
        # MQ is written from a MAPQ byte: one value byte, and no aux value is shorter, so an MQ already there
        # never grows
        if w.mq is not None:
            assert 0 <= w.mq <= 255 and len(K.mq_bytes(w.mq)) == 4
            assert all(len(it.src) >= 4 for it in r.items if it.kind == "mq")
