"""A BCF2 record and header encoder for the VCF text tests, and the crafted records: every rule of
hbam_vcf_render (include/hbam.h) that a decode of bcf_records.bcf_stream does not reach."""
import os
import struct

import numpy as np

import vcftext_ref as R

INT8, INT16, INT32, FLOAT, CHAR = 1, 2, 3, 5, 7
MISS = {INT8: -128, INT16: -32768, INT32: -(1 << 31)}
MISSF = 0x7F800001
_FMT = {INT8: "<b", INT16: "<h", INT32: "<i"}
HERE = os.path.dirname(os.path.abspath(__file__))


def f32bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def desc(t, k, long=False):
    """A descriptor byte, with the count behind it for 15 values or more (or when asked)."""
    if k < 15 and not long:
        return bytes([k << 4 | t])
    ct = INT8 if k <= 127 else INT16 if k <= 32767 else INT32
    return bytes([0xf0 | t, 0x10 | ct]) + struct.pack(_FMT[ct], k)


def ints(vals, t=INT8, long=False):
    return desc(t, len(vals), long) + b"".join(struct.pack(_FMT[t], v) for v in vals)


def floats(vals, long=False):
    """floats, or raw bit patterns given as ints"""
    return desc(FLOAT, len(vals), long) + b"".join(
        struct.pack("<I", v if isinstance(v, int) else f32bits(v)) for v in vals)


def string(s, long=False):
    s = s.encode() if isinstance(s, str) else s
    return desc(CHAR, len(s), long) + s


NULL = b"\x00"


def header_text(contigs, info=(), fmt=(), filters=(), samples=(), sites_only=False):
    """info / fmt: (ID, Number, Type)."""
    lines = ["##fileformat=VCFv4.2"]
    lines += ['##FILTER=<ID=%s,Description="f">' % f for f in filters]
    lines += ['##INFO=<ID=%s,Number=%s,Type=%s,Description="i">' % x for x in info]
    lines += ['##FORMAT=<ID=%s,Number=%s,Type=%s,Description="g">' % x for x in fmt]
    lines += ["##contig=<ID=%s,length=1000000>" % c for c in contigs]
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    if not sites_only:
        cols += "\tFORMAT" + "".join("\t" + s for s in samples)
    return "\n".join(lines + [cols]) + "\n"


class Enc:
    """Records under one header (a vcftext_ref.parse_header dict)."""

    def __init__(self, text):
        self.text = text
        self.hdr = R.parse_header(text)
        self.ix = {n: i for i, n in enumerate(self.hdr["dict"])}

    def key(self, k):
        k = self.ix[k] if isinstance(k, str) else k
        return ints([k], INT8 if -120 <= k <= 127 else INT16)

    def record(self, chrom=0, pos=0, ident=None, alleles=("A", "C"), qual=None, filt=None, info=(), fmt=(),
               n_sample=None, n_allele=None, tail=b""):
        """qual: a float, raw bits (int) or None (missing); filt: None (no value) or dictionary offsets /
        names; info: (key, typed value bytes); fmt: (key, t, k, rows) with a row of k raw values per sample
        (ints, float bits, or one bytes object of k chars), or (key, raw bytes)."""
        n_sample = len(self.hdr["samples"]) if n_sample is None else n_sample
        qb = MISSF if qual is None else qual if isinstance(qual, int) else f32bits(qual)
        s = struct.pack("<iiiI", chrom, pos, len(alleles[0]) if alleles else 0, qb)
        s += struct.pack("<II", (len(alleles) if n_allele is None else n_allele) << 16 | len(info),
                         len(fmt) << 24 | n_sample)
        s += NULL if ident is None else string(ident)
        for a in alleles:
            s += string(a) if not isinstance(a, bytes) or a else NULL
        if filt is None:
            s += NULL
        else:
            s += ints([self.ix[f] if isinstance(f, str) else f for f in filt])
        for k, v in info:
            s += self.key(k) + v
        g = b""
        for fd in fmt:
            if len(fd) == 2:
                g += self.key(fd[0]) + fd[1]
                continue
            k, t, cnt, rows = fd
            g += self.key(k) + desc(t, cnt)
            for row in rows:
                if t == CHAR:
                    g += bytes(row).ljust(cnt, b"\0")
                elif t == FLOAT:
                    g += b"".join(struct.pack("<I", v if isinstance(v, int) else f32bits(v)) for v in row)
                else:
                    g += b"".join(struct.pack(_FMT[t], v) for v in row)
        g += tail
        return struct.pack("<II", len(s), len(g)) + s + g


def pack(records):
    """-> (data bytes, rec_off uint64[n])."""
    off = np.zeros(len(records), np.uint64)
    at = 0
    for i, r in enumerate(records):
        off[i] = at
        at += len(r)
    return b"".join(records), off


def split_stream(stream):
    """The records of an uncompressed BCF2 stream (bcf_records.bcf_stream) -> (header text, [record])."""
    lt = struct.unpack_from("<I", stream, 5)[0]
    text = stream[9:9 + lt].rstrip(b"\0").decode()
    at, out = 9 + lt, []
    while at < len(stream):
        ls, li = struct.unpack_from("<II", stream, at)
        out.append(stream[at:at + 8 + ls + li])
        at += 8 + ls + li
    return text, out


# ---- the reference's own expectations ---------------------------------------------------------------
def golden_header_text(sites_only=False):
    with open(os.path.join(HERE, "golden", "test.vcf")) as f:
        lines = [ln for ln in f.read().split("\n") if ln.startswith("#")]
    if sites_only:
        lines = [ln for ln in lines if not ln.startswith("##FORMAT")]
        lines[-1] = "\t".join(lines[-1].split("\t")[:8])
    return "\n".join(lines) + "\n"


def simple_case():
    """TestVCFOutputFormat.testSimple -> (Enc, record, expected line)."""
    e = Enc(golden_header_text(sites_only=True))
    rec = e.record(0, 1, None, ("C", "A"), 80.0, [0], [("NS", ints([4]))])
    return e, rec, b"20\t2\t.\tC\tA\t80\tPASS\tNS=4\n"


GOLDEN_EXPECTED = (
    b"20\t14370\trs6054257\tG\tA\t29\tPASS\tAF=0.500;DB;DP=14;H2;NS=3\tGT:DP:GQ:HQ\t0|0:1:48:51,51\t1|0:8:48:51,51\t1/1:5:43\n"
    b"20\t17330\t.\tT\tA\t3\tq10\tAF=0.017;DP=11;NS=3\tGT:DP:GQ:HQ\t0|0:3:49:58,50\t0|1:5:3:65,3\t0/0:3:41\n"
    b"20\t1110696\trs6040355\tA\tG,T\t67\tPASS\tAA=T;AF=0.333,0.667;DB;DP=10;NS=2\tGT:DP:GQ:HQ\t1|2:6:21:23,27\t2|1:0:2:18,2\t2/2:4:35\n"
    b"20\t1230237\t.\tT\t.\t47\tPASS\tAA=T;DP=13;NS=3\tGT:DP:GQ:HQ\t0|0:7:54:56,60\t0|0:4:48:51,51\t0/0:2:61\n"
    b"20\t1234567\tmicrosat1\tGTC\tG,GTCT\t50\tPASS\tAA=G;DP=9;NS=3\tGT:DP:GQ\t0/1:4:35\t0/2:2:17\t1/1:3:40\n")


def _gt(text):
    """"0|1" -> the encoded alleles; a phased call has the bit on every allele, as htsjdk's writer sets it"""
    ph = 1 if "|" in text else 0
    return [((0 if a == "." else int(a) + 1) << 1) | ph for a in text.replace("|", "/").split("/")]


def golden_records():
    """The five records of tests/golden/test.vcf under its own header -> (Enc, [record])."""
    e = Enc(golden_header_text())
    M = MISS[INT8]

    def rec(pos, ident, alleles, qual, filt, info, gts, gq, dp, hq):
        fmt = [("GT", INT8, 2, [_gt(g) for g in gts]), ("GQ", INT8, 1, [[x] for x in gq]),
               ("DP", INT8, 1, [[x] for x in dp])]
        if hq is not None:
            fmt.append(("HQ", INT8, 2, hq))
        return e.record(0, pos - 1, ident, alleles, qual, filt, info, fmt)

    flag = NULL
    recs = [
        rec(14370, "rs6054257", ("G", "A"), 29.0, ["PASS"],
            [("NS", ints([3])), ("DP", ints([14])), ("AF", floats([0.5])), ("DB", flag), ("H2", flag)],
            ("0|0", "1|0", "1/1"), (48, 48, 43), (1, 8, 5), [[51, 51], [51, 51], [M, M]]),
        rec(17330, None, ("T", "A"), 3.0, ["q10"],
            [("NS", ints([3])), ("DP", ints([11])), ("AF", floats([0.017]))],
            ("0|0", "0|1", "0/0"), (49, 3, 41), (3, 5, 3), [[58, 50], [65, 3], [M, M]]),
        rec(1110696, "rs6040355", ("A", "G", "T"), 67.0, ["PASS"],
            [("NS", ints([2])), ("DP", ints([10])), ("AF", floats([0.333, 0.667])), ("AA", string("T")), ("DB", flag)],
            ("1|2", "2|1", "2/2"), (21, 2, 35), (6, 0, 4), [[23, 27], [18, 2], [M, M]]),
        rec(1230237, None, ("T",), 47.0, ["PASS"],
            [("NS", ints([3])), ("DP", ints([13])), ("AA", string("T"))],
            ("0|0", "0|0", "0/0"), (54, 48, 61), (7, 4, 2), [[56, 60], [51, 51], [M, M]]),
        rec(1234567, "microsat1", ("GTC", "G", "GTCT"), 50.0, ["PASS"],
            [("NS", ints([3])), ("DP", ints([9])), ("AA", string("G"))],
            ("0/1", "0/2", "1/1"), (35, 17, 40), (4, 2, 3), None),
    ]
    return e, recs


# ---- the crafted records ----------------------------------------------------------------------------
CRAFT_INFO = [("DP", "1", "Integer"), ("AF", "A", "Float"), ("DB", "0", "Flag"), ("IV", ".", "Integer"),
              ("ST", "1", "String"), ("FV", ".", "Float"), ("ZZ", "0", "Integer"), ("AA", "1", "String")]
CRAFT_FMT = [("GT", "1", "String"), ("DP", "1", "Integer"), ("GQ", "1", "Integer"), ("AD", "R", "Integer"),
             ("PL", "G", "Integer"), ("FT", "1", "String"), ("HQ", "2", "Integer"), ("XA", "A", "Integer"),
             ("XR", "R", "Integer"), ("XG", "G", "Integer"), ("XF", "1", "Float"), ("XS", "1", "String"),
             ("X1", ".", "Integer"), ("ZQ", "1", "Integer")]
CRAFT_FILTERS = ["q10", "s50", "zz9", "aa1"]
CRAFT_SAMPLES = ("S1", "S2", "S3")


def craft_encoder(samples=CRAFT_SAMPLES, extra_fmt=()):
    # NOFMT / NOINFO: dictionary entries (a FILTER line) without a FORMAT / an INFO line
    return Enc(header_text(["c1", "c2"], CRAFT_INFO, list(CRAFT_FMT) + list(extra_fmt),
                           CRAFT_FILTERS + ["NOLINE"], samples))


def crafted():
    """-> (Enc, [(name, record)]): every one renders (status OK); some are deferred."""
    e = craft_encoder()
    M8, M16, M32 = MISS[INT8], MISS[INT16], MISS[INT32]
    gt3 = ("GT", INT8, 2, [[2, 4], [2, 2], [4, 4]])
    out = []

    def add(name, **kw):
        kw.setdefault("fmt", [gt3])
        kw.setdefault("pos", 100 + len(out))
        out.append((name, e.record(**kw)))

    # integer widths, the count nibble 15, end-of-vector codes as numbers
    add("int8", info=[("IV", ints([1, -127, 127]))])
    add("int16", info=[("IV", ints([300, -32767, 32767], INT16))])
    add("int32", info=[("IV", ints([70000, -(1 << 31) + 1, (1 << 31) - 1], INT32))])
    add("long8", info=[("IV", ints(list(range(1, 21)), INT8))])
    add("long16", info=[("IV", ints(list(range(1000, 1015)), INT16))])
    add("long32", info=[("IV", ints(list(range(100000, 100016)), INT32))])
    add("long_forced", info=[("IV", ints([5, 6], INT8, long=True))], ident="x" * 40)
    # missing values in a vector
    add("miss_front", info=[("IV", ints([M8, 2, 3]))])
    add("miss_middle", info=[("IV", ints([1, M16, 3], INT16))])
    add("miss_end", info=[("IV", ints([1, 2, M32], INT32))])
    add("miss_all", info=[("IV", ints([M8, M8]))])
    add("miss_scalar", info=[("DP", ints([M8]))])
    add("count0", info=[("DP", NULL)])
    # strings
    add("comma_list", info=[("ST", string(",a,b,c"))])
    add("comma_only", info=[("ST", string(","))])
    add("nul_tail", info=[("ST", string(b"ab\0\0"))], ident=b"id\0")
    add("nul_only", info=[("ST", string(b"\0\0"))])
    add("flag_stored", info=[("DB", ints([7])), ("ZZ", ints([3]))])
    add("info_order", info=[("ST", string("s")), ("DP", ints([1])), ("AA", string("G")), ("DB", NULL)])
    add("info_twice", info=[("DP", ints([1])), ("AA", string("G")), ("DP", ints([2]))])
    # FILTER
    add("filter_null", filt=None)
    add("filter_one", filt=["q10"])
    add("filter_three", filt=["zz9", "aa1", "q10"])
    add("filter_dup", filt=["s50", "PASS", "s50"])
    # QUAL
    add("qual_missing", qual=None)
    add("qual_0", qual=0.0)
    add("qual_29_6", qual=29.6)
    add("qual_tie", qual=0.125)
    add("qual_1e7", qual=1e7)
    add("qual_neg0", qual=0x80000000)
    add("qual_big", qual=9999999.0)
    add("qual_small", qual=0.004)
    # INFO floats
    for i, v in enumerate([0.0, 0.0099999, 0.01, 0.0625, 0.9996, 1.0, 2.125, 1e-21, -1.0, float("nan"),
                           0x80000000, 0x3C23D70B, 9999999.0, 1e7, float("inf"), 0.5, 123.456]):
        add("float_%d" % i, info=[("FV", floats([v]))])
    add("float_vec", info=[("AF", floats([0.25, MISSF, 0.75]))])
    add("float_vec_missing", info=[("AF", floats([MISSF, MISSF]))])
    # alleles
    add("allele_lower", alleles=("acgtn", "<del>", "a[c1:5[", ".A", "g.", "]c1:9]t"))
    add("allele_dot", alleles=("A", "."))
    add("allele_ref_only", alleles=("g",), fmt=[("GT", INT8, 2, [[2, 2], [2, 2], [0, 2]])])
    add("no_id_no_info", ident=None, chrom=1)
    # genotypes: ploidy 1, 2, 3, a shorter sample, the '.' allele
    add("ploidy1", fmt=[("GT", INT8, 1, [[2], [4], [0]])])
    add("ploidy3", fmt=[("GT", INT8, 3, [[2, 4, 2], [3, 5, M8], [4, 0, 4]])])
    add("gt16", fmt=[("GT", INT16, 2, [[2, 4], [5, 3], [0, 0]])])
    add("gt_absent_dp", fmt=[("DP", INT8, 1, [[5], [M8], [7]])])
    add("gt_dp_gq", fmt=[gt3, ("GQ", INT8, 1, [[M8], [M8], [M8]]), ("DP", INT16, 1, [[300], [M16], [2]])])
    add("ad_pl", fmt=[gt3, ("PL", INT8, 3, [[0, 10, 20], [M8, 1, 2], [5, M8, 7]]),
                      ("AD", INT8, 2, [[3, 4], [1, 2], [M8, M8]])])
    add("generic_null", alleles=("A", "C", "G"),
        fmt=[gt3, ("HQ", INT8, 2, [[1, 2], [M8, M8], [M8, M8]]), ("XA", INT8, 2, [[1, 2], [M8, M8], [M8, M8]]),
             ("XR", INT8, 3, [[1, 2, 3], [M8, M8, M8], [M8, M8, M8]]), ("DP", INT8, 1, [[1], [2], [M8]]),
             ("ZQ", INT8, 1, [[7], [8], [9]])])
    add("generic_null_last", alleles=("A", "C", "G"),
        fmt=[gt3, ("XR", INT8, 3, [[1, 2, 3], [M8, M8, M8], [4, M8, 6]]), ("HQ", INT8, 2, [[1, 2], [3, 4], [M8, M8]])])
    add("all_stripped", fmt=[("DP", INT8, 1, [[5], [M8], [7]]), ("HQ", INT8, 2, [[1, 2], [M8, M8], [3, 4]])])
    add("field_count0", fmt=[gt3, ("HQ", NULL), ("DP", INT8, 1, [[1], [2], [3]])])
    add("x1_dot", fmt=[gt3, ("X1", INT8, 2, [[1, 2], [M8, M8], [3, M8]])])
    # deferred genotype blocks
    add("fmt_float", fmt=[gt3, ("XF", FLOAT, 1, [[0.5], [MISSF], [1e-9]])])
    add("fmt_char", fmt=[gt3, ("XS", CHAR, 3, [b"ab", b".", b"xyz"])])
    add("fmt_ft", fmt=[gt3, ("FT", CHAR, 4, [b"PASS", b"", b"q10"])])
    add("fmt_g_null", fmt=[gt3, ("XG", INT8, 3, [[1, 2, 3], [M8, M8, M8], [4, 5, 6]])])
    add("fmt_g_full", fmt=[gt3, ("XG", INT8, 3, [[1, 2, 3], [7, 8, 9], [4, 5, 6]])])
    add("ploidy17", fmt=[("GT", INT8, 17, [[2] * 17, [4] * 17, [2] * 16 + [M8]])])
    add("filter_65", filt=[i % 5 for i in range(65)])
    add("info_65", info=[("DP", ints([i])) for i in range(65)])
    add("fmt_twice", fmt=[gt3, ("HQ", INT8, 2, [[1, 2], [3, 4], [5, 6]]), ("HQ", INT8, 2, [[7, 8], [M8, M8], [9, 9]])])
    return e, out


def crafted_many_fields():
    """17 genotype fields (above the cap) under a header of its own -> (Enc, record)."""
    extra = [("Y%02d" % i, "1", "Integer") for i in range(16)]
    e = craft_encoder(extra_fmt=extra)
    fmt = [("GT", INT8, 2, [[2, 4], [2, 2], [4, 4]])] + [(n, INT8, 1, [[i], [i + 1], [i + 2]]) for i, (n, _, _) in enumerate(extra)]
    return e, e.record(pos=7, fmt=fmt)


def status_cases():
    """-> (Enc, [(name, record, status)]), one per error of the rule list (and of the frame)."""
    e = craft_encoder()
    M8 = MISS[INT8]
    gt3 = ("GT", INT8, 2, [[2, 4], [2, 2], [4, 4]])
    ok = e.record(fmt=[gt3])
    cut = bytearray(e.record(info=[("IV", ints([1, 2, 3]))], fmt=[gt3]))
    ls = struct.unpack_from("<I", cut, 0)[0]
    shared_cut = bytes(cut[:4]) + bytes(cut[4:8]) + bytes(cut[8:8 + ls - 2]) + bytes(cut[8 + ls:])
    shared_cut = struct.pack("<I", ls - 2) + shared_cut[4:]
    li = struct.unpack_from("<I", ok, 4)[0]
    indiv_cut = ok[:4] + struct.pack("<I", li - 1) + ok[8:-1]
    return e, [
        ("empty_allele", e.record(alleles=("A", b""), fmt=[gt3]), R.ERUNTIME),
        ("info_no_line", e.record(info=[("NOLINE", ints([1]))], fmt=[gt3]), R.ETRIBBLE),
        ("format_no_line", e.record(fmt=[gt3, ("NOLINE", INT8, 1, [[1], [2], [3]])]), R.ERUNTIME),
        ("gt_range", e.record(fmt=[("GT", INT8, 2, [[2, 4], [2, 6], [4, 4]])]), R.ERUNTIME),
        ("gt_eov", e.record(fmt=[("GT", INT8, 2, [[2, 4], [2, -127], [4, 4]])]), R.ERUNTIME),
        ("gt_null_sample", e.record(fmt=[("GT", INT8, 2, [[2, 4], [M8, M8], [4, 4]])]), R.ERUNTIME),
        ("no_keys_no_gt", e.record(fmt=[("DP", INT8, 1, [[M8], [M8], [M8]])]), R.ERUNTIME),
        ("dp_vector", e.record(fmt=[gt3, ("DP", INT8, 2, [[1, 2], [3, 4], [5, 6]])]), R.EUNSUPPORTED),
        ("indiv_past", indiv_cut, R.ETRIBBLE),
        ("shared_past", shared_cut, R.ETRIBBLE),
        ("chrom_range", e.record(chrom=2, fmt=[gt3]), R.ERUNTIME),
        ("sample_count", e.record(fmt=[("GT", INT8, 2, [[2, 4], [2, 2]])], n_sample=2), R.ETRIBBLE),
        ("filter_range", e.record(filt=[200 - 256], fmt=[gt3]), R.ERUNTIME),
        ("frame_past", ok[:4] + struct.pack("<I", 1 << 20) + ok[8:], R.ETRIBBLE),
    ]


def stop_streams():
    """-> [(name, Enc, records, n, status, deferred)]: 130 records with deferred ones at 3, 63 and 100, a
    failing record at 64 and another, of another status, at 90.  "lanes": three samples, a record of 17
    genotype fields deferred; "waves": 70 samples, so the samples' checks and the deferral (a null
    value under Number=G) are the wave pass's."""
    extra = [("Y%02d" % i, "1", "Integer") for i in range(16)]
    e = craft_encoder(extra_fmt=extra)
    gt3 = ("GT", INT8, 2, [[2, 4], [2, 2], [4, 4]])
    many = e.record(pos=7, fmt=[gt3] + [(n, INT8, 1, [[i], [i + 1], [i + 2]]) for i, (n, _, _) in enumerate(extra)])
    lanes = varied_records(e, 130)
    lanes[64] = e.record(fmt=[gt3, ("DP", INT8, 2, [[1, 2], [3, 4], [5, 6]])])  # status_cases' dp_vector
    lanes[90] = e.record(info=[("NOLINE", ints([1]))], fmt=[gt3])               # ... and info_no_line
    ns = 70
    w = craft_encoder(samples=tuple("N%d" % i for i in range(ns)))
    gt = [[2, 4]] * ns
    ok = w.record(pos=1, fmt=[("GT", INT8, 2, gt), ("DP", INT8, 1, [[s % 100] for s in range(ns)])])
    g_null = w.record(pos=4, fmt=[("GT", INT8, 2, gt),
                                  ("XG", INT8, 3, [[1, 2, 3]] * 65 + [[MISS[INT8]] * 3] + [[4, 5, 6]] * 4)])
    waves = [ok] * 130
    waves[64] = w.record(pos=2, fmt=[("GT", INT8, 2, gt[:68] + [[2, 8]] + gt[69:])])  # an allele the record lacks
    waves[90] = w.record(pos=3, fmt=[("DP", INT8, 2, [[1, 2]] * ns)])
    for k in (3, 63, 100):
        lanes[k], waves[k] = many, g_null
    return [("lanes", e, lanes, 64, R.EUNSUPPORTED, [3, 63]), ("waves", w, waves, 64, R.ERUNTIME, [3, 63])]


def sample_records(n_sample, n_rec=8, seed=3):
    """Records of n_sample samples with GT, DP, one Number=2 generic field and ragged trailing-missing
    samples; nothing in them is deferred -> (Enc, [record])."""
    rng = np.random.default_rng(seed + n_sample)
    e = craft_encoder(samples=tuple("N%d" % i for i in range(n_sample)))
    M8, M16 = MISS[INT8], MISS[INT16]
    recs = []
    for r in range(n_rec):
        gts, dps, hqs = [], [], []
        for s in range(n_sample):
            ph = int(rng.integers(0, 2))
            gts.append([int(rng.integers(0, 3)) << 1 | ph, int(rng.integers(0, 3)) << 1 | ph])
            dps.append([M16 if rng.random() < 0.3 else int(rng.integers(0, 1000))])
            hqs.append([M8, M8] if rng.random() < 0.5 else [int(rng.integers(0, 99)), int(rng.integers(-9, 99))])
        fmt = [("HQ", INT8, 2, hqs), ("GT", INT8, 2, gts), ("DP", INT16, 1, dps)] if n_sample else []
        recs.append(e.record(chrom=r % 2, pos=1000 * r + 5, ident="r%d" % r if r % 3 else None,
                             alleles=("A", "C", "G")[:2 + r % 2], qual=float(r * 7) + 0.5, filt=["PASS"],
                             info=[("DP", ints([r * 37], INT16))], fmt=fmt, n_sample=n_sample))
    return e, recs


def varied_records(e, n, seed=11):
    """n records whose lines have varying lengths (IDs of 0..40 bytes), so that lines start at every
    offset mod 16; none is deferred."""
    rng = np.random.default_rng(seed)
    gt3 = ("GT", INT8, 2, [[2, 4], [2, 2], [4, 4]])
    return [e.record(chrom=i % 2, pos=10 * i, ident="i" * int(rng.integers(0, 41)) or None, qual=float(i % 90),
                     filt=["q10"] if i % 4 == 0 else ["PASS"], info=[("DP", ints([i % 100]))],
                     fmt=[gt3, ("DP", INT8, 1, [[i % 50], [1], [MISS[INT8]]])]) for i in range(n)]


def host_input(e, records, wave_cut=64):
    """The input file of tools/vcf_text_host.cpp: the header's tables as hbam_vcf_meta holds them (built
    here from the vcftext_ref header, not by hadoop_bam) and the records."""
    h = e.hdr
    kinds = {"GT": 1, "DP": 2, "GQ": 3, "AD": 4, "PL": 5, "FT": 6}
    numbers = {".": -1, "A": -2, "R": -3, "G": -4, None: -1}

    def cat(names):
        off = np.zeros(len(names) + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in names])
        return off.tobytes() + "".join(names).encode("latin-1")
    flags, number = [], []
    for name in h["dict"]:
        f, num = 0, 0
        if name in h["info"]:
            f |= 1 | (2 if h["info"][name][1] == "Flag" or h["info"][name][0] == "0" else 0)
        if name in h["format"]:
            f |= 4 | kinds.get(name, 0) << 4
            x = h["format"][name][0]
            num = numbers[x] if x in numbers else int(x)
        flags.append(f)
        number.append(num)
    data, off = pack(records)
    return (struct.pack("<iiiI", len(h["contigs"]), len(h["dict"]), len(h["samples"]), wave_cut) + cat(h["contigs"]) +
            cat(h["dict"]) + np.array(h["rank"], np.uint32).tobytes() + np.array(flags, np.uint32).tobytes() +
            np.array(number, np.int32).tobytes() + struct.pack("<Q", len(records)) + off.tobytes() +
            struct.pack("<Q", len(data)) + data)
