"""Crafted SAM text for tests/test_sam.py and tests/test_sam_gpu.py: the smallest shapes at which
the SAM kernels can go wrong, and one line per error of hbam_sam_decode_split's lists."""
import f4_records
import helpers
import sam_ref

REFS = [(b"chr1", 1000000), (b"chr2", 2000000), (b"chrM", 16571), (b"GL000207.1", 4262)]
REF_NAMES = [n for n, _ in REFS]
HEADER = [b"@HD\tVN:1.4\tSO:unsorted"] + [b"@SQ\tSN:%s\tLN:%d" % r for r in REFS] + [b"@PG\tID:craft"]
DICT = {n: i for i, n in enumerate(REF_NAMES)}

INT_BOUNDS = [-(1 << 31), -32769, -32768, -129, -128, 127, 128, 255, 256, 32767, 32768, 65535, 65536,
              (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
# the type each boundary value is written with (the issue's width table)
INT_TYPES = ["i", "i", "s", "s", "c", "c", "C", "C", "s", "s", "S", "S", "i", "i", "I", "I"]


# float text at and next to float32 halfway points, and the float32 it must become: a tie goes
# to the even mantissa
HALFWAY = [
    (b"16777217", 16777216.0), (b"16777219", 16777220.0), (b"16777217.1", 16777218.0),
    (b"16777216.9", 16777216.0), (b"1.6777217e7", 16777216.0), (b"167772170E-1", 16777216.0),
    (b"33554434", 33554432.0), (b"33554438", 33554440.0), (b"33554434.1", 33554436.0),
    (b"8388608.5", 8388608.0), (b"8388609.5", 8388610.0), (b"8388608.51", 8388609.0),
    (b"8388608.49", 8388608.0), (b"4194304.25", 4194304.0), (b"4194304.75", 4194305.0),
    (b"4194304.26", 4194304.5), (b"-16777217", -16777216.0), (b"-8388609.5", -8388610.0),
    (b"1.6777217e27", 1.6777217e27), (b"1e-20", 1e-20), (b"999999999e20", 999999999e20),
    (b"0.1", 0.1), (b"0.3", 0.3), (b"3.4028235e20", 3.4028235e20),
]


def _line(rec):
    return sam_ref.render([rec], REF_NAMES)[0]


def _with_field(line, k, value):
    f = line.split(b"\t")
    f[k] = value
    return b"\t".join(f)


def every_tag():
    """One tag of every type, B arrays of every subtype with 1 and with 70 elements, the integer
    boundary values (as text: the renderer writes every integer as i)."""
    tags = [b"XA:A:Q", b"XZ:Z:hello world", b"XE:Z:x", b"XF:f:1.5", b"XG:f:-3.1415927", b"XH:f:1e-05",
            b"XI:f:16777217", b"XJ:f:0", b"XK:f:-0.0", b"XL:f:6.02e+20", b"XM:f:.5", b"XN:f:5.E-3"]
    for k, v in enumerate(INT_BOUNDS):
        tags.append(b"I%c:i:%d" % (65 + k, v))
    tags.append(b"IZ:i:+12")
    lim = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535),
           "i": (-(1 << 31), (1 << 31) - 1), "I": (0, (1 << 32) - 1)}
    for j, sub in enumerate("cCsSiI"):
        lo, hi = lim[sub]
        tags.append(b"B%c:B:%s,%d" % (97 + j, sub.encode(), lo))
        vals = [lo, hi] + [(lo + 37 * k * (hi - lo) // 2500) for k in range(68)]
        tags.append(b"C%c:B:%s,%s" % (97 + j, sub.encode(), b",".join(b"%d" % v for v in vals)))
    tags.append(b"Bf:B:f,0.1")
    tags.append(b"Cf:B:f," + b",".join(b"%d.%de%d" % (k, 7 * k % 1000, k % 25 - 12) for k in range(70)))
    tags.append(b"BE:B:c")  # an array without elements
    tags.append(b"HF:B:f," + b",".join(t for t, _ in HALFWAY))
    tags += [b"H%c:f:%s" % (65 + k, t) for k, (t, _) in enumerate(HALFWAY)]
    return tags


def crafted_lines():
    """Lines only (no header); placed and unplaced records mixed."""
    R = f4_records.record
    L = []
    for ls in (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        L.append(_line(R(b"ls%d" % ls, ref=0, pos=100 + ls, cigar=((max(ls, 1), 0),), l_seq=ls, seed=ls)))
    L.append(_line(R(b"long", ref=1, pos=5000, cigar=((3001, 0),), l_seq=3001, seed=77)))  # > one 4 KiB tile
    L.append(_line(R(b"n", ref=0, pos=1, seed=1)))
    L.append(_line(R(b"N" * 254, ref=0, pos=2, seed=2)))
    L.append(_line(R(b"c0", ref=0, pos=3, cigar=(), seed=3)))
    L.append(_line(R(b"c1", ref=0, pos=4, cigar=((10, 0),), seed=4)))
    L.append(_line(R(b"c300", ref=2, pos=5, cigar=tuple((1 + k % 7, k % 9) for k in range(300)), l_seq=50, seed=5)))
    L.append(_line(R(b"bigop", ref=0, pos=6, cigar=(((1 << 28) - 1, 3), (5, 0)), l_seq=5, seed=6)))
    L.append(_line(R(b"qstar", ref=0, pos=7, l_seq=37, cigar=((37, 0),), qual_absent=True, seed=7)))
    low = _line(R(b"lower", ref=0, pos=8, l_seq=70, cigar=((70, 0),), seed=8)).split(b"\t")
    low[9] = low[9].lower().replace(b"n", b".")
    L.append(b"\t".join(low))
    L.append(_line(R(b"rn_eq", flag=1, ref=1, pos=9, nref=1, npos=500, tlen=491, seed=9)))
    L.append(_line(R(b"rn_star", flag=1, ref=1, pos=10, nref=-1, npos=-1, seed=10)))
    L.append(_line(R(b"rn_name", flag=1, ref=1, pos=11, nref=3, npos=77, seed=11)))
    L.append(_with_field(_line(R(b"unk", ref=1, pos=12, nref=1, npos=5, seed=12)), 2, b"chrUnknown"))
    L.append(_with_field(_line(R(b"unk_next", ref=1, pos=13, seed=13)), 6, b"chrUnknown"))
    L.append(_line(R(b"pos0", flag=0, ref=0, pos=-1, seed=14)))  # POS 0: start 0 is not < 0, a placed key with low half -1
    L.append(_line(R(b"mapped_end", flag=16, ref=3, pos=(1 << 29) - 10, cigar=((100, 0),), l_seq=100, seed=15)))
    L.append(_line(R(b"tags", ref=0, pos=16, seed=16)) + b"\t" + b"\t".join(every_tag()))
    for k in range(64):  # a whole wave takes the key override
        L.append(_line(R(b"unpl%02d" % k, flag=4 | (1 if k % 2 else 0), ref=-1, pos=-1, cigar=(), l_seq=k + 1,
                         qual_absent=(k % 5 == 0), seed=100 + k)))
    L.append(_line(R(b"unm_placed", flag=4, ref=2, pos=300, cigar=(), l_seq=20, seed=17)))
    return L


BOUNDARIES = (16, 1024, 4096)


def boundary_file(eol=b"\n", base=None):
    """The header, then lines padded (a Z tag) so that their ends (the offset after the line end's
    last byte) fall one before, exactly at and one after a 16-byte, a 1 KiB and a 4 KiB boundary of
    the structural pass, then a last line without a line end.  The pass's grid is anchored at the
    window's first byte: `base` is that byte's file offset (None: data_start, the window the reader
    opens for the split at 0).  -> (file bytes, [(boundary, end offset)])"""
    out = sam_ref.sam_file(HEADER, [], eol)
    base = len(out) if base is None else base
    k, ends = 0, []
    for boundary in BOUNDARIES:
        for delta in (-1, 0, 1):
            line = _line(f4_records.record(b"b%d" % k, ref=k % 4, pos=1000 + k, l_seq=20 + k, cigar=((20 + k, 0),),
                                           seed=200 + k)) + b"\tXP:Z:"
            need = len(out) + len(line) + 1 + len(eol)  # with one byte of padding
            target = base + (need - base + boundary - 1) // boundary * boundary + delta
            if target < need:
                target += boundary
            out += line + b"p" * (1 + target - need) + eol
            assert len(out) == target
            ends.append((boundary, target))
            k += 1
    return out + _line(f4_records.record(b"last", ref=0, pos=9, seed=300)), ends


def good_line(k):
    return _line(f4_records.record(b"g%03d" % k, flag=(4 if k % 9 == 0 else 0), ref=k % 4, pos=10 * k, l_seq=45,
                                   cigar=((45, 0),), aux=f4_records.aux_int("NM", "C", k % 200), seed=400 + k))


def _bad_seq(line):
    f = line.split(b"\t")
    f[9] = f[9][:40] + b"J" + f[9][41:]
    return b"\t".join(f)


def _bad_qual(line):
    f = line.split(b"\t")
    f[10] = f[10][:44] + b" "
    return b"\t".join(f)


def error_cases():
    """[(name, expected status, line)]: every error of the two lists, made from one good line."""
    g = good_line(999)
    f = g.split(b"\t")
    E, U = sam_ref.HBAM_EFORMAT, sam_ref.HBAM_EUNSUPPORTED
    C = [
        ("ten_fields", E, b"\t".join(f[:10])),
        ("pos_not_numeric", E, _with_field(g, 3, b"12x")),
        ("flag_sign_only", E, _with_field(g, 1, b"-")),
        ("tlen_out_of_range", E, _with_field(g, 8, b"2147483648")),
        ("pnext_out_of_range", E, _with_field(g, 7, b"-2147483649")),
        ("empty_mapq", E, _with_field(g, 4, b"")),
        ("empty_tag", E, g + b"\t"),
        ("cigar_bad_op", E, _with_field(g, 5, b"40M5Q")),
        ("cigar_no_length", E, _with_field(g, 5, b"M45")),
        ("cigar_no_op", E, _with_field(g, 5, b"45")),
        ("cigar_length_2_28", E, _with_field(g, 5, b"268435456N45M")),
        ("seq_byte", E, _bad_seq(g)),
        ("qual_length", E, _with_field(g, 10, f[10][:-1])),
        ("qual_with_seq_star", E, _with_field(g, 9, b"*")),
        ("qual_byte", E, _bad_qual(g)),
        ("tag_short", E, g + b"\tXX:i"),
        ("tag_no_colon", E, g + b"\tXXi:5:1"),
        ("tag_type", E, g + b"\tXX:q:5"),
        ("tag_A_two_bytes", E, g + b"\tXX:A:ab"),
        ("tag_B_subtype", E, g + b"\tXX:B:d,1"),
        ("tag_B_range", E, g + b"\tXX:B:C,1,256"),
        ("tag_B_empty_element", E, g + b"\tXX:B:s,1,,2"),
        ("tag_i_text", E, g + b"\tXX:i:1.5"),
        ("tag_i_above", E, g + b"\tXX:i:4294967296"),
        ("tag_i_below", E, g + b"\tXX:i:-2147483649"),
        ("tag_H", U, g + b"\tXX:H:1AE3"),
        ("name_255", U, _with_field(g, 0, b"q" * 255)),
        ("cigar_65536_ops", U, _with_field(_with_field(_with_field(g, 5, b"1M" * 65536), 9, b"*"), 10, b"*")),
        ("float_10_digits", U, g + b"\tXX:f:1.234567891"),
        ("float_exponent", U, g + b"\tXX:f:1e40"),
        ("float_nan", U, g + b"\tXX:f:nan"),
        ("float_array", U, g + b"\tXX:B:f,1.0,1e-30"),
    ]
    return C


def error_file(line, at, total=130):
    """`total` lines, the failing one at index `at`."""
    lines = [good_line(k) for k in range(total)]
    lines[at] = line
    return sam_ref.sam_file(HEADER, lines)


def bam_header_and_records(data):
    """(SAMFileHeader, [block_size + record]) of a whole BAM, through zlib."""
    from hadoop_bam.output import SAMFileHeader
    u = helpers.bam_stream(data)
    h = SAMFileHeader.from_bam_bytes(u)
    return h, sam_ref.split_records(u[len(h.to_bam_bytes()):])


def sam_of_bam(data, eol=b"\n"):
    """A BAM rendered as SAM text -> (the file's bytes, its SAMFileHeader)"""
    h, recs = bam_header_and_records(data)
    lines = sam_ref.render(recs, [n for n, _ in h.refs])
    return sam_ref.sam_file(sam_ref.header_text(h.text, h.refs), lines, eol), h
