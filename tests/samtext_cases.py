"""Crafted BAM records for tests/test_samtext.py and tests/test_samtext_gpu.py: the smallest shapes
at which the SAM text renderer can go wrong, and one record per status of hbam_sam_render's lists."""
import struct

import numpy as np

import f4_records
import sam_cases
import sam_ref
import samtext_ref

NAMES = sam_cases.REF_NAMES
N_REF = len(NAMES)
E, R = samtext_ref.HBAM_EFORMAT, samtext_ref.HBAM_EREFID

# float32 values the device renders itself ...
DEVICE_FLOATS = [1.0, -3.0, 0.0, -0.0, 9999999.0, -9999999.0, 8388608.0, 2.0, 1234567.0, 65536.0, -1.0]
# ... and values just outside that domain
HOST_FLOATS = [1e7, -1e7, 0.5, -0.5, 999999.5, 0.1, 1e-3, 9.999e-4, 1.6777216e7, 3.4028235e38, 1.4e-45,
               float("nan"), float("inf"), float("-inf"), 1.5, 4194304.5, 0.99999994, 16777216.0]


def crafted_records():
    """The 95 crafted lines of the input side as BAM records."""
    return [sam_ref.parse_encode(ln, sam_cases.DICT) for ln in sam_cases.crafted_lines()]


def aux_f(tag, v):
    return tag.encode() + b"f" + struct.pack("<f", v)


def aux_bf(tag, vals):
    return tag.encode() + b"Bf" + struct.pack("<i", len(vals)) + b"".join(struct.pack("<f", v) for v in vals)


def aux_h(tag, hexes):
    return tag.encode() + b"H" + hexes + b"\0"


def float_records():
    """[(record, deferred?)]: floats inside the device's domain singly and in B:f (rendered by the
    device), each value just outside it singly and as the last element of a B:f, an H tag, and an
    empty B:f."""
    def rec(name, pos=0, cigar=((10, 0),), **kw):  # with the bin the input side computes: they read back
        return f4_records.record(name, pos=pos, cigar=cigar, bin_=sam_ref.reg2bin(pos, pos + cigar[0][0]), **kw)
    out = []
    for k, v in enumerate(DEVICE_FLOATS):
        out.append((rec(b"fd%d" % k, ref=k % 4, pos=10 + k, l_seq=10 + 2 * k, cigar=((10 + 2 * k, 0),), aux=aux_f("XF", v),
                        seed=500 + k), False))
    out.append((rec(b"fdB", ref=1, pos=50, aux=aux_bf("XB", DEVICE_FLOATS) + f4_records.aux_int("NM", "c", 3),
                    seed=520), False))
    out.append((rec(b"fdB0", ref=1, pos=51, aux=aux_bf("XB", []), seed=521), False))
    for k, v in enumerate(HOST_FLOATS):
        out.append((rec(b"fh%d" % k, ref=k % 4, pos=100 + k, aux=f4_records.aux_z("XZ", "z") + aux_f("XF", v),
                        seed=540 + k), True))
        out.append((rec(b"fhB%d" % k, ref=k % 4, pos=200 + k, aux=aux_bf("XB", [1.0, 2.0, v]), seed=560 + k), True))
    out.append((rec(b"hexed", ref=2, pos=300, aux=aux_h("XH", b"1AE301") + f4_records.aux_int("NM", "c", 1),
                    seed=580), True))
    out.append((rec(b"hex0", ref=2, pos=301, aux=aux_h("XH", b""), seed=581), True))
    return out


EDGE_LSEQ = (1, 15, 16, 17, 31, 32, 33)


def edge_records(n):
    """n records for the tile and alignment edges: name lengths 1-16 (the SEQ region starts at every
    output offset mod 16), l_seq over EDGE_LSEQ, every seventh QUAL absent, one read of about 6 KB
    (record 5), a tag on every third."""
    out = []
    for k in range(n):
        ls = 6001 if k == 5 else EDGE_LSEQ[k % len(EDGE_LSEQ)]
        name = b"abcdefghijklmnop"[:1 + k % 16]
        aux = f4_records.aux_int("NM", "C", k % 200) if k % 3 == 0 else b""
        out.append(f4_records.record(name, flag=k % 3, ref=k % 4, pos=100 * k, cigar=((ls, 0),), l_seq=ls, aux=aux,
                                     nref=(k % 4 if k % 2 else -1), npos=5 * k, tlen=k - 60,
                                     qual_absent=(k % 7 == 3), seed=700 + k))
    return out


def good_record(k):
    return f4_records.record(b"g%03d" % k, flag=(4 if k % 9 == 0 else 0), ref=k % 4, pos=10 * k, l_seq=45,
                             cigar=((45, 0),), aux=f4_records.aux_int("NM", "C", k % 200), seed=400 + k)


def _patched(rec, fmt, at, value):
    b = bytearray(rec)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def _with_aux(aux):
    """good_record(999)'s fields with this aux block"""
    return f4_records.record(b"g999", ref=3, pos=9990, l_seq=45, cigar=((45, 0),), aux=aux, seed=1399)


def _with_qual(at, value):
    g = good_record(999)
    q = 36 + 5 + 4 + 23 + at
    return g[:q] + bytes([value]) + g[q + 1:]


def _reaux(rec, old, aux):
    """rec with its last `old` aux bytes replaced by aux"""
    b = rec[:len(rec) - old] + aux
    return struct.pack("<i", len(b) - 4) + b[4:]


def status_cases():
    """[(name, expected status, the bytes of the record's rec_off slot)]: every status of the
    header's two lists, each made from one good record; the slot keeps the good record's size where
    block_size is what lies."""
    g = good_record(999)
    bs = len(g) - 4
    fixed = 32 + 5 + 4 + 23 + 45  # the record up to its tags
    nm = f4_records.aux_int("NM", "C", 7)
    C = [
        ("block_size_below_fields", E, _patched(g, "<i", 0, fixed - 1)),
        ("block_size_below_32", E, _patched(g, "<i", 0, 31)),
        ("block_size_negative", E, _patched(g, "<i", 0, -5)),
        ("block_size_past_slot", E, _patched(g, "<i", 0, bs + 100)),
        ("block_size_huge", E, _patched(g, "<i", 0, 0x7fffffff)),
        ("l_read_name_0", E, _patched(g, "<B", 12, 0)),
        ("l_seq_negative", E, _patched(g, "<i", 20, -1)),
        ("l_seq_huge", E, _patched(g, "<i", 20, 0x7fffffff)),
        ("n_cigar_past_record", E, _patched(g, "<H", 16, 60000)),
        ("tag_two_bytes", E, _with_aux(nm + b"XY")),
        ("tag_int_cut", E, _with_aux(nm + b"XYi\x01\x02")),
        ("tag_float_cut", E, _with_aux(b"XYf\x00\x00\x80")),
        ("tag_A_cut", E, _with_aux(nm + b"XYA")),
        ("tag_B_header_cut", E, _with_aux(nm + b"XYBc\x01\x00")),
        ("tag_B_past_record", E, _with_aux(nm + b"XYBs" + struct.pack("<i", 3) + b"\x01\x00\x02\x00\x03")),
        ("tag_B_count_2_30", E, _with_aux(b"XYBi" + struct.pack("<i", 1 << 30) + b"\0" * 8)),
        ("tag_type_unknown", E, _with_aux(nm + b"XYq\x05")),
        ("tag_B_subtype_unknown", E, _with_aux(nm + b"XYBd" + struct.pack("<i", 1) + b"\0" * 8)),
        ("tag_B_subtype_A", E, _with_aux(nm + b"XYBA" + struct.pack("<i", 1) + b"Q")),
        ("tag_B_count_negative", E, _with_aux(nm + b"XYBc" + struct.pack("<i", -1))),
        ("tag_Z_without_NUL", E, _with_aux(nm + b"XYZhello")),
        ("tag_H_without_NUL", E, _with_aux(b"XYH1A")),
        ("ref_id_n_ref", R, _patched(g, "<i", 4, N_REF)),
        ("ref_id_minus_2", R, _patched(g, "<i", 4, -2)),
        ("next_ref_id_n_ref", R, _patched(g, "<i", 24, N_REF)),
        ("next_ref_id_minus_2", R, _patched(g, "<i", 24, -2)),
        ("cigar_op_9", R, f4_records.record(b"g999", ref=3, pos=9990, l_seq=45, raw_ops=[(40 << 4) | 0, (5 << 4) | 9],
                                            aux=nm, seed=1399)),
        ("qual_94_first", R, _with_qual(0, 94)),
        ("qual_94_at_17", R, _with_qual(17, 94)),
        ("qual_200_last", R, _with_qual(44, 200)),
        ("qual_ff_not_first", R, _with_qual(30, 0xff)),
        ("qual_94_in_a_deferred_record", R, _reaux(_with_qual(20, 94), 4, aux_f("XF", 0.5))),
    ]
    return C


def stream(case_slot, at, total=130):
    """`total` record slots, the failing one at index `at`."""
    recs = [good_record(k) for k in range(total)]
    recs[at] = case_slot
    return recs


def deferred_record(k):
    """good_record(k) with its NM tag replaced by a float outside the device's domain"""
    return _reaux(good_record(k), 4, aux_f("XF", 0.5))


def stop_streams():
    """[(name, slots, n, status, deferred)]: 130 records with deferred ones at 3, 63 and 100, and one or
    two failing records: a malformed tag (found when the lines are sized) and a quality byte of 94
    (found when SEQ and QUAL are written).  The first failing record in output order ends the output,
    and only the deferred records before it are listed."""
    malformed = _with_aux(f4_records.aux_int("NM", "C", 7) + b"XY")
    quality = _with_qual(17, 94)

    def make(bad):
        recs = [good_record(k) for k in range(130)]
        for k in (3, 63, 100):
            recs[k] = deferred_record(k)
        for k, slot in bad.items():
            recs[k] = slot
        return recs
    return [
        ("malformed_64", make({64: malformed}), 64, E, [3, 63]),
        ("quality_64", make({64: quality}), 64, R, [3, 63]),
        ("quality_101", make({101: quality}), 101, R, [3, 63, 100]),
        ("malformed_100_quality_40", make({100: malformed, 40: quality}), 40, R, [3]),
        ("quality_120_malformed_100", make({120: quality, 100: malformed}), 100, E, [3, 63]),
    ]


def host_input(slots, names=NAMES):
    """The input file of tools/sam_text_host.cpp."""
    noff = np.zeros(len(names) + 1, np.uint32)
    noff[1:] = np.cumsum([len(x) for x in names])
    ub, off = f4_records.pack(slots)
    return (struct.pack("<i", len(names)) + noff.tobytes() + b"".join(names) + struct.pack("<Q", len(slots)) +
            off.tobytes() + ub.tobytes())
