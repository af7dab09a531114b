"""BCF2 site-decode cases with stated answers.

CASES is a list of (label, record bytes, expected status).  The expected status is written by hand
from the rules listed at the top of oracle/hbam_oracle_bcf.c (1: sizes, 2: CHROM / sample count /
isValid, 3: typed values, 4: genotype bytes); it is computed by neither implementation:
    OK (0)    the record decodes
    TRIBBLE   htsjdk TribbleException
    RUNTIME   another RuntimeException that escapes BCF2Codec.decode
Each record is placed as record K of a short valid stream (stream(rec)) and followed by TAIL valid
records: a failing record ends the read with n = K and its status, the later records never appear;
a record that decodes gives n = K + 1 + TAIL and status 0.

The header is bcf_records.header_text(): 25 contigs, 3 samples, a string dictionary of 6.
"""
import struct

import bcf_records as br
import chain_craft as cc

OK, TRIBBLE, RUNTIME = 0, -14, -15
K, TAIL = 3, 3
N_CONTIG, N_SAMPLE, N_DICT = 25, 3, 6

I8, I16, I32, FLT, CHR = 1, 2, 3, 5, 7
_PACK = {I8: "<b", I16: "<h", I32: "<i"}


def ext(t, count, ctype, payload=b"", cdesc=None):
    """A typed value with an extended count: descriptor 0xF|t, the count as a typed integer of
    type ctype (its descriptor byte: cdesc, default one element of ctype), the elements."""
    return bytes([0xf0 | t, (0x10 | ctype) if cdesc is None else cdesc]) + struct.pack(_PACK[ctype], count) + payload


def ints(vals, t):
    return bytes([len(vals) << 4 | t]) + b"".join(struct.pack(_PACK[t], v) for v in vals)


ID0 = br.typed_str("id1")
ALLELES0 = (br.typed_str("A"), br.typed_str("CT"))
FILTER0 = ints([0], I8)
INFO0 = ((br.typed_int(br.DICT["DP"]), br.typed_int(17)),)


def rec(chrom=0, pos=100, ident=ID0, alleles=ALLELES0, filt=FILTER0, info=INFO0, n_allele=None, n_info=None,
        nfs=N_SAMPLE, l_shared=None, l_indiv=None, indiv=b"", tail=b""):
    """One record.  n_allele / n_info default to what is present; nfs is the whole n_fmt_sample
    word; l_shared / l_indiv default to the bytes present (tail: further site bytes)."""
    shared = struct.pack("<iiif", chrom, pos, 1, 30.0)
    shared += struct.pack("<iI", (len(alleles) if n_allele is None else n_allele) << 16 |
                          (len(info) if n_info is None else n_info), nfs & 0xffffffff)
    shared += ident + b"".join(alleles) + filt + b"".join(k + v for k, v in info) + tail
    return struct.pack("<ii", len(shared) if l_shared is None else l_shared,
                       len(indiv) if l_indiv is None else l_indiv) + shared + indiv


def _with_value(where, v):
    """the default record with the typed value v as its ID, its second allele, its FILTER or its
    INFO value"""
    if where == "id":
        return rec(ident=v)
    if where == "allele":
        return rec(alleles=(ALLELES0[0], v))
    if where == "filter":
        return rec(filt=v)
    return rec(info=((INFO0[0][0], v),))


def _stream_parts():
    s = cc.BcfStream()
    s.add_trues(K)
    head = s.bytes()
    t = cc.BcfStream()
    t._k = K
    t.add_trues(TAIL)
    return head, t.bytes()[t.header_len:], s.header_len


HEAD, TAIL_BYTES, HEADER_LEN = _stream_parts()


def stream(record):
    """(stream bytes, offset of the crafted record)"""
    return HEAD + record + TAIL_BYTES, len(HEAD)


def _cases():
    c = []
    add = lambda label, r, st: c.append((label, r, st))  # noqa: E731
    add("default", rec(), OK)

    # ---- count forms
    for ct, nm in ((I8, "int8"), (I16, "int16"), (I32, "int32")):
        add("ext_%s_id" % nm, _with_value("id", ext(CHR, 20, ct, b"x" * 20)), OK)
        add("ext_%s_allele" % nm, _with_value("allele", ext(CHR, 20, ct, b"ACGT" * 5)), OK)
        add("ext_%s_filter" % nm, _with_value("filter", ext(I8, 16, ct, bytes([0, 1] * 8))), OK)
        add("ext_%s_info" % nm, _with_value("info", ext(I16, 20, ct, struct.pack("<20h", *range(20)))), OK)
    add("ext_count_15_id", _with_value("id", ext(CHR, 15, I8, b"y" * 15)), OK)
    add("ext_count_15_filter", _with_value("filter", ext(I8, 15, I8, bytes(15))), OK)
    add("ext_count_200_int16_info", _with_value("info", ext(I8, 200, I16, bytes(200))), OK)
    for where in ("id", "allele", "filter", "info"):
        # an empty value: the type (here none at all, a float, an undefined nibble) is never consulted
        add("ext_count_0_%s" % where, _with_value(where, ext(CHR if where in ("id", "allele") else 0, 0, I8)), OK)
        add("ext_count_neg_%s" % where, _with_value(where, ext(FLT, -1, I8)), OK)
        add("ext_count_neg16_%s" % where, _with_value(where, ext(9, -300, I16)), OK)
    for t2 in (0, 5, 7):
        # the bytes a reader that took the count's type as it came (none, 4 or 1 bytes) would accept
        cnt = {0: b"", 5: struct.pack("<i", 3), 7: b"\x03"}[t2]
        add("ext_count_type_%d" % t2, _with_value("id", bytes([0xf7, 0x10 | t2]) + cnt + (b"abc" if t2 else b"")), RUNTIME)
        add("ext_count_type_%d_info" % t2, _with_value("info", bytes([0xf1, 0x10 | t2, 2, 0, 0, 0, 1, 2])), RUNTIME)
    # the extended count cut by the end of the site block, at each of its bytes (the ID is the value)
    for ct, nm, nb in ((I8, "int8", 1), (I16, "int16", 2), (I32, "int32", 4)):
        full = rec(ident=ext(CHR, 3, ct, b"abc"))
        for have in range(0, 2 + nb):  # bytes of (descriptor, count type, count) inside the block
            r = bytearray(full)
            struct.pack_into("<ii", r, 0, 24 + have, len(full) - 8 - 24 - have)
            if have >= 1:
                add("ext_%s_cut_after_%d" % (nm, have), bytes(r), TRIBBLE)

    # ---- type nibbles
    for t in (0, 4, 6) + tuple(range(8, 16)):
        add("type_%d_count_0" % t, _with_value("info", bytes([t])), OK)
        add("type_%d_count_1" % t, _with_value("info", bytes([0x10 | t, 0])), RUNTIME)
    add("type_4_count_2_id", _with_value("id", bytes([0x24, 0, 0])), RUNTIME)
    add("info_float", _with_value("info", bytes([0x20 | FLT]) + struct.pack("<ff", 0.5, 0.25)), OK)
    add("info_char", _with_value("info", br.typed_str("abc")), OK)
    add("info_int32", _with_value("info", ints([1 << 20, -5], I32)), OK)

    # ---- FILTER and INFO keys
    add("filter_empty", rec(filt=b"\x00"), OK)
    add("filter_int8", rec(filt=ints([0, 1], I8)), OK)
    add("filter_int16", rec(filt=ints([1, 5], I16)), OK)
    add("filter_int32", rec(filt=ints([5, 0, 1], I32)), OK)
    add("filter_eq_n_dict", rec(filt=ints([N_DICT], I8)), RUNTIME)
    add("filter_eq_n_dict_second", rec(filt=ints([0, N_DICT], I16)), RUNTIME)
    add("filter_minus_1", rec(filt=ints([-1], I8)), RUNTIME)
    add("filter_minus_1_int32", rec(filt=ints([-1], I32)), RUNTIME)
    add("filter_float", rec(filt=bytes([0x10 | FLT]) + struct.pack("<f", 1.0)), RUNTIME)
    add("filter_string", rec(filt=br.typed_str("q")), RUNTIME)
    add("info_key_eq_n_dict", rec(info=((br.typed_int(N_DICT), br.typed_int(1)),)), RUNTIME)
    add("info_key_minus_1", rec(info=((br.typed_int(-1), br.typed_int(1)),)), RUNTIME)
    add("info_key_int16_in_range", rec(info=((ints([4], I16), b"\x00"),)), OK)
    add("info_key_string", rec(info=((br.typed_str("DP"), br.typed_int(1)),)), RUNTIME)
    add("n_info_0", rec(info=()), OK)
    add("n_info_3_present_1", rec(n_info=3), TRIBBLE)
    add("n_info_2_second_value_missing", rec(info=(INFO0[0], (br.typed_int(3), b""))), TRIBBLE)

    # ---- alleles
    add("n_allele_0", rec(alleles=()), TRIBBLE)
    add("n_allele_0_values_first", rec(alleles=(), info=((br.typed_int(2), bytes([0x14, 0])),)), RUNTIME)
    add("allele_int", rec(alleles=(ALLELES0[0], ints([5], I8))), RUNTIME)
    add("allele_float", rec(alleles=(bytes([0x10 | FLT]) + bytes(4),)), RUNTIME)
    add("allele_int_count_0", rec(alleles=(ALLELES0[0], bytes([I8]))), OK)
    add("allele_missing_value", rec(n_allele=3), RUNTIME)  # the FILTER's int8 vector read as the third allele

    # ---- counts word and CHROM
    add("n_fmt_0x80", rec(nfs=0x80 << 24 | N_SAMPLE), TRIBBLE)
    add("n_fmt_0x7f", rec(nfs=0x7f << 24 | N_SAMPLE), OK)
    add("n_sample_4", rec(nfs=4), TRIBBLE)
    add("n_sample_bit_19", rec(nfs=N_SAMPLE | 1 << 19), TRIBBLE)
    add("n_sample_bits_20_23", rec(nfs=N_SAMPLE | 0xf << 20), OK)
    add("chrom_eq_n_contig", rec(chrom=N_CONTIG), RUNTIME)
    add("chrom_last", rec(chrom=N_CONTIG - 1), OK)
    add("chrom_minus_1", rec(chrom=-1), RUNTIME)
    add("chrom_before_sample_count", rec(chrom=N_CONTIG, nfs=4), RUNTIME)
    add("sample_count_before_values", rec(nfs=4, filt=ints([N_DICT], I8)), TRIBBLE)
    add("filter_before_n_allele", rec(alleles=(), filt=ints([N_DICT], I8)), RUNTIME)
    add("filter_before_n_fmt", rec(nfs=0x80 << 24 | N_SAMPLE, filt=ints([-1], I8)), RUNTIME)

    # ---- sizes.  The minimum record's site block is 24 fixed bytes + 07 07 00; with fewer bytes
    # the missing ones read as 0xFF: CHROM negative up to 3 bytes, then the sample count wrong up to
    # 22, then (n_fmt -1, checked last) the ID / allele / FILTER descriptor missing
    full = cc.bcf_min_record(50)
    for ls in range(0, 28):
        r = struct.pack("<ii", ls, 0) + full[8:8 + ls]
        add("l_shared_%d" % ls, r, RUNTIME if ls < 4 else TRIBBLE if ls < 27 else OK)
    exact = rec(info=((br.typed_int(br.DICT["AF"]), br.typed_str("hello")),))
    add("value_ends_at_l_shared", exact, OK)
    r = bytearray(exact)
    struct.pack_into("<ii", r, 0, len(exact) - 9, 1)
    add("value_ends_1_past_l_shared", bytes(r), TRIBBLE)
    add("int32_value_ends_3_past_l_shared", rec(info=((br.typed_int(2), ints([7], I32)),), l_shared=24 + 4 + 5 + 2 + 2 + 2,
                                               l_indiv=3), TRIBBLE)
    add("l_shared_negative", struct.pack("<ii", -1, 0), TRIBBLE)
    add("l_indiv_negative", rec(l_indiv=-1), TRIBBLE)
    add("l_indiv_min_int", rec(l_indiv=-(1 << 31)), TRIBBLE)
    add("l_indiv_to_stream_end", rec(l_indiv=len(TAIL_BYTES)), OK)            # swallows the tail: n = K + 1
    add("l_indiv_1_past_stream", rec(l_indiv=len(TAIL_BYTES) + 1), TRIBBLE)
    add("l_shared_1_past_stream", rec(l_shared=len(rec()) - 8 + len(TAIL_BYTES) + 1), TRIBBLE)
    return c


CASES = _cases()
LABELS = [c[0] for c in CASES]
assert len(set(LABELS)) == len(LABELS)


def expected(label, status):
    """(n, status) a reader must report for the case's stream"""
    if status != OK:
        return K, status
    return (K + 1 if label == "l_indiv_to_stream_end" else K + 1 + TAIL), OK
