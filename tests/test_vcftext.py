"""VCF text output, the host side: the rule restatement (tests/vcftext_ref.py) pinned on the
reference's own expectations, hadoop_bam.vcf_text.render_record against it on every crafted record,
the status cases, and the output format classes.  No GPU."""
import io

import pytest

import bcf_records
import vcftext_cases as C
import vcftext_ref as R
from hadoop_bam import vcf_text as V
from hadoop_bam.formats import Configuration, IllegalArgumentException, IOException
from hadoop_bam.vcf import VCFFormat


def host(e):
    return V.VCFHeader(e.text.encode())


def host_result(rec, H):
    """(status, line, deferred) as vcftext_ref.render returns it, from render_record"""
    try:
        return R.OK, V.render_record(rec, H), V.should_defer(rec, H)
    except V.TribbleException:
        return R.ETRIBBLE, None, False
    except V.BCFDecodeRuntimeException:
        return R.ERUNTIME, None, False
    except V.VCFUnsupportedException:
        return R.EUNSUPPORTED, None, False


# ---- 1. the restatement on the reference's own expectations ------------------------------------------
def test_simple_matches_TestVCFOutputFormat():
    e, rec, expected = C.simple_case()
    assert R.render(rec, e.hdr) == (R.OK, expected, False)
    assert V.render_record(rec, host(e)) == expected


def test_golden_vcf_records():
    e, recs = C.golden_records()
    got = R.render_stream(recs, e.hdr)
    assert got["status"] == R.OK and got["deferred"] == []
    assert got["text"] == C.GOLDEN_EXPECTED
    H = host(e)
    assert b"".join(V.render_record(r, H) for r in recs) == C.GOLDEN_EXPECTED


def test_header_dictionary_order():
    e, _ = C.golden_records()
    H = host(e)
    want = ["PASS", "NS", "DP", "AF", "AA", "DB", "H2", "q10", "s50", "GT", "GQ", "HQ"]
    assert e.hdr["dict"] == want and [x.decode() for x in H.dictionary] == want
    assert [x.decode() for x in H.samples] == ["NA00001", "NA00002", "NA00003"] == e.hdr["samples"]
    assert H.contigs == [b"20"] and H.rank == e.hdr["rank"]
    m = H.meta()
    assert m["dict_flags"][want.index("DB")] == 3 and m["dict_flags"][want.index("GT")] == 4 | 1 << 4
    assert m["dict_flags"][want.index("DP")] == 1 | 4 | 2 << 4 and m["dict_number"][want.index("HQ")] == 2


# ---- 2. render_record equals the restatement -----------------------------------------------------------
CRAFT_ENC, CRAFTED = C.crafted()


@pytest.mark.parametrize("name", [n for n, _ in CRAFTED])
def test_render_record_on_crafted(name):
    rec = dict(CRAFTED)[name]
    ref = R.render(rec, CRAFT_ENC.hdr)
    assert ref[0] == R.OK, "every crafted record renders"
    assert host_result(rec, host(CRAFT_ENC)) == ref


def test_crafted_texts():
    """the rules' own examples, literally"""
    got = {n: R.render(r, CRAFT_ENC.hdr) for n, r in CRAFTED}
    col = lambda n, i: got[n][1].rstrip(b"\n").split(b"\t")[i]  # noqa: E731
    assert col("qual_0", 5) == b"0" and col("qual_29_6", 5) == b"29.60" and col("qual_missing", 5) == b"."
    assert col("qual_tie", 5) == b"0.13" and col("qual_1e7", 5) == b"10000000"
    want = [b"0.00", b"1.000e-02", b"1.000e-02", b"0.063", b"1.000", b"1.00", b"2.13", b"0.00",
            b"-1.000e+00", b"NaN"]
    assert [col("float_%d" % i, 7) for i in range(10)] == [b"FV=" + w for w in want]
    assert col("comma_list", 7) == b"ST=a,b,c" and col("nul_tail", 7) == b"ST=ab" and col("nul_tail", 2) == b"id"
    assert col("miss_front", 7) == b"IV=2,3" and col("miss_middle", 7) == b"IV=1,3" and col("miss_all", 7) == b"IV=."
    assert col("filter_three", 6) == b"aa1;q10;zz9" and col("filter_dup", 6) == b"PASS;s50"
    assert col("ploidy3", 10) == b"0|1" and col("gt_absent_dp", 8) == b"DP" and col("all_stripped", 10) == b""
    assert col("generic_null", 10) == b"0/0:2:.,.:.,.:.,.,.:8" and col("generic_null", 11) == b"1/1:.:.,.:.,.:.,.,.:9"
    assert col("allele_lower", 3) == b"ACGTN" and col("allele_lower", 4) == b"<del>,a[c1:5[,.A,g.,]c1:9]t"
    deferred = sorted(n for n in got if got[n][2])
    assert deferred == sorted(
        ["info_twice", "qual_tie", "qual_1e7", "qual_neg0", "float_1", "float_2", "float_7", "float_8", "float_9",
         "float_13", "float_14", "fmt_float", "fmt_char", "fmt_ft", "fmt_g_null", "ploidy17", "filter_65", "info_65"])


def test_many_fields_is_deferred():
    e, rec = C.crafted_many_fields()
    ref = R.render(rec, e.hdr)
    assert ref[0] == R.OK and ref[2] is True
    assert host_result(rec, host(e)) == ref


@pytest.mark.parametrize("ns", [0, 1, 3, 63, 64, 65, 130])
def test_sample_records(ns):
    e, recs = C.sample_records(ns)
    H = host(e)
    for r in recs:
        ref = R.render(r, e.hdr)
        assert ref[0] == R.OK and ref[2] is False
        assert host_result(r, H) == ref


# ---- 3. status cases ---------------------------------------------------------------------------------------
STATUS_ENC, STATUS = C.status_cases()


@pytest.mark.parametrize("name", [n for n, _, _ in STATUS])
def test_status_case(name):
    rec, status = [(r, s) for n, r, s in STATUS if n == name][0]
    assert R.render(rec, STATUS_ENC.hdr) == (status, None, False)
    assert host_result(rec, host(STATUS_ENC)) == (status, None, False)


# ---- 4. output format classes --------------------------------------------------------------------------------
def test_restatement_stops_at_the_first_of_two_failing_records():
    """the streams of test_vcftext_gpu.test_stop_among_deferred_records: the first failing record ends the
    output, the deferred records before it are listed, and the record behind it fails on its own"""
    for name, e, recs, n, status, deferred in C.stop_streams():
        got = R.render_stream(recs, e.hdr)
        assert (got["n"], got["status"], got["deferred"]) == (n, status, deferred), name
        assert len(got["text"]) == got["line_off"][n] and len(got["line_off"]) == n + 1, name
        assert R.render(recs[90], e.hdr)[0] not in (R.OK, status) and R.render(recs[100], e.hdr)[2] is True, name


def test_output_format_constructors():
    assert V.OUTPUT_VCF_FORMAT_PROPERTY == "hadoopbam.vcf.output-format"
    assert V.WRITE_HEADER_PROPERTY == "hadoopbam.vcf.write-header"
    assert V.KeyIgnoringVCFOutputFormat(VCFFormat.VCF).format == VCFFormat.VCF
    with pytest.raises(IllegalArgumentException):
        V.KeyIgnoringVCFOutputFormat(None)
    conf = Configuration()
    with pytest.raises(IllegalArgumentException):
        V.KeyIgnoringVCFOutputFormat(conf)
    assert V.KeyIgnoringVCFOutputFormat(conf, "out.vcf").format == VCFFormat.VCF
    assert V.KeyIgnoringVCFOutputFormat(conf, "out.bcf").format == VCFFormat.BCF
    with pytest.raises(IllegalArgumentException):
        V.KeyIgnoringVCFOutputFormat(conf, "out.txt")
    conf[V.OUTPUT_VCF_FORMAT_PROPERTY] = "BCF"
    assert V.KeyIgnoringVCFOutputFormat(conf, "out.vcf").format == VCFFormat.BCF
    assert V.VCFOutputFormat(conf).format == VCFFormat.BCF
    conf[V.OUTPUT_VCF_FORMAT_PROPERTY] = "vcf4"
    with pytest.raises(IllegalArgumentException):
        V.KeyIgnoringVCFOutputFormat(conf)


def test_record_writer_needs_the_header():
    f = V.KeyIgnoringVCFOutputFormat(VCFFormat.VCF)
    assert f.getHeader() is None
    with pytest.raises(IOException, match="Can't create a RecordWriter without the VCF header"):
        f.getRecordWriter(io.BytesIO())


def test_write_header_property_and_bcf_format():
    e, _ = C.golden_records()
    f = V.KeyIgnoringVCFOutputFormat(VCFFormat.VCF)
    f.setHeader(host(e))
    out = io.BytesIO()
    f.getRecordWriter(out).close()
    assert out.getvalue() == e.text.encode()  # the header text as it stands
    out = io.BytesIO()
    f.getRecordWriter(out, Configuration({V.WRITE_HEADER_PROPERTY: "false"})).close()
    assert out.getvalue() == b""
    g = V.KeyIgnoringVCFOutputFormat(VCFFormat.BCF)
    g.setHeader(host(e))
    with pytest.raises(NotImplementedError):
        g.getRecordWriter(io.BytesIO())


def test_text_record_is_not_written():
    from hadoop_bam.vcf import VCFRecord
    e, _ = C.golden_records()
    w = V.VCFRecordWriter(io.BytesIO(), host(e), False)
    with pytest.raises(NotImplementedError):
        w.write(0, VCFRecord.__new__(VCFRecord))


# ---- 5. the end-to-end input's deferred share, on the restatement alone -------------------------------------
def stream_share(**kw):
    text, recs = C.split_stream(bcf_records.bcf_stream(2000, **kw))
    got = R.render_stream(recs, C.Enc(text).hdr)
    return got, len(got["deferred"]) / 2000.0


def test_stream_deferred_share():
    """The end-to-end input's deferred share is above 0 and below 5 %, known before any GPU run.  The
    input is bcf_records.bcf_stream(2000, hom_ref=1.0): its AF values are uniform in [0, 1), so about
    1.5 % of its records hold one below 0.01.  The generator's default (hom_ref=0.0) cannot serve: it
    draws every GT allele from 1..3 (allele index 0..2) whatever the record's allele count, so 948 of
    its 2000 records name an allele the record does not have, which the rule list makes HBAM_ERUNTIME
    (`encoded >> 1` outside [0, n_allele]); test_default_stream_stops_at_its_first_bad_call pins that."""
    got, share = stream_share(hom_ref=1.0)
    print("deferred", len(got["deferred"]), "share", share)
    assert got["status"] == R.OK and got["n"] == 2000
    assert 0 < share < 0.05


def test_default_stream_stops_at_its_first_bad_call():
    got, share = stream_share()
    assert (got["status"], got["n"], got["deferred"]) == (R.ERUNTIME, 0, [])


# ---- 6. the device's record rules on the CPU -----------------------------------------------------------------
def test_device_record_rules_on_the_cpu_match_the_restatement(tmp_path):
    """csrc/vcf_text.h is host-and-device C++: tools/vcf_text_host.cpp, a stand-alone program built here
    with the address and undefined-behaviour sanitizers, runs every record through the rules the
    kernels run (both passes; the wave path with its lanes one after the other) over records held in
    a heap block of exactly their bytes + 64: every status, every line length, every byte and every
    deferral must be the restatement's.  The golden and crafted records, the sample counts around the
    path cut, and every status case, each of those also as the last record of the block (nothing but
    the slack behind it).  wave_cut 1 sends even three samples through the wave path, 2^32 - 1 keeps
    130 samples on the lane path."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(C.HERE)
    exe = str(tmp_path / "vcf_text_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "hadoop-bam_amd", "csrc"),
                    "-o", exe, os.path.join(root, "tools", "vcf_text_host.cpp")], check=True)
    ge, grecs = C.golden_records()
    me, mrec = C.crafted_many_fields()
    sets = [("golden", ge, grecs, 64), ("golden_wave", ge, grecs, 1), ("many", me, [mrec], 64), ("many_wave", me, [mrec], 1),
            ("crafted", CRAFT_ENC, [r for _, r in CRAFTED] + [r for _, r, _ in STATUS], 64),
            ("crafted_wave", CRAFT_ENC, [r for _, r in CRAFTED] + [r for _, r, _ in STATUS], 1)]
    for k, (_, r, _) in enumerate(STATUS):
        sets.append(("last_%d" % k, STATUS_ENC, [CRAFTED[0][1], r], 64))
        sets.append(("last_wave_%d" % k, STATUS_ENC, [CRAFTED[0][1], r], 1))
    for ns in (0, 1, 3, 63, 64, 65, 130):
        e, recs = C.sample_records(ns)
        sets.append(("samples_%d" % ns, e, recs, 64))
        sets.append(("samples_lane_%d" % ns, e, recs, 0xffffffff))
    for name, e, recs, cut in sets:
        src, out = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(src, "wb") as f:
            f.write(C.host_input(e, recs, cut))
        subprocess.run([exe, src, out], check=True)
        got, p = open(out, "rb").read(), 0
        for k, rec in enumerate(recs):
            st, dfr, ln = struct.unpack_from("<iII", got, p)
            text = got[p + 12:p + 12 + ln]
            p += 12 + ln
            # a record is judged inside the bytes from its offset to the end of the block, as on the device
            want = R.render(b"".join(recs[k:]), e.hdr)
            assert st == want[0], (name, k, st, want[0])
            if want[0] != R.OK:
                assert ln == 0 and dfr == 0, (name, k)
                continue
            assert dfr == int(want[2]), (name, k)
            assert text == (b"" if dfr else want[1]), (name, k, text[:160], want[1][:160])


def test_public_names():
    import hadoop_bam
    for name in ("VCFRecordWriter", "KeyIgnoringVCFRecordWriter", "VCFOutputFormat", "KeyIgnoringVCFOutputFormat",
                 "VCFHeader", "read_vcf_header_from"):
        assert getattr(hadoop_bam, name)
    assert {"hbam_vcf_render", "hbam_bcf_header_text"} <= set(hadoop_bam._lib.EXPORTS)
    for name in ("bcf_header_text", "bcf_decode_split_device", "vcf_render_device", "vcf_render"):
        assert hasattr(hadoop_bam.Context, name)
    assert (hadoop_bam._lib.HBAM_VCF_MAX_INFO, hadoop_bam._lib.HBAM_VCF_MAX_FORMAT) == (R.MAX_INFO, R.MAX_FORMAT)
