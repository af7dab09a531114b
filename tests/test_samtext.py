"""SAM text output, CPU side: the device's per-record rules (csrc/sam_text.h) run by a sanitizer-built
host program against the tests' restatement (tests/samtext_ref.py), the product's host renderer
and Float.toString against the same restatement, the round trip through the input side's
restatement, and the output format classes, the SAM preparer and the SAM merge with a stub in place
of the device call."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import f4_records
import sam_cases
import sam_ref
import samtext_cases as cases
import samtext_ref as ref
from conftest import GOLDEN, ROOT

GOLDEN_BAMS = ["small_pe.bam", "edge_uniform_long.bam", "edge_unsorted_l1.bam"]
FLOATS = [1, -3, 0, -0.0, 9999999, 1e7, 0.5, 0.1, 1e-3, 9.999e-4, 1.6777216e7, 3.4028235e38, 1.4e-45,
          float("nan"), float("inf"), float("-inf")]
FLOAT_TEXT = ["1.0", "-3.0", "0.0", "-0.0", "9999999.0", "1.0E7", "0.5", "0.1", "0.001", "9.999E-4", "1.6777216E7",
              "3.4028235E38", "1.4E-45", "NaN", "Infinity", "-Infinity"]


def test_import_exports_the_sam_output_classes():
    import hadoop_bam
    for name in ("SAMRecordWriter", "KeyIgnoringSAMRecordWriter", "AnySAMOutputFormat",
                 "KeyIgnoringAnySAMOutputFormat", "render_record", "java_float_to_string", "view"):
        assert getattr(hadoop_bam, name)
    assert "hbam_sam_render" in hadoop_bam._lib.EXPORTS


def test_device_record_rules_on_the_cpu_match_the_restatement(tmp_path):
    """csrc/sam_text.h is host-and-device C++: tools/sam_text_host.cpp, a stand-alone program built
    here with the address and undefined-behaviour sanitizers, runs every record through the rules
    the kernels run (both passes, SEQ \\t QUAL unit by unit on the output's 16-byte grid) over
    records held in a heap block of exactly their bytes + 64: every status, every line length,
    every byte and every deferral must be the restatement's.  A golden BAM, the crafted records,
    the float and H records, the edge records and every status case, each of those also as the
    last record of the block (nothing but the slack behind it)."""
    exe = str(tmp_path / "sam_text_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hadoop-bam_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tools", "sam_text_host.cpp")], check=True)
    h, golden = sam_cases.bam_header_and_records(np.fromfile(os.path.join(GOLDEN, "edge_unsorted_l1.bam"), np.uint8))
    bad = [c[2] for c in cases.status_cases()]
    sets = {
        "golden": (golden, [n for n, _ in h.refs]),
        "crafted": (cases.crafted_records() + [r for r, _ in cases.float_records()] + cases.edge_records(40) + bad,
                    cases.NAMES),
        "no_refs": ([f4_records.record(b"u", flag=4, ref=-1, pos=-1, cigar=(), l_seq=3)], []),
    }
    for k, slot in enumerate(bad):  # each failing record with nothing but the slack behind it
        sets["last_%d" % k] = ([cases.good_record(1), slot], cases.NAMES)
    for name, (slots, names) in sets.items():
        src, out = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(src, "wb") as f:
            f.write(cases.host_input(slots, names))
        subprocess.run([exe, src, out], check=True)
        got, p = open(out, "rb").read(), 0
        assert len(slots) > 0
        for k, slot in enumerate(slots):
            st, dfr, ln = struct.unpack_from("<iII", got, p)
            text = got[p + 12:p + 12 + ln]
            p += 12 + ln
            want = ref.status(slot, len(names))
            assert st == want, (name, k, st, want)
            if want != ref.HBAM_OK:
                assert ln == 0 and dfr == 0, (name, k)
                continue
            assert dfr == int(ref.deferred(slot)), (name, k)
            if dfr:
                assert ln == 0, (name, k)
            else:
                wl = ref.line(slot, names)
                assert ln == len(wl), (name, k, ln, len(wl))
                assert text == wl, (name, k, text[:120], wl[:120])
        assert p == len(got)
    assert [ref.status(s, cases.N_REF) for s in bad] == [c[1] for c in cases.status_cases()]
    assert [ref.deferred(r) for r, _ in cases.float_records()] == [d for _, d in cases.float_records()]


def test_restatement_stops_at_the_first_of_two_failing_records():
    """The streams of test_samtext_gpu.test_stops_among_deferred_records: the restatement ends at the
    first failing record in output order, whichever rule finds it, and lists the deferred records
    before it."""
    for name, slots, n, status, deferred in cases.stop_streams():
        want = ref.render(slots, cases.NAMES)
        assert (want["n"], want["status"], want["deferred"]) == (n, status, deferred), name
        assert len(want["text"]) == int(want["line_off"][n]) and len(want["line_off"]) == n + 1, name
        assert all(want["lines"][k] == b"" for k in deferred) and want["lines"][0] != b"", name


def test_java_float_to_string_matches_the_restatement():
    from hadoop_bam import java_float_to_string
    for v, text in zip(FLOATS, FLOAT_TEXT):
        bits = ref.bits_of(v)
        assert java_float_to_string(bits) == ref.java_float(bits) == text, v
    assert java_float_to_string(7) == ref.java_float(7) == "9.8E-45"  # one digit would be the next power's 1
    rng = np.random.default_rng(5)
    some = list(rng.integers(0, 1 << 32, 3000, dtype=np.uint64)) + list(range(1, 40)) + \
        [ref.bits_of(x) for x in cases.DEVICE_FLOATS + cases.HOST_FLOATS + [1e10, 123456.79, 1e-5, 8.5e-4, 100.0]]
    # every power of two, where the rounding interval is lopsided (a quarter of a step below, half a
    # step above) and the nearest decimal of a length may lie outside it while the next one is inside;
    # their neighbours and negatives too
    pow2 = [ex << 23 for ex in range(1, 255)]
    some += pow2 + [b + 1 for b in pow2] + [b - 1 for b in pow2] + [b | 0x80000000 for b in pow2]
    for bits in some:
        assert java_float_to_string(int(bits)) == ref.java_float(int(bits)), hex(int(bits))
    assert java_float_to_string(0x0f800000) == "1.2621775E-29" and java_float_to_string(0x6b000000) == "1.5474251E26"
    assert java_float_to_string(0xec800000) == "-1.2379401E27"


def test_render_record_matches_the_restatement():
    from hadoop_bam import render_record
    from hadoop_bam.formats import IllegalArgumentException, SAMFormatException
    recs = cases.crafted_records() + [r for r, _ in cases.float_records()] + cases.edge_records(20)
    for r in recs:
        assert render_record(r, cases.NAMES) == ref.line(r, cases.NAMES)
    h, golden = sam_cases.bam_header_and_records(np.fromfile(os.path.join(GOLDEN, "small_pe.bam"), np.uint8))
    names = [n for n, _ in h.refs]
    for r in golden[:300]:
        assert render_record(r, names) == ref.line(r, names)
    for name, status, slot in cases.status_cases():
        bs = struct.unpack_from("<i", slot, 0)[0]
        with pytest.raises(SAMFormatException if status == ref.HBAM_EFORMAT else IllegalArgumentException):
            render_record(slot if name.startswith("block_size") else slot[:4 + bs], cases.NAMES)


def test_rendered_lines_parse_back_to_their_records():
    """sam_ref.parse_encode of the line the product's host renderer writes returns the record's bytes
    for 94 of the 95 crafted records; the 95th carries 1.0E29, outside the input side's float
    domain."""
    from hadoop_bam import render_record
    recs = cases.crafted_records()
    assert len(recs) == 95
    out = []
    for r in recs:
        back = sam_ref.parse_encode(render_record(r, cases.NAMES)[:-1], sam_cases.DICT)
        if back != r:
            out.append((sam_ref.fields(r)["name"], back))
    assert out == [(b"tags", sam_ref.HBAM_EUNSUPPORTED)]
    assert b":1.0E29" in render_record(recs[[sam_ref.fields(r)["name"] for r in recs].index(b"tags")], cases.NAMES)
    assert sum(ref.deferred(r) for r in recs) == 1
    for name in GOLDEN_BAMS:  # only i and Z tags: nothing for the host
        h, golden = sam_cases.bam_header_and_records(np.fromfile(os.path.join(GOLDEN, name), np.uint8))
        assert not any(ref.deferred(r) for r in golden[:2000])


class StubContext:
    """Context.sam_render answered by the restatement."""

    def __init__(self):
        self.calls = 0

    def sam_render(self, ubuf, rec_off, n, names, perm=None, on_device=True):
        assert not on_device and perm is None
        self.calls += 1
        ro = [int(x) for x in rec_off]
        r = ref.render([bytes(ubuf[ro[k]:ro[k + 1]]) for k in range(n)], names)
        return {"rc": 0, "n": r["n"], "status": r["status"], "err_record": r["n"] if r["status"] else 0,
                "text": r["text"], "line_off": r["line_off"], "deferred": np.array(r["deferred"], np.uint32)}


def _header():
    from hadoop_bam import SAMFileHeader
    return SAMFileHeader(b"@HD\tVN:1.4\tSO:unsorted", sam_cases.REFS)


def test_sam_record_writer_with_a_stub_device():
    """The header text (a final newline added, @SQ lines from the dictionary when the text has none,
    as sam_ref.header_text), then every line, the deferred ones rendered on the host and spliced in
    at their places; a failing record raises after the lines before it are written."""
    from hadoop_bam import SAMRecordWriter, SAMRecordWritable
    from hadoop_bam.formats import BAMRecordBytes, IllegalArgumentException
    recs = [r for r, _ in cases.float_records()] + cases.crafted_records()[:30]
    want_header = b"".join(ln + b"\n" for ln in sam_ref.header_text(_header().text, sam_cases.REFS))
    want = b"".join(ref.line(r, cases.NAMES) for r in recs)
    out, ctx = io.BytesIO(), StubContext()
    w = SAMRecordWriter(out, _header(), True, ctx)
    w.write_encoded(b"".join(recs[:10]))
    for r in recs[10:20]:
        w.writeAlignment(BAMRecordBytes(r))
    for r in recs[20:]:
        v = SAMRecordWritable()
        v.set(BAMRecordBytes(r))
        w.write(None, v)
    w.close()
    assert out.getvalue() == want_header + want and ctx.calls == 1
    assert want_header.count(b"@SQ") == 4 and want_header.endswith(b"LN:4262\n")
    out = io.BytesIO()
    w = SAMRecordWriter(out, _header(), False, StubContext())
    w.write_encoded(b"".join(recs[:5]) + cases.status_cases()[-7][2] + recs[5])
    with pytest.raises(IllegalArgumentException):
        w.close()
    assert out.getvalue() == b"".join(ref.line(r, cases.NAMES) for r in recs[:5])
    from hadoop_bam import SAMFileHeader
    out = io.BytesIO()  # a text that has its @SQ lines and its final newline stays as it is
    text = b"".join(ln + b"\n" for ln in sam_cases.HEADER)
    SAMRecordWriter(out, SAMFileHeader(text, sam_cases.REFS), True, StubContext()).close()
    assert out.getvalue() == text


def test_any_sam_output_format_properties_and_exceptions(tmp_path):
    from hadoop_bam import (AnySAMOutputFormat, Configuration, KeyIgnoringAnySAMOutputFormat,
                            KeyIgnoringBAMRecordWriter, KeyIgnoringSAMRecordWriter)
    from hadoop_bam.formats import IllegalArgumentException, IOException
    P, W = "hadoopbam.anysam.output-format", "hadoopbam.anysam.write-header"
    assert AnySAMOutputFormat.OUTPUT_SAM_FORMAT_PROPERTY == P and KeyIgnoringAnySAMOutputFormat.WRITE_HEADER_PROPERTY == W
    assert AnySAMOutputFormat(Configuration()).format is None
    assert AnySAMOutputFormat(Configuration({P: "SAM"})).format == "SAM"
    assert AnySAMOutputFormat("BAM").format == "BAM"
    with pytest.raises(IllegalArgumentException, match="null SAMFormat"):
        AnySAMOutputFormat(None)
    with pytest.raises(IllegalArgumentException):  # SAMFormat.valueOf
        AnySAMOutputFormat(Configuration({P: "sam"}))
    with pytest.raises(IllegalArgumentException, match="OUTPUT_SAM_FORMAT_PROPERTY not set"):
        KeyIgnoringAnySAMOutputFormat(Configuration())
    with pytest.raises(IllegalArgumentException, match="unknown SAM format: .*out.txt"):
        KeyIgnoringAnySAMOutputFormat(Configuration(), "/x/out.txt")
    assert KeyIgnoringAnySAMOutputFormat(Configuration(), "/x/out.sam").format == "SAM"
    assert KeyIgnoringAnySAMOutputFormat(Configuration({P: "BAM"}), "/x/out.sam").format == "BAM"
    f = KeyIgnoringAnySAMOutputFormat("SAM")
    with pytest.raises(IOException, match="without the SAM header"):
        f.getRecordWriter(io.BytesIO(), ctx=StubContext())
    f.setSAMHeader(_header())
    assert f.getSAMHeader() is not None and f.getWriteHeader() is True
    out = io.BytesIO()
    w = f.getRecordWriter(out, ctx=StubContext())
    assert isinstance(w, KeyIgnoringSAMRecordWriter)
    w.close()
    assert out.getvalue().startswith(b"@HD")
    for conf, deprecated, expect in (({W: "false"}, True, False), ({W: "true"}, False, True), ({}, False, False)):
        g = KeyIgnoringAnySAMOutputFormat(Configuration(dict(conf, **{P: "SAM"})))
        g.setSAMHeader(_header())
        g.setWriteHeader(deprecated)
        out = io.BytesIO()
        g.getRecordWriter(out, ctx=StubContext()).close()
        assert bool(out.getvalue()) == expect
    b = KeyIgnoringAnySAMOutputFormat(Configuration({P: "BAM", W: "false"}))
    b.setSAMHeader(_header())
    assert isinstance(b.getRecordWriter(io.BytesIO(), ctx=StubContext()), KeyIgnoringBAMRecordWriter)
    sam = tmp_path / "h.sam"
    sam.write_bytes(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()[:3]))
    f.readSAMHeaderFrom(str(sam), ctx=StubContext())
    assert f.getSAMHeader().refs == sam_cases.REFS


def test_sam_preparer_and_sam_merge(tmp_path):
    """prepareForRecords(out, "SAM", header) writes the header text and returns out;
    merge_sam_into(fmt="SAM") writes it, then the parts in name order, no terminator, and removes
    the parts."""
    from hadoop_bam import SAMOutputPreparer, merge_sam_into
    from hadoop_bam.output import get_mergeable_work_file
    want_header = b"".join(ln + b"\n" for ln in sam_ref.header_text(_header().text, sam_cases.REFS))
    out = io.BytesIO()
    assert SAMOutputPreparer().prepareForRecords(out, "SAM", _header()) is out
    assert out.getvalue() == want_header
    with pytest.raises(ValueError):
        SAMOutputPreparer().prepareForRecords(io.BytesIO(), "CRAM", _header())
    lines = [ref.line(r, cases.NAMES) for r in cases.crafted_records()[:9]]
    d = tmp_path / "work"
    d.mkdir()
    for task in (2, 0, 1):
        with open(get_mergeable_work_file(str(d), "", "", "part", task), "wb") as f:
            f.write(b"".join(lines[3 * task:3 * task + 3]))
    merged = str(tmp_path / "merged.sam")
    merge_sam_into(merged, str(d), "", "", _header(), "part", fmt="SAM")
    assert open(merged, "rb").read() == want_header + b"".join(lines)
    assert os.listdir(str(d)) == []
