"""FASTQ / QSEQ without a device: the tests' restatement (tests/seqfrag_ref.py) reproduces every value
the reference's TestFastqInputFormat and TestQseqInputFormat assert (tests/golden/seqfrag/expected.json),
the ABI names and the exception mapping are in place, and the generated inputs of the device tests
hold nothing the device path would answer HBAM_EUNSUPPORTED."""
import gzip
import json
import os
import re

import pytest

import seqfrag_ref as ref
from conftest import GOLDEN, ROOT

SEQ = os.path.join(GOLDEN, "seqfrag")
EXPECTED = json.load(open(os.path.join(SEQ, "expected.json")))
CASES = [("fastq", c) for c in EXPECTED["fastq"]] + [("qseq", c) for c in EXPECTED["qseq"]]


def run_case(fmt, case):
    """The restatement over one expected.json entry -> (result or None when the constructor raises,
    the raised class name, the reader's end)."""
    data = open(os.path.join(SEQ, case["file"]), "rb").read()
    illumina, flt = ref.parse_conf(case.get("conf", {}), fmt)
    gz = case.get("gz", False)
    if gz:  # the round trip the reference's test makes through GzipCodec
        data = gzip.decompress(gzip.compress(data))
    run = ref.run_fastq if fmt == "fastq" else ref.run_qseq
    try:
        res = run(data, case["start"], case["length"], illumina, flt, compressed=gz)
    except ref.RuntimeException:
        return None, "RuntimeException", None
    return res, None, ref.LONG_MAX if gz else case["start"] + case["length"]


@pytest.mark.parametrize("fmt,case", CASES, ids=["%s-%s" % (f, c["test"]) for f, c in CASES])
def test_restatement_reproduces_reference_assertions(fmt, case):
    res, raised, end = run_case(fmt, case)
    if res is None:
        assert "records" not in case and case["raises"] == raised
        return
    ref.assert_case(case, res, end)


def test_expected_covers_the_reference_tests():
    want_fastq = {"testReadFromStart", "testReadStartInMiddle", "testSliceEndsBeforeEndOfFile",
                  "testGetReadNumFromName", "testNameWithoutReadNum", "testIlluminaMetaInfo",
                  "testIlluminaMetaInfoNullFC", "testIlluminaMetaInfoNegativeXYpos", "testOneIlluminaThenNot",
                  "testOneNotThenIllumina", "testProgress", "testReadFastqWithIdTwice",
                  "testReadFastqWithAmpersandQuality", "testFastqWithIlluminaEncoding",
                  "testFastqWithIlluminaEncodingAndGenericInputConfig", "testGzCompressedInput",
                  "testCompressedSplit", "testIlluminaNoIndex", "testSkipFailedQC", "testSkipFailedQCGenericConfig"}
    want_qseq = {"testReadFromStart", "testReadStartInMiddle", "testSliceEndsBeforeEndOfFile", "testIlluminaMetaInfo",
                 "testNs", "testConvertDotInIndexSequence", "testSangerQualities", "testConfigureForSangerQualities",
                 "testGenericInputConfigureForSangerQualities", "testProgress", "testGzCompressedInput",
                 "testCompressedSplit", "testSkipFailedQC", "testSkipFailedQCGenericConfig"}
    assert {c["test"] for c in EXPECTED["fastq"]} == want_fastq
    assert {c["test"] for c in EXPECTED["qseq"]} == want_qseq


def test_line_reader_terminators_and_hint():
    """readLine's three terminators, the CR that ends a buffer, and the hint that only acts there."""
    data = b"ab\rcd\r\nef\n\r\rgh"
    lr, t, got = ref.LineReader(ref.Stream(data)), ref.Text(), []
    while True:
        n = lr.readLine(t)
        if n == 0:
            break
        got.append((bytes(t.b), n))
    assert got == [(b"ab", 3), (b"cd", 4), (b"ef", 3), (b"", 1), (b"", 1), (b"gh", 2)]
    for buf in (1, 2, 3, 5):  # every boundary placement, CR last in a buffer included
        lr, out = ref.LineReader(ref.Stream(data), buf), []
        while True:
            n = lr.readLine(t)
            if n == 0:
                break
            out.append((bytes(t.b), n))
        assert out == got, buf
    # the hint ends a call only at a buffer boundary: "abcdef\n" in 4-byte buffers with hint 2
    lr = ref.LineReader(ref.Stream(b"abcdef\nxy"), 4)
    assert lr.readLine(t, ref.INT_MAX, 2) == 4 and bytes(t.b) == b"abcd"
    # maxLineLength drops what it does not store but counts it
    lr = ref.LineReader(ref.Stream(b"abcdef\nxy"))
    assert lr.readLine(t, 3) == 7 and bytes(t.b) == b"abc"
    assert lr.skip(1) == 1 and lr.readLine(t) == 1 and bytes(t.b) == b"y" and lr.skip(1) == 0


def test_positioning_walk_exits():
    """positionAtFirstRecord: a hit, the exit at an '@' line without a line + 2, the end of the file,
    and no '@' seen from the split's end on."""
    rec = b"@r1\nACGT\n+\n@@@@\n@r2\nAC\n+\n!!\n"
    assert ref.run_fastq(rec, 1, len(rec))["first_pos"] == 16  # "@@@@" fails (line + 2 is "AC"), "@r2" hits
    tail = b"xx\n@a\nlast"
    assert ref.run_fastq(tail, 1, 100)["first_pos"] == 6  # '@a' has no line + 2: the reader stands at "last"
    assert ref.run_fastq(tail, 1, 100)["status"] == ref.ERUNTIME
    assert ref.run_fastq(b"xx\nyy\n", 1, 100)["first_pos"] == 6
    r = ref.run_fastq(rec, 1, 2)  # end = 3: the '@' lines at 11 and 16 are not seen
    assert r["first_pos"] == len(rec) and r["n"] == 0


def test_abi_names_present():
    from hadoop_bam import _lib
    header = open(os.path.join(ROOT, "include", "hbam.h")).read()
    for name in ("hbam_fastq_decode_split", "hbam_qseq_decode_split", "hbam_frag_columns_to_host",
                 "hbam_frag_release"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b%s\(" % name, header)
    assert re.search(r"#define HBAM_ESEQFORMAT \(-18\)", header) and _lib.HBAM_ESEQFORMAT == -18
    assert re.search(r"#define HBAM_ENUMBER \(-19\)", header) and _lib.HBAM_ENUMBER == -19
    assert ref.ESEQFORMAT == _lib.HBAM_ESEQFORMAT and ref.ENUMBER == _lib.HBAM_ENUMBER
    assert ref.ERUNTIME == _lib.HBAM_ERUNTIME and ref.EUNSUPPORTED == _lib.HBAM_EUNSUPPORTED


def test_raise_for_maps_the_new_codes():
    from hadoop_bam import _lib, fastq, formats
    with pytest.raises(fastq.FormatException):
        formats.raise_for(_lib.HBAM_ESEQFORMAT, "x")
    with pytest.raises(fastq.NumberFormatException):
        formats.raise_for(_lib.HBAM_ENUMBER, "x")
    assert issubclass(fastq.FormatException, RuntimeError)  # FormatException extends RuntimeException
    assert issubclass(fastq.NumberFormatException, formats.IllegalArgumentException)


def test_host_classes():
    from hadoop_bam import fastq
    F, E = fastq.SequencedFragment, fastq.FormatConstants.BaseQualityEncoding
    assert F.verifyQuality(b"#~", E.Sanger) == -1 and F.verifyQuality(b"# ", E.Sanger) == 1
    assert F.verifyQuality(b"@\x80", E.Illumina) == 1 and F.verifyQuality(b"?", E.Illumina) == 0
    q = bytearray(b"bbb")
    F.convertQuality(q, E.Illumina, E.Sanger)
    assert q == b"CCC"
    with pytest.raises(fastq.FormatException):
        F.convertQuality(bytearray(b"#"), E.Illumina, E.Sanger)
    with pytest.raises(ValueError):
        F.convertQuality(q, E.Sanger, E.Sanger)
    a, b = F(), F()
    assert a.equals(b) and not a.equals(None)
    b.setLane(3)
    assert not a.equals(b) and b.getLane() == 3
    fmt = fastq.FastqInputFormat()
    assert fmt.isSplitable(None, "x.fastq") and not fmt.isSplitable(None, "x.fastq.gz")
    with pytest.raises(NotImplementedError):
        fmt.isSplitable(None, "x.fastq.bz2")
    with pytest.raises(fastq.RuntimeException):  # setConf runs before anything is read
        fastq.FastqRecordReader({"hbam.input.base-quality-encoding": "solexa"}, fastq.FileSplit("x.fastq", 0, 1))
    assert fastq.FormatConstants.CONF_INPUT_FILTER_FAILED_QC == "hbam.input.filter-failed-qc"
    assert fastq.QseqInputFormat.CONF_BASE_QUALITY_ENCODING == "hbam.qseq-input.base-quality-encoding"


@pytest.mark.parametrize("fmt", ["fastq", "qseq"])
def test_generated_inputs_hold_nothing_unsupported(fmt):
    """The generated files of the device tests: about 24 KiB, six 4 KiB tiles, all three terminators, a
    line above 10000 bytes, and no split of any tested size that the restatement refuses."""
    data = ref.generate_fastq() if fmt == "fastq" else ref.generate_qseq()
    run = ref.run_fastq if fmt == "fastq" else ref.run_qseq
    assert 20 * 1024 < len(data) <= 24 * 1024 + 4096
    assert all(data.count(t) > 10 for t in (b"\r\n", b"\n", b"\r"))
    whole = run(data, 0, len(data))
    assert whole["status"] == ref.OK and whole["n"] > 40
    if fmt == "fastq":
        assert max(len(r["seq"]) for r in whole["records"]) == 10000  # 10001 stored as 10000
        assert any(r["instrument"] is None for r in whole["records"]) and whole["records"][0]["instrument"]
    unsupported = 0
    for size in (61, 257, 4099):
        for flt in (False, True):
            union = []
            for s, n in ref.file_splits(len(data), size):
                r = run(data, s, n, filter_qc=flt)
                unsupported += r["status"] == ref.EUNSUPPORTED
                assert r["status"] == ref.OK
                union += [(x["rec_off"], x["key"], x["seq"], x["qual"]) for x in r["records"]]
            if not flt:
                assert union == [(x["rec_off"], x["key"], x["seq"], x["qual"]) for x in whole["records"]]
    assert unsupported == 0
