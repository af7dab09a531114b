"""FASTQ / QSEQ on the device (hbam_fastq.hip through hadoop_bam.fastq and Context.frag_decode_split)
against the tests' restatement (tests/seqfrag_ref.py) and the reference's own assertions
(tests/golden/seqfrag/expected.json).  The device is never compared with itself."""
import gzip
import json
import os

import pytest

import seqfrag_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEQ = os.path.join(GOLDEN, "seqfrag")
EXPECTED = json.load(open(os.path.join(SEQ, "expected.json")))
CASES = [("fastq", c) for c in EXPECTED["fastq"]] + [("qseq", c) for c in EXPECTED["qseq"]]
FILES = sorted(f for f in os.listdir(SEQ) if f.endswith((".fastq", ".qseq")))
EMORE = -12
INTS = ("run", "lane", "tile", "xpos", "ypos", "read", "control")
STRS = ("instrument", "flowcell", "index")


def fmt_of(name):
    return "fastq" if name.endswith(".fastq") else "qseq"


def ref_run(fmt, data, start, length, illumina=None, flt=False, compressed=False):
    illumina = (fmt == "qseq") if illumina is None else illumina
    return (ref.run_fastq if fmt == "fastq" else ref.run_qseq)(data, start, length, illumina, flt, compressed)


def as_result(fmt, cols, window):
    """Host columns of one device call -> the restatement's result form."""
    from hadoop_bam import _lib
    assert cols["rc"] == 0, cols
    P = _lib.FRAG_PRESENT
    out = {k: cols[k] for k in ("n", "status", "first_pos", "end_pos", "err_pos")}
    recs = []
    for i in range(cols["n"]):
        p = int(cols["present"][i])
        r = {"present": p, "rec_off": int(cols["rec_off"][i]), "pos_after": int(cols["pos_after"][i])}
        for k in ("key", "seq", "qual"):
            r[k] = cols[k][int(cols[k + "_off"][i]):int(cols[k + "_off"][i + 1])].tobytes()
        for k in INTS:
            r[k] = int(cols[k][i]) if p & P[k] else None
        r["filter_passed"] = bool(cols["filter_passed"][i]) if p & P["filter_passed"] else None
        for k in STRS:
            o, n = (int(x) for x in cols[k][i])
            r[k] = bytes(window[o:o + n]) if p & P[k] else None
        if fmt == "qseq" and r["index"] is not None:
            r["index"] = r["index"].replace(b".", b"N")  # the column is the raw field (include/hbam.h)
        recs.append(r)
    out["records"] = recs
    return out


def device_run(ctx, fmt, data, start, length, illumina=None, flt=False, window_end=None, device_window=False):
    """One device call over the window [the reader's first byte, window_end or the end of the file).
    device_window: the window is device memory that begins at the reader's first byte inside a
    256-aligned allocation, so an odd first byte is an unaligned window."""
    illumina = (fmt == "qseq") if illumina is None else illumina
    base = min(start if fmt == "fastq" else max(start - 1, 0), len(data))
    stop = len(data) if window_end is None else window_end
    window = bytes(data[base:stop])
    arg = window
    if device_window:
        import torch
        t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        arg = t[base:stop]
        assert arg.data_ptr() % 16 == base % 16
    cols = ctx.frag_decode_split(fmt, arg, start, length, int(illumina), flt, text_base=base, file_len=len(data))
    return as_result(fmt, cols, window)


def assert_same(dev, want, what):
    """Every column, the three pools, the positions and the status."""
    assert dev["status"] == want["status"], (what, dev["status"], want["status"])
    assert dev["n"] == want["n"], (what, dev["n"], want["n"])
    assert dev["first_pos"] == want["first_pos"], (what, dev["first_pos"], want["first_pos"])
    if want["status"] == ref.OK:
        assert dev["end_pos"] == want["end_pos"], (what, dev["end_pos"], want["end_pos"])
    elif want["err_pos"] is not None:
        assert dev["err_pos"] == want["err_pos"], (what, dev["err_pos"], want["err_pos"])
    for i, (d, w) in enumerate(zip(dev["records"], want["records"])):
        for k in ("rec_off", "pos_after", "present", "key", "seq", "qual", "filter_passed") + INTS + STRS:
            assert d[k] == w[k], (what, i, k, d[k], w[k])


def check_splits(ctx, fmt, data, size, illumina=None, flt=False, **kw):
    """Every split of `size` against the restatement -> (device union, unsupported answers)."""
    union, unsupported = [], 0
    for s, n in ref.file_splits(len(data), size):
        dev = device_run(ctx, fmt, data, s, n, illumina, flt, **kw)
        assert_same(dev, ref_run(fmt, data, s, n, illumina, flt), (fmt, size, s))
        unsupported += dev["status"] == ref.EUNSUPPORTED
        union += dev["records"]
    return union, unsupported


def body(r):
    return r["rec_off"], r["key"], r["seq"], r["qual"]


@pytest.mark.parametrize("fmt,case", CASES, ids=["%s-%s" % (f, c["test"]) for f, c in CASES])
def test_reference_assertions_through_the_public_classes(gpu_ctx, fmt, case, tmp_path):
    """Every value the reference's own tests assert, through FastqInputFormat / QseqInputFormat."""
    from hadoop_bam import fastq
    data = open(os.path.join(SEQ, case["file"]), "rb").read()
    path = str(tmp_path / (case["file"] + (".gz" if case.get("gz") else "")))
    with open(path, "wb") as f:
        f.write(gzip.compress(data) if case.get("gz") else data)
    split = fastq.FileSplit(path, case["start"], case["length"])
    informat = fastq.FastqInputFormat() if fmt == "fastq" else fastq.QseqInputFormat()
    exc = {"RuntimeException": fastq.RuntimeException, "FormatException": fastq.FormatException}
    if "raises" in case and "records" not in case:
        with pytest.raises(exc[case["raises"]]):
            informat.createRecordReader(split, dict(case.get("conf", {})))
        return
    reader = informat.createRecordReader(split, dict(case.get("conf", {})))
    assert reader.makePositionMessage() == "%s:%d" % (path, reader.getPos())
    res = {"first_pos": reader.getPos(), "records": [], "status": ref.OK}
    progress = [reader.getProgress()]
    try:
        while reader.nextKeyValue():
            v = reader.getCurrentValue()
            res["records"].append({
                "key": reader.getCurrentKey(), "seq": v.getSequence(), "qual": v.getQuality(),
                "pos_after": reader.getPos(), "instrument": v.getInstrument(), "run": v.getRunNumber(),
                "flowcell": v.getFlowcellId(), "lane": v.getLane(), "tile": v.getTile(), "xpos": v.getXpos(),
                "ypos": v.getYpos(), "read": v.getRead(), "filter_passed": v.getFilterPassed(),
                "control": v.getControlNumber(), "index": v.getIndexSequence()})
            progress.append(reader.getProgress())
    except fastq.FormatException:
        res["status"] = ref.ESEQFORMAT
    res["n"] = len(res["records"])
    ref.assert_case(case, res, reader.end)
    for want, got in zip(case.get("progress", []), progress):  # the reader's own float32 getProgress
        assert abs(got - want) <= 0.01
    reader.close()


@pytest.mark.parametrize("name", FILES)
def test_fixtures_whole_and_split(gpu_ctx, name):
    fmt = fmt_of(name)
    data = open(os.path.join(SEQ, name), "rb").read()
    # (sangerQseq under the QSEQ default raises FormatException in both: the status is compared)
    whole = device_run(gpu_ctx, fmt, data, 0, len(data))
    want = ref_run(fmt, data, 0, len(data))
    assert_same(whole, want, (name, "whole"))
    unsupported = whole["status"] == ref.EUNSUPPORTED
    for size in (10, 61, 97, 257):
        union, u = check_splits(gpu_ctx, fmt, data, size)
        unsupported += u
        if want["status"] == ref.OK:
            # the splits return every record once; the sticky Illumina flag makes only the metadata
            # depend on the split, and check_splits has compared that with the restatement
            assert [body(r) for r in union] == [body(r) for r in want["records"]], (name, size)
    assert unsupported == 0


@pytest.fixture(scope="module")
def generated():
    return {"fastq": ref.generate_fastq(), "qseq": ref.generate_qseq()}


@pytest.mark.parametrize("fmt", ["fastq", "qseq"])
@pytest.mark.parametrize("flt", [False, True], ids=["all", "filter-failed-qc"])
def test_generated_whole_and_split(gpu_ctx, generated, fmt, flt):
    """About 24 KiB (six 4 KiB tiles), all three terminators, a 10001-byte sequence."""
    data = generated[fmt]
    want = ref_run(fmt, data, 0, len(data), flt=flt)
    assert want["status"] == ref.OK and want["n"] > 20
    assert_same(device_run(gpu_ctx, fmt, data, 0, len(data), flt=flt), want, (fmt, "whole"))
    unsupported = 0
    for size in (61, 257, 4099):
        union, u = check_splits(gpu_ctx, fmt, data, size, flt=flt)
        unsupported += u
        if not flt:
            assert [body(r) for r in union] == [body(r) for r in want["records"]], size
    assert unsupported == 0


def crafted_fastq(t_at, term, tail=b"\n"):
    """Three records; the first key line's terminator `term` begins at file offset t_at."""
    key = b"@" + b"k" * (t_at - 1)
    rest = (b"ACGT" + b"\r\n" + b"+" + b"\r" + b"IIII" + b"\n" + b"@M1:2:FC:3:4:5:6 1:N:0:AC" + b"\r" + b"GG" + b"\n+\r\n"
            + b"#5" + b"\r" + b"@r3/2\nTTT\n+\n!!!" + tail)
    return key + term + rest


BOUNDARIES = (15, 1023, 4095)
PLACEMENTS = [(p - len(t) + 1, t) for p in BOUNDARIES for t in (b"\r", b"\r\n", b"\n")]  # last byte at p
PLACEMENTS += [(p, b"\r\n") for p in BOUNDARIES]  # CR at p, LF at p + 1
PLACEMENTS += [(p + 1, t) for p in BOUNDARIES for t in (b"\r", b"\n")]  # first byte behind the boundary


@pytest.mark.parametrize("t_at,term", PLACEMENTS, ids=["%d-%s" % (a, t.hex()) for a, t in PLACEMENTS])
def test_terminators_across_quad_step_and_tile(gpu_ctx, t_at, term):
    data = crafted_fastq(t_at, term)
    assert_same(device_run(gpu_ctx, "fastq", data, 0, len(data)), ref_run("fastq", data, 0, len(data)), "whole")
    # an odd start: the walk crosses the same bytes, and the device window begins off a 16-byte boundary
    for start in (7, 13):
        want = ref_run("fastq", data, start, len(data))
        assert_same(device_run(gpu_ctx, "fastq", data, start, len(data)), want, ("host", start))
        assert_same(device_run(gpu_ctx, "fastq", data, start, len(data), device_window=True), want, ("device", start))
    # the same bytes as a QSEQ file are lines with the wrong field count: the status and positions agree
    assert_same(device_run(gpu_ctx, "qseq", data, 7, len(data), device_window=True),
                ref_run("qseq", data, 7, len(data)), "qseq")


def crafted_qseq(t_at, term):
    """Four 11-field lines; the first line's terminator `term` begins at file offset t_at."""
    rest = b"\t" + b"\t".join(QS[1:])
    return (b"M" * (t_at - len(rest)) + rest + term + qline(f8=b"AC.T") + b"\r" + qline(f6=b"ACG") + b"\r\n"
            + qline(f10=b"0") + b"\n")


QS_BOUNDARIES = (31, 1023, 4095)  # (a valid line is longer than 15 bytes: the second quad's last byte)
QS_PLACEMENTS = [(p - len(t) + 1, t) for p in QS_BOUNDARIES for t in (b"\r", b"\r\n", b"\n")]
QS_PLACEMENTS += [(p, b"\r\n") for p in QS_BOUNDARIES]
QS_PLACEMENTS += [(p + 1, t) for p in QS_BOUNDARIES for t in (b"\r", b"\n")]


@pytest.mark.parametrize("t_at,term", QS_PLACEMENTS, ids=["%d-%s" % (a, t.hex()) for a, t in QS_PLACEMENTS])
def test_qseq_terminators_across_quad_step_and_tile(gpu_ctx, t_at, term):
    """The same placements under the structural pass that also writes the tab bitmap: the lines are
    records here, so their fields (cut at the bitmap's tabs) are compared, not only a status."""
    data = crafted_qseq(t_at, term)
    want = ref_run("qseq", data, 0, len(data))
    assert want["status"] == ref.OK and want["n"] == 4
    assert_same(device_run(gpu_ctx, "qseq", data, 0, len(data)), want, "whole")
    for start in (7, 13):
        want = ref_run("qseq", data, start, len(data))
        assert want["n"] == 3
        assert_same(device_run(gpu_ctx, "qseq", data, start, len(data)), want, ("host", start))
        assert_same(device_run(gpu_ctx, "qseq", data, start, len(data), device_window=True), want, ("device", start))


@pytest.mark.parametrize("tail", [b"", b"\n", b"\r", b"\r\n", b"\r\r", b"\n\n"], ids=lambda t: t.hex() or "none")
def test_terminator_at_the_files_last_byte(gpu_ctx, tail):
    """The end of the file counts as "not LF": a last CR ends its line; a blank line behind the last
    record is "unexpected end of file"."""
    data = crafted_fastq(15, b"\n", tail)
    want = ref_run("fastq", data, 0, len(data))
    assert want["status"] == (ref.ERUNTIME if tail in (b"\r\r", b"\n\n") else ref.OK)
    assert_same(device_run(gpu_ctx, "fastq", data, 0, len(data)), want, tail)
    for start in (9, len(data) - 3):
        assert_same(device_run(gpu_ctx, "fastq", data, start, len(data), device_window=True),
                    ref_run("fastq", data, start, len(data)), (tail, start))
    q = b"\t".join([b"M", b"1", b"2", b"3", b"4", b"5", b"0", b"1", b"AC.T", b"hhhh", b"1"])
    qdata = q + b"\r" + q + tail
    for start in (0, 5, len(q) + 1):
        assert_same(device_run(gpu_ctx, "qseq", qdata, start, len(qdata)), ref_run("qseq", qdata, start, len(qdata)),
                    (tail, start))


def test_terminator_at_the_windows_end(gpu_ctx):
    """A CR as the window's last byte before the end of the file is undecidable: HBAM_EMORE, then the
    answer with a longer window.  A window that ends behind what the split reads is enough."""
    for term in (b"\r", b"\r\n", b"\n"):
        data = crafted_fastq(15, b"\n", b"\n")
        cut = data.index(b"#5") + 2  # the second record's quality line ends here
        data = data[:cut] + term + data[cut + 1:]
        want = ref_run("fastq", data, 0, len(data))
        assert want["n"] == 3 and want["status"] == ref.OK
        # the window ends at the terminator's first byte: for '\r' nothing tells whether '\n' follows
        dev = device_run(gpu_ctx, "fastq", data, 0, len(data), window_end=cut + 1)
        assert dev["status"] == EMORE, term
        assert_same(device_run(gpu_ctx, "fastq", data, 0, len(data), window_end=len(data)), want, term)
        # a split that ends inside the first record reads only it: the same short window answers
        short = ref_run("fastq", data, 0, 10)
        assert short["n"] == 1
        assert_same(device_run(gpu_ctx, "fastq", data, 0, 10, window_end=cut + 1), short, term)
        # the positioning walk needs line + 2: a window that ends before it asks for more
        dev = device_run(gpu_ctx, "fastq", data, 20, len(data) - 20, window_end=data.index(b"GG"))
        assert dev["status"] == EMORE
        # the same from an odd start, in a device window that begins off a 16-byte boundary
        dev = device_run(gpu_ctx, "fastq", data, 21, len(data) - 21, window_end=data.index(b"GG"), device_window=True)
        assert dev["status"] == EMORE
        dev = device_run(gpu_ctx, "fastq", data, 21, len(data) - 21, window_end=cut + 1, device_window=True)
        assert dev["status"] == EMORE, term
        assert_same(device_run(gpu_ctx, "fastq", data, 21, len(data) - 21, device_window=True),
                    ref_run("fastq", data, 21, len(data) - 21), (term, 21))
    q = b"\t".join([b"M", b"1", b"2", b"3", b"4", b"5", b"0", b"1", b"ACGT", b"hhhh", b"1"])
    qdata = q + b"\r\n" + q + b"\n"
    assert device_run(gpu_ctx, "qseq", qdata, 0, len(qdata), window_end=len(q) + 1)["status"] == EMORE
    assert_same(device_run(gpu_ctx, "qseq", qdata, 0, len(q), window_end=len(q) + 2), ref_run("qseq", qdata, 0, len(q)),
                "qseq")


def test_reader_grows_its_window(gpu_ctx, generated, monkeypatch):
    """read_split_columns starts with a tail and grows it x4 on HBAM_EMORE."""
    from hadoop_bam import fastq
    monkeypatch.setattr(fastq, "SEQ_WINDOW_TAIL", 16)
    data = generated["fastq"]
    want = ref_run("fastq", data, 100, 900)
    reader = fastq.FastqRecordReader({}, fastq.FileSplit("gen.fastq", 100, 900), data=data)
    assert reader.getPos() == want["first_pos"]
    got = []
    while reader.nextKeyValue():
        got.append((reader.getCurrentKey().encode(), reader.getCurrentValue().getSequence(), reader.getPos()))
    assert got == [(r["key"], r["seq"], r["pos_after"]) for r in want["records"]] and got


REC = b"@r1\nACGT\n+\nIIII\n"
ILL = b"@M1:%s:FC:3:4:5:6 1:N:0:AC\nACGT\n+\nIIII\n"
QS = [b"M", b"1", b"2", b"3", b"4", b"5", b"0", b"1", b"ACGT", b"hhhh", b"1"]


def qline(**kw):
    f = list(QS)
    for k, v in kw.items():
        f[int(k[1:])] = v
    return b"\t".join(f)


STATUS_CASES = [
    # (id, format, data, sanger / illumina (None = the format's default), expected status)
    ("bad-plus-line", "fastq", REC + b"@r2\nAC\nx+\nII\n" + REC, None, ref.ERUNTIME),
    ("empty-plus-line", "fastq", REC + b"@r2\nAC\n\nII\n", None, ref.ERUNTIME),
    ("eof-after-line-1", "fastq", REC + b"@r2\n", None, ref.ERUNTIME),
    ("eof-after-line-2", "fastq", REC + b"@r2\nAC", None, ref.ERUNTIME),
    ("eof-after-line-3", "fastq", REC + b"@r2\nAC\r+\r", None, ref.ERUNTIME),
    ("eof-after-line-4", "fastq", REC + b"@r2\nAC\n+\nII", None, ref.OK),
    ("trailing-blank-line", "fastq", REC + b"\n", None, ref.ERUNTIME),
    ("trailing-blank-crlf", "fastq", REC + b"\r\n", None, ref.ERUNTIME),
    ("run-number-99999999999", "fastq", ILL % b"7" + ILL % b"99999999999" + REC, None, ref.ENUMBER),
    ("run-number-after-plain-name", "fastq", REC + ILL % b"99999999999", None, ref.OK),
    ("quality-32-sanger", "fastq", REC + b"@r2\nAC\n+\nI \n", False, ref.ESEQFORMAT),
    ("quality-127-sanger", "fastq", REC + b"@r2\nAC\n+\nI\x7f\n", False, ref.ESEQFORMAT),
    ("quality-0x80-sanger", "fastq", REC + b"@r2\nAC\n+\n\x80I\n", False, ref.ESEQFORMAT),
    ("quality-63-illumina", "fastq", b"@r1\nAC\n+\nhh\n@r2\nAC\n+\nh?\n", True, ref.ESEQFORMAT),
    ("quality-126-both", "fastq", b"@r1\nAC\n+\n~@\n", True, ref.OK),
    ("sequence-10001", "fastq", b"@r1\n" + b"A" * 10001 + b"\n+\n" + b"I" * 10001 + b"\n" + REC, None, ref.OK),
    ("key-10002", "fastq", b"@" + b"k" * 10002 + b"/1\nAC\n+\nII\n" + REC, None, ref.OK),
    ("qseq-10-fields", "qseq", qline() + b"\n" + b"\t".join(QS[:10]) + b"\n", None, ref.ESEQFORMAT),
    ("qseq-12-fields", "qseq", qline() + b"\textra\n" + qline() + b"\n", None, ref.OK),
    ("qseq-trailing-tab", "qseq", b"\t".join(QS[:10]) + b"\t\n", None, ref.ESEQFORMAT),
    ("qseq-empty-line", "qseq", qline() + b"\n\n" + qline() + b"\n", None, ref.ESEQFORMAT),
    ("qseq-empty-int", "qseq", qline(f3=b"") + b"\n", None, ref.ENUMBER),
    ("qseq-plus-int", "qseq", qline(f4=b"+17", f5=b"-3") + b"\n", None, ref.OK),
    ("qseq-int-overflow", "qseq", qline(f7=b"2147483648") + b"\n", None, ref.ENUMBER),
    ("qseq-20000-byte-line", "qseq", qline() + b"\n" + qline(f8=b"A" * (19999 - len(qline(f8=b"")))) + b"\n", None,
     ref.ERUNTIME),
    ("qseq-19999-byte-line", "qseq", qline(f8=b"A" * (19998 - len(qline(f8=b"")))) + b"\n", None, ref.OK),
    ("qseq-quality-63", "qseq", qline(f9=b"hh?h") + b"\n", None, ref.ESEQFORMAT),
    ("qseq-quality-sanger", "qseq", qline(f9=b"#~5!") + b"\n", False, ref.OK),
    ("qseq-empty-index", "qseq", qline(f6=b"") + b"\n" + qline(f6=b"0A") + b"\n" + qline(f6=b".A.") + b"\n", None, ref.OK),
]


@pytest.mark.parametrize("fmt,data,illumina,status", [c[1:] for c in STATUS_CASES], ids=[c[0] for c in STATUS_CASES])
def test_one_case_per_status(gpu_ctx, fmt, data, illumina, status):
    want = ref_run(fmt, data, 0, len(data), illumina)
    assert want["status"] == status
    assert_same(device_run(gpu_ctx, fmt, data, 0, len(data), illumina), want, "whole")
    for start in (3, len(data) // 2):
        assert_same(device_run(gpu_ctx, fmt, data, start, len(data), illumina),
                    ref_run(fmt, data, start, len(data), illumina), start)


def test_truncation_counts_the_dropped_bytes(gpu_ctx):
    data = b"@r1\n" + b"A" * 10001 + b"\n+\n" + b"I" * 10001 + b"\n" + REC
    dev = device_run(gpu_ctx, "fastq", data, 0, len(data))
    assert [len(r["seq"]) for r in dev["records"]] == [10000, 4] and len(dev["records"][0]["qual"]) == 10000
    assert dev["records"][0]["pos_after"] == len(data) - len(REC) and dev["end_pos"] == len(data)


UNSUPPORTED_CASES = [
    ("empty-record-start-then-data", "fastq", REC + b"\n" + REC, 1),
    ("empty-record-start-cr-then-data", "fastq", REC + REC + b"\r" + REC, 2),
    ("key-byte-0x80", "fastq", ILL % b"7" + b"@M1:2:F\xc3\xa9:3:4:5:6 1:N:0:AC\nACGT\n+\nIIII\n" + REC, 1),
    ("qseq-byte-0x80-in-field-0", "qseq", qline() + b"\n" + qline(f0=b"M\xff") + b"\n", 1),
]


@pytest.mark.parametrize("fmt,data,n", [c[1:] for c in UNSUPPORTED_CASES], ids=[c[0] for c in UNSUPPORTED_CASES])
def test_documented_unsupported_inputs(gpu_ctx, fmt, data, n):
    from hadoop_bam import fastq
    want = ref_run(fmt, data, 0, len(data))
    assert want["status"] == ref.EUNSUPPORTED and want["n"] == n
    assert_same(device_run(gpu_ctx, fmt, data, 0, len(data)), want, "whole")
    reader = (fastq.FastqRecordReader if fmt == "fastq" else fastq.QseqRecordReader)(
        {}, fastq.FileSplit("x." + fmt, 0, len(data)), data=data)
    for _ in range(n):
        assert reader.nextKeyValue()
    with pytest.raises(fastq.SeqUnsupportedException):
        reader.nextKeyValue()


def test_high_byte_key_after_the_flag_fell_is_supported(gpu_ctx):
    """Once a key has not matched, the pattern is not run again: a byte >= 0x80 is an ordinary byte."""
    data = REC + b"@caf\xc3\xa9/2\nACGT\n+\nIIII\n"
    want = ref_run("fastq", data, 0, len(data))
    assert want["status"] == ref.OK and want["records"][1]["read"] == 2
    assert_same(device_run(gpu_ctx, "fastq", data, 0, len(data)), want, "whole")


def illumina_rec(k, passed=b"N"):
    return b"@M1:%d:FC:3:4:5:6 2:%s:0:AC\nACGTACGTAC\n+\nIIIIIIIIII\n" % (k, passed)


@pytest.mark.parametrize("flt", [False, True], ids=["all", "filter-failed-qc"])
def test_sticky_illumina_flag(gpu_ctx, flt):
    plain = b"@plain/1\nACGT\n+\nIIII\n"
    files = {
        "record-0": plain + illumina_rec(1) + illumina_rec(2),
        # 120 matching records are above 4 KiB: the first non-matching key lies in a later tile
        "later-tile": b"".join(illumina_rec(k, b"Y" if k % 3 == 0 else b"N") for k in range(120)) + plain
        + illumina_rec(200, b"Y") + illumina_rec(201),
        # the records before the non-matching one are dropped by the filter, and still counted
        "behind-dropped": illumina_rec(1, b"Y") + illumina_rec(2, b"Y") + plain + illumina_rec(3, b"Y")
        + illumina_rec(4),
        # the whole split is dropped: the filter loop runs to the end of the file
        "all-dropped": illumina_rec(1, b"Y") + illumina_rec(2, b"Y"),
    }
    for name, data in files.items():
        want = ref_run("fastq", data, 0, len(data), flt=flt)
        assert want["status"] == ref.OK
        assert_same(device_run(gpu_ctx, "fastq", data, 0, len(data), flt=flt), want, name)
        # a split that ends inside a dropped record's predecessor: the filter loop reads past its end
        for size in (50, 4099):
            check_splits(gpu_ctx, "fastq", data, size, flt=flt)
    want = ref_run("fastq", files["later-tile"], 0, len(files["later-tile"]), flt=False)
    assert want["records"][119]["instrument"] == b"M1" and want["records"][121]["instrument"] is None


def test_gz_input_through_fastq_input_format(gpu_ctx, generated, tmp_path):
    from hadoop_bam import fastq
    data = generated["fastq"]
    path = str(tmp_path / "gen.fastq.gz")
    with open(path, "wb") as f:
        f.write(gzip.compress(data))
    informat = fastq.FastqInputFormat()
    assert not informat.isSplitable(None, path)
    want = ref_run("fastq", data, 0, 1, compressed=True)  # the length is ignored: end = Long.MAX_VALUE
    assert want["n"] == ref_run("fastq", data, 0, len(data))["n"]
    reader = informat.createRecordReader(fastq.FileSplit(path, 0, 1), {})
    got = []
    while reader.nextKeyValue():
        v = reader.getCurrentValue()
        got.append((reader.getCurrentKey().encode(), v.getSequence(), v.getQuality(), v.getRead(), reader.getPos()))
    assert got == [(r["key"], r["seq"], r["qual"], r["read"], r["pos_after"]) for r in want["records"]]
    assert reader.getProgress() < 1e-9
    with pytest.raises(fastq.RuntimeException):
        informat.createRecordReader(fastq.FileSplit(path, 10, 100), {})
