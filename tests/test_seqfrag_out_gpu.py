"""FASTQ / QSEQ output on the device (hbam_fragtext.hip through Context.frag_render and
hadoop_bam.fastq_text) against the tests' restatement of the two writers (tests/seqfrag_out_ref.py,
with tests/seqfrag_ref.py as the decoder where a file is the input) and the reference's own
assertions (tests/golden/seqfrag_out/expected.json).  The device is never compared with itself."""
import io
import os
import random
import zlib

import numpy as np
import pytest

import seqfrag_out_cases as cases
import seqfrag_out_ref as ref
import seqfrag_ref
from conftest import GOLDEN
from test_seqfrag_out import IDENTITIES

pytestmark = pytest.mark.gpu

SEQ = os.path.join(GOLDEN, "seqfrag")
FILES = sorted(f for f in os.listdir(SEQ) if f.endswith((".fastq", ".qseq")))
FMT = {"fastq": cases.FASTQ, "qseq": cases.QSEQ}
EINVAL = -11


def fmt_of(name):
    return "fastq" if name.endswith(".fastq") else "qseq"


def assert_render(got, want, what):
    assert got["rc"] == 0, (what, got)
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    assert got["n"] == want["n"], (what, got["n"], want["n"])
    if want["status"]:
        assert got["err_record"] == want["err_record"], (what, got["err_record"], want["err_record"])
    assert [int(x) for x in got["line_off"]] == want["line_off"], what
    if got["text"] != want["text"]:
        at = next((i for i, (a, b) in enumerate(zip(got["text"], want["text"])) if a != b),
                  min(len(got["text"]), len(want["text"])))
        raise AssertionError((what, "text differs at byte", at, got["text"][max(0, at - 40):at + 40],
                              want["text"][max(0, at - 40):at + 40]))
    assert got["partial"] == want["partial"], (what, got["partial"][:80], want["partial"][:80])


def host_render(ctx, records, fmt, illumina, flags=0):
    c = cases.columns(records)
    return ctx.frag_render(c, c["window"], None, FMT[fmt], int(illumina), flags)


def want_render(records, fmt, illumina, flags=0):
    if flags & cases.INDEX_DOTS:
        records = [dict(f, index=None if f["index"] is None else f["index"].replace(b".", b"N")) for f in records]
    return ref.render(records, fmt, bool(illumina), bool(flags & cases.USE_KEY))


@pytest.fixture(scope="module")
def grid():
    return cases.grid_records()


# ---- 1. the reference's own assertions through the public writer classes -----------------------------
def fragment_object(f):
    from hadoop_bam import SequencedFragment
    v = SequencedFragment()
    for attr, k in (("instrument", "instrument"), ("runNumber", "run"), ("flowcellId", "flowcell"), ("lane", "lane"),
                    ("tile", "tile"), ("xpos", "xpos"), ("ypos", "ypos"), ("read", "read"),
                    ("filterPassed", "filter_passed"), ("controlNumber", "control"), ("indexSequence", "index")):
        x = f[k]
        setattr(v, attr, x.decode("ascii") if isinstance(x, bytes) else x)
    v.setSequence(f["seq"])
    v.setQuality(f["qual"])
    return v


@pytest.mark.parametrize("fmt", ["fastq", "qseq"])
def test_reference_assertions_through_the_public_classes(gpu_ctx, fmt):
    import hadoop_bam
    from hadoop_bam.fastq import RuntimeException
    section = cases.expected()[fmt]
    cls = hadoop_bam.FastqRecordWriter if fmt == "fastq" else hadoop_bam.QseqRecordWriter
    for case in section["cases"]:
        out = io.BytesIO()
        writer = cls({}, out, ctx=gpu_ctx)  # setup(): a default Configuration
        if case.get("raises"):
            with pytest.raises(RuntimeException):
                writer.setConf(case["conf"])
            continue
        writer.setConf(case["conf"])
        if not case.get("close_only"):
            writer.write(case["key"], fragment_object(cases.case_fragment(section, case)))
        writer.close(None)
        cases.check_case(case, out.getvalue())


def test_writers_batch_key_changes_and_report_failures(gpu_ctx, shorts, monkeypatch):
    """write() buffers and renders in batches: a change of `key is None` and the byte threshold both
    flush, and the output is the reference's stream whatever the batching.  A failing record leaves
    the records before it and what the reference's stream holds of it, then raises."""
    import hadoop_bam
    from hadoop_bam import fastq_text
    from hadoop_bam.fastq import RuntimeException, SeqUnsupportedException
    recs = shorts[:12]
    keyed = [k in (3, 4, 5, 6, 9) for k in range(len(recs))]
    for flush_bytes in (fastq_text._FLUSH_BYTES, 300):
        monkeypatch.setattr(fastq_text, "_FLUSH_BYTES", flush_bytes)
        for illumina in (False, True):
            conf = {"hbam.fastq-output.base-quality-encoding": "illumina" if illumina else "sanger",
                    "hbam.qseq-output.base-quality-encoding": "illumina" if illumina else "sanger"}
            out, want = io.BytesIO(), bytearray()
            w = hadoop_bam.FastqRecordWriter(conf, out, ctx=gpu_ctx)
            for f, k in zip(recs, keyed):
                w.write(f["key"].decode() if k else None, fragment_object(f))
                ref.fastq_write(want, f["key"] if k else None, f, illumina)
            w.close()
            assert out.getvalue() == bytes(want), (flush_bytes, illumina)
            out = io.BytesIO()
            w = hadoop_bam.QseqRecordWriter(conf, out, ctx=gpu_ctx)
            for f, k in zip(recs, keyed):
                w.write(f["key"].decode() if k else None, fragment_object(f))
            w.close()
            assert out.getvalue() == ref.render(recs, "qseq", illumina)["text"], (flush_bytes, illumina)
    monkeypatch.undo()
    for cls, fmt, byte, exc in ((hadoop_bam.FastqRecordWriter, "fastq", 127, hadoop_bam.FormatException),
                                (hadoop_bam.QseqRecordWriter, "qseq", 96, RuntimeException),
                                (hadoop_bam.QseqRecordWriter, "qseq", 0x80, SeqUnsupportedException)):
        bad = cases.with_qual_byte(recs, 7, -1, byte)
        out = io.BytesIO()
        w = cls({cls.CONF_BASE_QUALITY_ENCODING: "illumina"}, out, ctx=gpu_ctx)
        for f in bad:
            w.write(None, fragment_object(f))
        with pytest.raises(exc):
            w.close()
        want = ref.render(bad, fmt, True)
        assert want["err_record"] == 7
        assert out.getvalue() == want["text"] + want["partial"], fmt


# ---- 2. the field grid, host columns ------------------------------------------------------------------
@pytest.mark.parametrize("fmt,illumina,flags", [("fastq", 0, 0), ("fastq", 1, cases.USE_KEY), ("fastq", 0, cases.INDEX_DOTS),
                                                ("qseq", 1, 0), ("qseq", 0, cases.INDEX_DOTS)])
def test_field_grid_all_present_masks_in_one_call(gpu_ctx, grid, fmt, illumina, flags):
    assert sorted(int(x) for x in cases.columns(grid)["present"]) == list(range(2048))
    want = want_render(grid, fmt, illumina, flags)
    assert want["status"] == 0 and want["n"] == 2048
    lo = np.array(want["line_off"][:-1])
    assert set(int(x) for x in lo % 16) == set(range(16))
    # ... and so do the bulk regions (the byte behind the id line / the eighth tab)
    if fmt == "fastq":
        bulk = [want["text"].index(b"\n", o) + 1 for o in want["line_off"][:-1]]
        assert set(b % 16 for b in bulk) == set(range(16))
    assert_render(host_render(gpu_ctx, grid, fmt, illumina, flags), want, (fmt, illumina, flags))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("fmt", ["fastq", "qseq"])
def test_record_counts_with_a_long_read_among_short_ones(gpu_ctx, grid, fmt, n):
    recs = grid[95:95 + n]  # records 100 and 101 carry the 10,000-byte sequence and quality
    for flags in (0, cases.USE_KEY):
        assert_render(host_render(gpu_ctx, recs, fmt, 0, flags), want_render(recs, fmt, 0, flags), (fmt, n, flags))
    r = random.Random(n)
    recs = [cases.short_record(r) for _ in range(n)]
    if n > 1:
        recs[n // 2] = cases.short_record(r, cases.LONG, 17)
    assert_render(host_render(gpu_ctx, recs, fmt, 1, cases.USE_KEY), want_render(recs, fmt, 1, cases.USE_KEY), (fmt, n))


# ---- 3. quality edges -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shorts():
    r = random.Random(17)
    return [cases.short_record(r, ls) for ls in (1, 16, 17, 40, 33, 70, 5)] + \
           [cases.short_record(r) for _ in range(70)]


def test_fastq_illumina_quality_edges(gpu_ctx, shorts):
    recs = [dict(f) for f in shorts]
    recs[3]["qual"] = bytes([33, 95, 96, 126])
    got = host_render(gpu_ctx, recs, "fastq", 1, cases.USE_KEY)
    assert_render(got, want_render(recs, "fastq", 1, cases.USE_KEY), "legal")
    line = got["text"][int(got["line_off"][3]):int(got["line_off"][4])]
    assert line.endswith(b"\n+\n" + bytes([64, 126, 127, 157]) + b"\n")
    last = len(recs) - 1
    for byte in (32, 127, 0x80):
        for where in (0, -1):
            for at in (0, 37, last):
                bad = cases.with_qual_byte(recs, at, where, byte)
                want = want_render(bad, "fastq", 1, cases.USE_KEY)
                assert (want["status"], want["err_record"]) == (ref.ESEQFORMAT, at)
                assert want["partial"] == b"@" + bad[at]["key"] + b"\n" + bad[at]["seq"] + b"\n+\n"
                assert_render(host_render(gpu_ctx, bad, "fastq", 1, cases.USE_KEY), want, (byte, where, at))
                # makeId's id line in the partial record
                assert_render(host_render(gpu_ctx, bad, "fastq", 1, 0), want_render(bad, "fastq", 1, 0), (byte, at))
    two = cases.with_qual_byte(cases.with_qual_byte(recs, 50, 0, 127), 20, -1, 32)
    want = want_render(two, "fastq", 1, cases.USE_KEY)
    assert want["err_record"] == 20
    assert_render(host_render(gpu_ctx, two, "fastq", 1, cases.USE_KEY), want, "two")


def test_fastq_sanger_passes_any_byte(gpu_ctx, shorts):
    recs = [dict(f) for f in shorts]
    recs[2]["qual"] = bytes(range(256))
    recs[9]["qual"] = bytes([0, 10, 13, 0x7f, 0x80, 0xff])
    want = want_render(recs, "fastq", 0, cases.USE_KEY)
    assert want["status"] == 0
    assert_render(host_render(gpu_ctx, recs, "fastq", 0, cases.USE_KEY), want, "sanger")


def test_qseq_quality_edges(gpu_ctx, shorts):
    recs = [dict(f) for f in shorts]
    recs[3]["qual"] = bytes([95, 0x20, 33, 0])
    want = want_render(recs, "qseq", 1)
    assert want["status"] == 0
    got = host_render(gpu_ctx, recs, "qseq", 1)
    assert_render(got, want, "legal")
    assert bytes([126, 0x3f, 64, 31]) + b"\t" in got["text"][int(got["line_off"][3]):int(got["line_off"][4])]
    for at, where in ((0, 0), (37, -1), (len(recs) - 1, -1)):
        bad = cases.with_qual_byte(recs, at, where, 96)
        want = want_render(bad, "qseq", 1)
        assert (want["status"], want["err_record"], want["partial"]) == (ref.ERUNTIME, at, b"")
        assert_render(host_render(gpu_ctx, bad, "qseq", 1), want, ("96", at))
    for illumina in (0, 1):
        for at in (0, 41, len(recs) - 1):
            bad = cases.with_qual_byte(recs, at, -1, 0x80)
            want = want_render(bad, "qseq", illumina)
            assert (want["status"], want["err_record"]) == (ref.EUNSUPPORTED, at)
            assert_render(host_render(gpu_ctx, bad, "qseq", illumina), want, ("qual 0x80", illumina, at))
            bad = [dict(f) for f in recs]
            bad[at]["seq"] = bad[at]["seq"] + b"\x80"
            want = want_render(bad, "qseq", illumina)
            assert (want["status"], want["err_record"]) == (ref.EUNSUPPORTED, at)
            assert_render(host_render(gpu_ctx, bad, "qseq", illumina), want, ("seq 0x80", illumina, at))
    # a byte > 95 before the byte >= 0x80, in one unit and 70 bytes apart
    for qual in (bytes([100, 0x81]), bytes([100]) + bytes(70 * [40]) + bytes([0x81])):
        bad = [dict(f) for f in recs]
        bad[12]["qual"] = qual
        want = want_render(bad, "qseq", 1)
        assert (want["status"], want["err_record"]) == (ref.EUNSUPPORTED, 12)
        assert_render(host_render(gpu_ctx, bad, "qseq", 1), want, "both")
    # Sanger: verbatim
    recs[5]["qual"] = bytes(range(0x80))
    want = want_render(recs, "qseq", 0)
    assert want["status"] == 0
    assert_render(host_render(gpu_ctx, recs, "qseq", 0), want, "sanger")


def test_invalid_arguments(gpu_ctx, shorts):
    c = cases.columns(shorts[:4])
    assert gpu_ctx.frag_render(c, c["window"], None, 2, 0, 0)["rc"] == EINVAL
    assert gpu_ctx.frag_render(c, c["window"], None, 0, 2, 0)["rc"] == EINVAL
    assert gpu_ctx.frag_render(c, c["window"], 5, 0, 0, 0)["rc"] == EINVAL
    assert gpu_ctx.frag_render(c, c["window"][:-1], None, 0, 0, 0)["rc"] == EINVAL  # the last string runs past
    d = dict(c, seq_off=c["seq_off"][::-1].copy())
    assert gpu_ctx.frag_render(d, c["window"], None, 0, 0, 0)["rc"] == EINVAL
    import torch
    perm = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert gpu_ctx.frag_render(c, c["window"], 4, 0, 0, 0, perm=perm)["rc"] == EINVAL  # perm with host columns
    assert gpu_ctx.frag_render(c, c["window"], 4, 0, 0, 0)["rc"] == 0


# ---- 4. / 5. device columns ---------------------------------------------------------------------------
def ref_decode(fmt, data, start=0, length=None):
    run = seqfrag_ref.run_fastq if fmt == "fastq" else seqfrag_ref.run_qseq
    return run(data, start, len(data) if length is None else length, fmt == "qseq")


def device_decode(ctx, fmt, data, device_window):
    """The whole file decoded on the device -> (device columns, the window argument); device_window:
    a device tensor slice that begins one byte into its allocation."""
    arg = bytes(data)
    if device_window:
        import torch
        t = torch.zeros(len(data) + 1 + 64, dtype=torch.uint8, device="cuda")
        t[1:1 + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        arg = t[1:1 + len(data)]
        assert arg.data_ptr() % 2 == 1
    rc, d = ctx.frag_decode_split_device(fmt, arg, 0, len(data), int(fmt == "qseq"), False)
    assert rc == 0, ctx.last_error()
    return d, arg


def convert_flags(src, dst):
    return (cases.INDEX_DOTS if src == "qseq" else 0) | (cases.USE_KEY if src == dst == "fastq" else 0)


@pytest.mark.parametrize("name", FILES)
def test_device_columns_of_every_fixture(gpu_ctx, name):
    src = fmt_of(name)
    data = open(os.path.join(SEQ, name), "rb").read()
    dec = ref_decode(src, data)
    for dst in ("fastq", "qseq"):
        flags = convert_flags(src, dst)
        # (the restatement's decode has already replaced the dots of a QSEQ index)
        want = ref.render(dec["records"], dst, dst == "qseq", bool(flags & cases.USE_KEY))
        for device_window in (False, True):
            d, window = device_decode(gpu_ctx, src, data, device_window)
            assert int(d.n) == dec["n"] and int(d.status) == dec["status"]
            got = gpu_ctx.frag_render(d, window, None, FMT[dst], int(dst == "qseq"), flags)
            assert_render(got, want, (name, dst, device_window))
    if name == "indexWithUnknown.qseq":
        want = ref.render(dec["records"], "fastq", False)
        assert dec["n"] >= 1 and b"N" in want["text"].split(b"\n")[0].rsplit(b":", 1)[1]


@pytest.mark.parametrize("name,fmt,illumina,use_key", IDENTITIES)
def test_identities_on_the_device(gpu_ctx, name, fmt, illumina, use_key):
    data = open(os.path.join(SEQ, name), "rb").read()
    rc, d = gpu_ctx.frag_decode_split_device(fmt, data, 0, len(data), int(illumina), False)
    assert rc == 0 and int(d.status) == 0
    flags = (cases.USE_KEY if use_key else 0) | (cases.INDEX_DOTS if fmt == "qseq" else 0)
    got = gpu_ctx.frag_render(d, data, None, FMT[fmt], int(illumina), flags)
    assert got["rc"] == 0 and got["status"] == 0
    assert got["text"] == data + b"\n"


def test_perm_on_device_columns(gpu_ctx):
    import torch
    data = seqfrag_ref.generate_fastq()
    dec = ref_decode("fastq", data)
    n = dec["n"]
    assert dec["status"] == 0 and n > 40
    d, window = device_decode(gpu_ctx, "fastq", data, False)
    assert int(d.n) == n
    r = random.Random(4)
    perms = {"reverse": list(range(n - 1, -1, -1)), "subset": sorted(r.sample(range(n), n // 3)),
             "duplicates": [r.randrange(n) for _ in range(2 * n + 5)]}
    for what, p in perms.items():
        t = torch.tensor(p, dtype=torch.int32, device="cuda")
        for dst, flags in (("fastq", cases.USE_KEY), ("fastq", 0), ("qseq", 0)):
            want = ref.render([dec["records"][i] for i in p], dst, False, bool(flags))
            got = gpu_ctx.frag_render(d, window, len(p), FMT[dst], 0, flags, perm=t)
            assert_render(got, want, (what, dst, flags))
    # an index outside the columns ends the output there, with HBAM_EINVAL as the status
    t = torch.tensor([3, 1, n, 0], dtype=torch.int32, device="cuda")
    got = gpu_ctx.frag_render(d, window, 4, cases.FASTQ, 0, cases.USE_KEY, perm=t)
    want = ref.render([dec["records"][3], dec["records"][1]], "fastq", False, True)
    assert (got["rc"], got["status"], got["err_record"], got["n"]) == (0, EINVAL, 2, 2)
    assert got["text"] == want["text"]


def device_columns(ctx, c):
    """cases.columns' host arrays uploaded -> (a device FragColumnsC, the buffers to free)."""
    from hadoop_bam._lib import FragColumnsC
    d, bufs = FragColumnsC(), []
    d.n, d.host = c["n"], 0

    def up(name, a):
        bufs.append(ctx.upload(np.ascontiguousarray(a).tobytes() + bytes(16)))
        setattr(d, name, bufs[-1].ptr)
    for k in ("present",) + cases.INT_COLS + cases.STR_COLS:
        up(k, c[k])
    for k in ("key", "seq", "qual"):
        up(k + "_off", c[k + "_off"])
        up(k, c[k])
        setattr(d, k + "_len", len(c[k]))
    return d, bufs


@pytest.mark.parametrize("fmt", ["fastq", "qseq"])
def test_a_bad_index_and_a_bad_quality_byte_in_one_call(gpu_ctx, shorts, fmt):
    """130 output positions over device columns: an index outside the columns (the sizes pass's
    HBAM_EINVAL) and a record with an illegal quality byte (the bulk pass), either one first.  The
    first of the two in output order ends the output.  The restatement knows no index, so the
    expectation is its render of the records before the bad index: with the quality byte among them it
    stops there with the writer's exception and the partial record; with the byte behind the bad index
    it renders them all, and the status is HBAM_EINVAL at that position."""
    import torch
    recs = cases.with_qual_byte(shorts, 7, -1, 127 if fmt == "fastq" else 96)
    c = cases.columns(recs)
    d, bufs = device_columns(gpu_ctx, c)
    try:
        for bad_index, bad_qual in ((100, 40), (40, 100)):
            perm = [(3 * k) % 7 + 8 * (k % 8) + 8 for k in range(130)]  # never record 7
            perm[bad_qual], perm[bad_index] = 7, len(recs)
            assert max(perm[:bad_index] + perm[bad_index + 1:]) < len(recs) and perm.count(7) == 1
            want = ref.render([recs[i] for i in perm[:bad_index]], fmt, True, True)
            t = torch.tensor(perm, dtype=torch.int32, device="cuda")
            got = gpu_ctx.frag_render(d, c["window"], len(perm), FMT[fmt], 1, cases.USE_KEY, perm=t)
            if bad_qual < bad_index:
                assert (want["status"], want["err_record"]) == (ref.ESEQFORMAT if fmt == "fastq" else ref.ERUNTIME, 40)
                assert (len(want["partial"]) > 0) == (fmt == "fastq")
                assert_render(got, want, (fmt, "quality first"))
            else:
                assert (want["status"], want["n"], len(want["line_off"])) == (0, 40, 41)
                assert (got["rc"], got["status"], got["err_record"], got["n"]) == (0, EINVAL, 40, 40)
                assert [int(x) for x in got["line_off"]] == want["line_off"]
                assert (got["text"], got["partial"]) == (want["text"], b"")
    finally:
        for b in bufs:
            b.free()


# ---- 6. convert -----------------------------------------------------------------------------------------
def generated_fastq(term, records=2000, seed=9):
    r = random.Random(seed)
    out = bytearray()
    for k in range(records):
        n = r.randrange(30, 150)
        seq = bytes(r.choice(b"ACGTN") for _ in range(n))
        qual = bytes(r.randrange(33, 127) for _ in range(n))
        if k < records // 2:
            name = b"M%d:%d:FC%d:%d:%d:%d:%d %d:%s:%d:%s" % (
                r.randrange(100), r.randrange(1000), r.randrange(10), r.randrange(1, 9), r.randrange(1, 3000),
                r.randrange(-50, 30000), r.randrange(-50, 30000), r.randrange(1, 4), r.choice((b"Y", b"N")),
                r.randrange(0, 40), r.choice((b"ACGTAC", b"", b"NNN")))
        else:
            name = b"read.%d plain/%d" % (k, 1 + k % 2)
        for line in (b"@" + name, seq, b"+", qual):
            out += line + term
    return bytes(out)


@pytest.mark.parametrize("term", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_convert_over_three_splits(gpu_ctx, term, tmp_path):
    import hadoop_bam
    data = generated_fastq(term)
    dec = ref_decode("fastq", data)
    assert dec["status"] == 0 and dec["n"] == 2000
    want = ref.render(dec["records"], "fastq", False, True)["text"]
    out = io.BytesIO()
    n = hadoop_bam.convert(data, out, "fastq", "fastq", split_size=len(data) // 3 + 1)
    assert n == 2000 and out.getvalue() == want
    out = io.BytesIO()
    assert hadoop_bam.convert(data, out, "fastq", "qseq", split_size=len(data) // 3 + 1,
                              conf={"hbam.qseq-output.base-quality-encoding": "sanger"}) == 2000
    assert out.getvalue() == ref.render(dec["records"], "qseq", False)["text"]
    src = str(tmp_path / "in.fastq")
    with open(src, "wb") as f:
        f.write(data)
    dst = str(tmp_path / "out.fastq")
    assert hadoop_bam.convert(src, dst, "fastq", "fastq", split_size=len(data) // 3 + 1, compress=True) == 2000
    raw = open(dst + ".gz", "rb").read()
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    text = bytearray()
    while raw:
        z = zlib.decompressobj(31)
        text += z.decompress(raw) + z.flush()
        raw = z.unused_data
    assert bytes(text) == want
    reader = hadoop_bam.FastqInputFormat().createRecordReader(hadoop_bam.FileSplit(dst + ".gz", 0, os.path.getsize(dst + ".gz")), {})
    k = 0
    while reader.next():
        f = dec["records"][k]
        assert reader.getCurrentKey().encode() == f["key"], k
        v = reader.getCurrentValue()
        assert (v.sequence, v.quality) == (f["seq"], f["qual"]), k
        k += 1
    assert k == 2000


# ---- 7. context reuse ------------------------------------------------------------------------------------
def test_context_reuse(gpu_ctx, grid, shorts):
    big = want_render(grid, "fastq", 0, cases.USE_KEY)
    assert_render(host_render(gpu_ctx, grid, "fastq", 0, cases.USE_KEY), big, "large")
    assert_render(host_render(gpu_ctx, shorts[:1], "qseq", 1), want_render(shorts[:1], "qseq", 1), "small")
    data = seqfrag_ref.generate_qseq()
    dec = ref_decode("qseq", data)
    d, window = device_decode(gpu_ctx, "qseq", data, False)
    assert int(d.n) == dec["n"] > 0
    got = gpu_ctx.frag_render(d, window, None, cases.QSEQ, 1, cases.INDEX_DOTS)
    assert_render(got, ref.render(dec["records"], "qseq", True), "decode then render")
    assert_render(host_render(gpu_ctx, grid, "qseq", 0), want_render(grid, "qseq", 0), "large again")
