"""Text VCF on the device (hbam_vcf.hip through hadoop_bam.vcf) against the tests' restatement
(tests/vcf_ref.py) and the reference's fixture (tests/golden/test.vcf, TestVCFInputFormat)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import vcf_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE_KEYS = [14369, 17329, 1110695, 1230236, 1234566]
COLUMNS = ("line_off", "line_len", "chrom", "pos", "ref_len", "key")


@pytest.fixture(scope="module")
def fixture_vcf():
    return open(os.path.join(GOLDEN, "test.vcf"), "rb").read()


class Generated:
    def __init__(self, crlf):
        self.data = vcf_ref.gen_vcf(crlf=crlf)
        self.parsed = vcf_ref.parse_header(self.data)
        self.whole = vcf_ref.read_split(self.data, 0, len(self.data), self.parsed)
        self.long = [(o, n) for o, n in zip(self.whole["line_off"], self.whole["line_len"]) if n > 190_000]


@pytest.fixture(scope="module")
def generated():
    return {"lf": Generated(False), "crlf": Generated(True)}


def _table(ctx, data):
    from hadoop_bam import vcf
    _, contigs, data_start = vcf.read_vcf_header(data)
    return ctx.vcf_contig_table(contigs), data_start


def _decode(ctx, data, start, length, table, data_start):
    from hadoop_bam import vcf
    from hadoop_bam.formats import SeekableFile
    return vcf.read_split_columns(ctx, SeekableFile(data), start, length, data_start, table)


def _same(got, ref, what):
    assert got["n"] == ref["n"], (what, got["n"], ref["n"])
    assert got["status"] == ref["status"], (what, got["status"], ref["status"])
    n = ref["n"]
    for k in COLUMNS:
        assert np.array_equal(np.asarray(got[k][:n], np.int64), np.asarray(ref[k], np.int64)), (what, k)
    assert np.array_equal(got["tab"][:n], np.asarray(ref["tab"], np.uint32).reshape(n, 8)), (what, "tab")


def test_reference_fixture_one_split(gpu_ctx, fixture_vcf):
    """TestVCFInputFormat: 5 records; testFirstSecond's assertions on the first two."""
    from hadoop_bam import bcf, vcf
    fmt = bcf.VCFInputFormat()
    split = vcf.FileSplit("test.vcf", 0, len(fixture_vcf))
    rr = fmt.createRecordReader(split, data=fixture_vcf)
    assert isinstance(rr, vcf.VCFRecordReader)
    keys, recs = [], []
    while rr.nextKeyValue():
        keys.append(rr.getCurrentKey())
        recs.append(rr.getCurrentValue())
    assert keys == FIXTURE_KEYS
    assert rr.getProgress() == 1.0
    a, b = recs[0], recs[1]
    assert a.getChr() == "20" and a.getStart() == 14370 and a.getEnd() == 14370
    assert a.getReference() == "G" and a.getAlternateAlleles()[0] == "A" and a.getID() == "rs6054257"
    assert b.getChr() == "20" and b.getStart() == 17330 and b.getEnd() == 17330
    assert b.getReference() == "T" and b.getAlternateAlleles()[0] == "A"
    assert recs[2].getAlternateAlleles() == ["G", "T"]
    assert recs[4].getReference() == "GTC" and recs[4].getEnd() == 1234569
    assert recs[4].getLine() == fixture_vcf.split(b"\n")[-2]
    rr.close()


@pytest.mark.parametrize("size", [64, 77, 229, 251, 311, 512, 1645])
def test_reference_fixture_split_sizes(gpu_ctx, fixture_vcf, size):
    """Every split's lines, keys and status equal the restatement's, the lines lost at a split's
    end - 1 (sizes 77, 229, 251, 311) and the splits that begin inside the header included."""
    table, data_start = _table(gpu_ctx, fixture_vcf)
    parsed = vcf_ref.parse_header(fixture_vcf)
    seen = []
    for start, length in vcf_ref.file_splits(len(fixture_vcf), size):
        ref = vcf_ref.read_split(fixture_vcf, start, length, parsed)
        got, _, _ = _decode(gpu_ctx, fixture_vcf, start, length, table, data_start)
        _same(got, ref, (size, start))
        seen += [int(x) for x in got["line_off"][:got["n"]]]
    # (a split that begins inside the header ends at its first '#' line: the lines after it in that
    # split are not read either, so only these sizes are plain position-rule cases)
    whole = vcf_ref.read_split(fixture_vcf, 0, len(fixture_vcf), parsed)["line_off"]
    lost = sorted(set(whole) - set(seen))
    want = {64: [], 77: [1462], 229: [1144], 1645: []}.get(size)
    if want is not None:
        assert lost == want


@pytest.mark.parametrize("variant", ["lf", "crlf"])
@pytest.mark.parametrize("size", [4096, 65537, 0])
def test_generated_file_against_the_restatement(gpu_ctx, generated, variant, size):
    """About 20,000 lines (3-4 MB): header and absent contigs (names of 1..20 bytes: every tail case
    of the hash, one and two blocks), POS 0 / 2147483647 / +5, short and 8-field lines, two lines of
    200 KB (a split wholly inside one returns nothing), a last line without a newline."""
    g = generated[variant]
    data = g.data
    assert 3_000_000 < len(data) < 4_500_000 and g.whole["n"] == 20000
    assert min(g.whole["chrom"]) < 0 and -1 in g.whole["key"] and 2147483646 in [k & 0xffffffff for k in g.whole["key"]]
    assert min(g.whole["line_len"]) < 64 and max(g.whole["line_len"]) > 190_000
    table, data_start = _table(gpu_ctx, data)
    assert data_start == g.parsed[2]
    splits = vcf_ref.file_splits(len(data), size) if size else [(0, len(data))]
    empty_inside_long = 0
    total = 0
    for start, length in splits:
        ref = vcf_ref.read_split(data, start, length, g.parsed)
        got, _, _ = _decode(gpu_ctx, data, start, length, table, data_start)
        _same(got, ref, (variant, size, start))
        total += got["n"]
        for off, ln in g.long:
            if off < start - 1 and start + length < off + ln:
                assert got["n"] == 0
                empty_inside_long += 1
    if size:
        assert empty_inside_long >= 2
        assert 20000 - len(splits) <= total <= 20000  # at most one line lost per split boundary
    else:
        assert total == 20000


def _small(bad_line):
    head = (b"##fileformat=VCFv4.1\n##contig=<ID=1,length=100>\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    good = [b"1\t%d\t.\tA\tC\t.\t.\t." % (10 + i) for i in range(3)]
    return head + b"\n".join(good[:2] + [bad_line] + good[2:]) + b"\n"


@pytest.mark.parametrize("bad", [b"1\t5\t.\tA\tC\t.\t.", b"", b"1\t12a\t.\tA\tC\t.\t.\t.", b"1\t\t.\tA\tC\t.\t.\t.",
                                 b"1\t2147483648\t.\tA\tC\t.\t.\t.", b"1\t-2147483649\t.\tA\tC\t.\t.\t.",
                                 b"1\t+-5\t.\tA\tC\t.\t.\t.", b"1\t+\t.\tA\tC\t.\t.\t."])
def test_error_lines_end_the_split(gpu_ctx, bad):
    from hadoop_bam import bcf, vcf
    data = _small(bad)
    ref = vcf_ref.read_split(data, 0, len(data))
    assert ref["n"] == 2 and ref["status"] == vcf_ref.HBAM_ETRIBBLE
    table, data_start = _table(gpu_ctx, data)
    got, _, _ = _decode(gpu_ctx, data, 0, len(data), table, data_start)
    _same(got, ref, bad)
    rr = vcf.VCFRecordReader()
    rr.initialize(vcf.FileSplit("e.vcf", 0, len(data)), data=data)
    keys, exc = bcf.record_keys(rr)
    assert list(keys) == ref["key"] and isinstance(exc, bcf.TribbleException)


def test_accepted_pos_forms(gpu_ctx):
    data = _small(b"1\t-2147483648\t.\tA\tC\t.\t.\t.\n1\t-0\t.\tA\tC\t.\t.\t.\n1\t0000000000000000000012\t.\tA\tC\t.\t.\t.")
    ref = vcf_ref.read_split(data, 0, len(data))
    assert ref["n"] == 6 and ref["status"] == 0 and ref["pos"][2:5] == [-(1 << 31), 0, 12]
    table, data_start = _table(gpu_ctx, data)
    _same(_decode(gpu_ctx, data, 0, len(data), table, data_start)[0], ref, "pos forms")


def test_split_inside_the_header_raises_runtime(gpu_ctx, fixture_vcf):
    from hadoop_bam import bcf, vcf
    ref = vcf_ref.read_split(fixture_vcf, 100, 1545)
    assert ref["n"] == 0 and ref["status"] == vcf_ref.HBAM_ERUNTIME
    rr = vcf.VCFRecordReader()
    rr.initialize(vcf.FileSplit("test.vcf", 100, 1545), data=fixture_vcf)
    keys, exc = bcf.record_keys(rr)
    assert len(keys) == 0 and isinstance(exc, bcf.BCFDecodeRuntimeException)


def test_splits_at_and_past_the_end_of_the_file(gpu_ctx, fixture_vcf):
    """A split that begins at the last byte, at the end of the file or past it reads nothing; one
    whose bound lies past the end reads to the end."""
    table, data_start = _table(gpu_ctx, fixture_vcf)
    parsed = vcf_ref.parse_header(fixture_vcf)
    n = len(fixture_vcf)
    for start, length in ((n - 1, 1), (n, 5), (n + 10, 5), (1400, 10 * n), (0, 10 * n), (1255, 0)):
        ref = vcf_ref.read_split(fixture_vcf, start, length, parsed)
        got, _, _ = _decode(gpu_ctx, fixture_vcf, start, length, table, data_start)
        _same(got, ref, (start, length))
    assert vcf_ref.read_split(fixture_vcf, 1400, 10 * n, parsed)["n"] == 2


def test_window_grows_over_a_long_line(gpu_ctx, generated, monkeypatch):
    from hadoop_bam import vcf
    g = generated["lf"]
    monkeypatch.setattr(vcf, "VCF_WINDOW_TAIL", 4096)
    i = int(np.argmax(g.whole["line_len"]))
    off, ln = g.whole["line_off"][i], g.whole["line_len"][i]
    prev = g.whole["line_off"][i - 1]
    start, length = prev, off + 10 - prev  # the long line begins inside the split, and ends far past it
    ref = vcf_ref.read_split(g.data, start, length, g.parsed)
    assert ref["line_off"][-1] == off
    rr = vcf.VCFRecordReader()
    rr.initialize(vcf.FileSplit("g.vcf", start, length), data=g.data)
    assert rr.cols["n"] == ref["n"] and rr.cols["status"] == 0
    last = None
    while rr.nextKeyValue():
        last = rr.getCurrentValue()
    assert last.getLine() == ref["lines"][-1] and len(last.getLine()) == ln
    assert rr.window_bytes > length + 1 + 4096 and rr.window_bytes >= off + ln - (start - 1)


def _upload_u32(ctx, a):
    a = np.ascontiguousarray(a, np.uint32)
    p = C.c_void_p()
    rc = ctx.L.hbam_upload(ctx.h, C.c_void_p(a.ctypes.data), a.nbytes, C.byref(p))
    assert rc == 0, ctx.last_error()
    return p


@pytest.mark.parametrize("variant", ["lf", "crlf"])
def test_gather_lines(gpu_ctx, generated, variant):
    g = generated[variant]
    table, data_start = _table(gpu_ctx, g.data)
    rc, d = gpu_ctx.vcf_decode_split_device(g.data, 0, len(g.data), data_start, table, keep_text=True)
    assert rc == 0 and d.n == 20000 and d.status == 0
    lines = g.whole["lines"]
    assert gpu_ctx.vcf_gather_lines(d) == b"".join(ln + b"\n" for ln in lines)
    perm = np.random.default_rng(3).permutation(20000).astype(np.uint32)
    p = _upload_u32(gpu_ctx, perm)
    try:
        assert gpu_ctx.vcf_gather_lines(d, p, 20000) == b"".join(lines[j] + b"\n" for j in perm)
        assert gpu_ctx.vcf_gather_lines(d, p, 777) == b"".join(lines[j] + b"\n" for j in perm[:777])
    finally:
        gpu_ctx.L.hbam_device_free(gpu_ctx.h, p)
    # without keep_text there is nothing to gather from
    rc, d2 = gpu_ctx.vcf_decode_split_device(g.data, 0, len(g.data), data_start, table)
    assert rc == 0 and not d2.text
    with pytest.raises(RuntimeError):
        gpu_ctx.vcf_gather_lines(d2)


def test_vcf_sort(gpu_ctx, generated, tmp_path):
    from hadoop_bam import vcf
    g = generated["lf"]
    header = g.parsed[0]
    lines = list(g.whole["lines"])
    random.Random(11).shuffle(lines)
    data = header + b"\n".join(lines)
    src, dst = tmp_path / "in.vcf", tmp_path / "out.vcf"
    src.write_bytes(data)
    ref = vcf_ref.read_split(data, 0, len(data))
    keys = ref["key"]
    assert min(keys) < -1 and -1 in keys and len(set(keys)) < len(keys)
    order = sorted(range(len(keys)), key=lambda j: keys[j])  # stable: ties keep input order
    info = vcf.vcf_sort(str(src), str(dst))
    assert info["n"] == 20000
    assert dst.read_bytes() == header + b"".join(ref["lines"][j] + b"\n" for j in order)
    with pytest.raises(NotImplementedError):
        vcf.vcf_sort(str(src), str(tmp_path / "out.bcf"))


def test_input_format_mirror(gpu_ctx, fixture_vcf, tmp_path):
    """bcf.VCFInputFormat over a .vcf path: the plain FileSplits, each read by a VCFRecordReader."""
    from hadoop_bam import bcf, vcf
    path = tmp_path / "fixture.vcf"
    path.write_bytes(fixture_vcf)
    fmt = bcf.VCFInputFormat()
    parsed = vcf_ref.parse_header(fixture_vcf)
    for size in (229, 1645):
        splits = fmt.getSplits(str(path), size)
        assert [(s.getStart(), s.getLength()) for s in splits] == vcf_ref.file_splits(1645, size)
        for s in splits:
            ref = vcf_ref.read_split(fixture_vcf, s.getStart(), s.getLength(), parsed)
            rr = fmt.createRecordReader(s)
            assert isinstance(rr, vcf.VCFRecordReader)
            keys, exc = bcf.record_keys(rr)
            assert list(keys) == ref["key"]
            want = {0: type(None), vcf_ref.HBAM_ERUNTIME: bcf.BCFDecodeRuntimeException}[ref["status"]]
            assert type(exc) is want
            rr.close()


def test_unaligned_device_window_and_limits(gpu_ctx, generated):
    """A device-resident window that does not begin on a 16-byte boundary gives the same columns;
    a window above 2 GiB is refused."""
    import torch
    g = generated["lf"]
    data = g.data[:300_000]
    data = data[:data.rindex(b"\n") + 1]
    ref = vcf_ref.read_split(data, 0, len(data))
    table, data_start = _table(gpu_ctx, data)
    buf = torch.zeros(len(data) + 5 + 64, dtype=torch.uint8, device="cuda")
    buf[5:5 + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    view = buf[5:5 + len(data)]
    assert view.data_ptr() % 16 == 5
    got = gpu_ctx.vcf_decode_split(view, 0, len(data), data_start, table)
    assert got["rc"] == 0
    _same(got, ref, "unaligned")
    d = _lib_columns()
    tab, size, names = table
    rc = gpu_ctx.L.hbam_vcf_decode_split(gpu_ctx.h, C.c_void_p(view.data_ptr()), 1, 0, (1 << 31) + 1, 1 << 40, 0,
                                         1 << 40, data_start, C.cast(tab, C.c_void_p), size,
                                         C.cast(C.c_char_p(names), C.c_void_p), len(names), 0, C.byref(d))
    assert rc == -11  # HBAM_EINVAL, before anything is read


def _lib_columns():
    from hadoop_bam import _lib
    return _lib.VcfColumnsC()
