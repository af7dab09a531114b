"""SAM text output on the device (hbam_samtext.hip through Context.sam_render, SAMRecordWriter and
view) against the tests' restatement (tests/samtext_ref.py), byte for byte, never against the
product's host renderer.  Deferral must not hide a device failure: every test pins the deferred
count or list."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import f4_records
import sam_cases
import sam_ref
import samtext_cases as cases
import samtext_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_BAMS = ["small_pe.bam", "edge_uniform_long.bam", "edge_unsorted_l1.bam"]
_GOLDEN = {}


def golden(name):
    """(file bytes, header, names, records, the restatement's render) of a golden BAM, computed once."""
    if name not in _GOLDEN:
        data = np.fromfile(os.path.join(GOLDEN, name), np.uint8)
        h, recs = sam_cases.bam_header_and_records(data)
        names = [n for n, _ in h.refs]
        _GOLDEN[name] = (data, h, names, recs, ref.render(recs, names))
    return _GOLDEN[name]


def same(got, want, what=""):
    assert got["rc"] == 0, (what, got)
    assert got["n"] == want["n"] and got["status"] == want["status"], (what, got["n"], got["status"], want["n"],
                                                                       want["status"])
    assert got["err_record"] == (want["n"] if want["status"] else 0), what
    assert [int(x) for x in got["deferred"]] == want["deferred"], what
    assert np.array_equal(got["line_off"], want["line_off"]), what
    assert got["text"] == want["text"], what


def render_host(ctx, slots, names=cases.NAMES):
    ub, off = f4_records.pack(slots)
    return ctx.sam_render(ub, off, len(slots), names, on_device=False)


class Dev:
    """Host arrays uploaded to the device with 64 bytes of slack, freed on exit."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def __enter__(self):
        return self

    def up(self, a):
        a = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])
        p = C.c_void_p()
        assert self.ctx.L.hbam_upload(self.ctx.h, C.c_void_p(a.ctypes.data), a.size, C.byref(p)) == 0
        self.bufs.append(p)
        return p.value

    def __exit__(self, *exc):
        for p in self.bufs:
            self.ctx.L.hbam_device_free(self.ctx.h, p)


def decode_bam(ctx, data, n_ref):
    h = ctx.parse_header(data)
    rc, d = ctx.decode_split_device(data, h["first_voffset"], (len(data) << 16) | 0xffff, n_ref)
    assert rc == 0 and int(d.status) == 0
    return d


@pytest.mark.parametrize("name", GOLDEN_BAMS)
def test_golden_bam_whole_file(gpu_ctx, name):
    """The columns of a whole-file decode rendered where they stand: the whole text equals the
    restatement and nothing is deferred (the files hold only i and Z tags)."""
    data, h, names, recs, want = golden(name)
    d = decode_bam(gpu_ctx, data, len(names))
    assert int(d.n_records) == len(recs) > 0
    got = gpu_ctx.sam_render(d.ubuf, d.rec_off, len(recs), names)
    assert want["deferred"] == [] and want["status"] == 0
    same(got, want, name)
    assert got["timing"]["n_records"] == len(recs) and got["timing"]["ubuf_bytes"] == len(want["text"])


def test_crafted_records_and_deferral(gpu_ctx):
    """The 95 crafted records (l_seq 0-65, 70, 100, 3001; names of 1-10 and 254 bytes; 300 CIGAR
    ops; 14 absent QUALs; every tag type): exactly one is deferred.  Then the float records: values
    in the device's domain, singly and in B:f, come from the device; values just outside it and H
    tags are deferred; the deferred list is the restatement's predicate exactly."""
    recs = cases.crafted_records()
    want = ref.render(recs, cases.NAMES)
    assert want["n"] == 95 and len(want["deferred"]) == 1
    assert sum(1 for r in recs if sam_ref.fields(r)["l_seq"] and sam_ref.fields(r)["qual"][0] == 0xff) == 14
    same(render_host(gpu_ctx, recs), want, "crafted")
    fl = cases.float_records()
    want = ref.render([r for r, _ in fl], cases.NAMES)
    assert want["deferred"] == [k for k, (_, d) in enumerate(fl) if d] and 0 < len(want["deferred"]) < len(fl)
    assert b"XF:f:9999999.0\n" in want["text"] and b"XF:f:-0.0\n" in want["text"] and b"XB:B:f\n" in want["text"]
    assert b"XB:B:f,1.0,-3.0,0.0,-0.0,9999999.0," in want["text"]
    same(render_host(gpu_ctx, [r for r, _ in fl]), want, "floats")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_tile_and_alignment_edges(gpu_ctx, n):
    """Name lengths 1-16 put the SEQ region at every output offset mod 16; l_seq 1, 15, 16, 17, 31,
    32, 33 and one read of about 6 KB; n around the 64-line tile.  Device-resident too, with a perm
    that reverses and one that repeats an index."""
    recs = cases.edge_records(n)
    want = ref.render(recs, cases.NAMES)
    assert want["n"] == n and want["deferred"] == []
    if n == 129:  # the region's first byte: behind the ninth tab
        starts = {(int(want["line_off"][k]) + len(b"\t".join(ln.split(b"\t")[:9])) + 1) % 16
                  for k, ln in enumerate(want["lines"])}
        assert starts == set(range(16))
    same(render_host(gpu_ctx, recs), want, n)
    if n < 2:
        return
    ub, off = f4_records.pack(recs)
    rev = np.arange(n, dtype=np.uint32)[::-1].copy()
    rep = np.array([k // 2 for k in range(n)], np.uint32)
    with Dev(gpu_ctx) as dev:
        dub, doff = dev.up(ub), dev.up(off)
        same(gpu_ctx.sam_render(dub, doff, n, cases.NAMES), want, "device")
        for perm in (rev, rep):
            got = gpu_ctx.sam_render(dub, doff, n, cases.NAMES, perm=dev.up(perm))
            same(got, ref.render([recs[int(i)] for i in perm], cases.NAMES), "perm")


@pytest.mark.parametrize("case", cases.status_cases(), ids=[c[0] for c in cases.status_cases()])
def test_status_cases(gpu_ctx, case):
    """A malformed record at positions 0, 63, 64 and last of a 130-record stream: its status,
    err_record = n_records = its index, and the text of the records before it."""
    name, status, slot = case
    for at in (0, 63, 64, 129):
        slots = cases.stream(slot, at)
        want = ref.render(slots, cases.NAMES)
        assert want["status"] == status and want["n"] == at and want["deferred"] == []
        same(render_host(gpu_ctx, slots), want, (name, at))


@pytest.mark.parametrize("case", cases.stop_streams(), ids=[c[0] for c in cases.stop_streams()])
def test_stops_among_deferred_records(gpu_ctx, case):
    """A stop found by the sizes pass, by the bulk pass, or by both in one stream, with deferred records
    before and behind it: the first failing record in output order ends the output, the deferred list
    holds the positions before it, and text_len is the offset of that record's line."""
    name, slots, n, status, deferred = case
    want = ref.render(slots, cases.NAMES)
    assert (want["n"], want["status"], want["deferred"]) == (n, status, deferred)
    got = render_host(gpu_ctx, slots)
    same(got, want, name)
    assert len(got["text"]) == int(got["line_off"][n])


@pytest.mark.parametrize("name", GOLDEN_BAMS)
def test_sam_text_in_and_out_on_the_device(gpu_ctx, name):
    """SAM text -> hbam_sam_decode_split -> hbam_sam_render over the decode's device columns gives
    back the original lines."""
    from hadoop_bam import read_sam_text_header
    data, h, names, recs, want = golden(name)
    sam = sam_ref.sam_file(sam_ref.header_text(h.text, h.refs), [ln[:-1] for ln in want["full"]])
    _, data_start, header = read_sam_text_header(sam)
    rc, d = gpu_ctx.sam_decode_split_device(sam, 0, len(sam), data_start, gpu_ctx.vcf_contig_table(names), len(names))
    assert rc == 0 and int(d.status) == 0 and int(d.n_records) == len(recs)
    got = gpu_ctx.sam_render(d.ubuf, d.rec_off, len(recs), names)
    assert got["rc"] == 0 and got["status"] == 0 and len(got["deferred"]) == 0
    assert got["text"] == sam[data_start:]


def test_sorted_run_written_from_the_device(gpu_ctx):
    """A sorted run's payload through SAMRecordWriter.write_device: the header text, then the lines
    in key order (stable), the one deferred line spliced in by the host."""
    from hadoop_bam import SAMFileHeader, SAMRecordWriter, sort
    recs = cases.crafted_records()
    names = cases.NAMES
    sam = sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines())
    whole = sam_ref.decode_split(sam, 0, len(sam))
    rc, d = gpu_ctx.sam_decode_split_device(sam, 0, len(sam), sam_ref.data_start(sam),
                                            gpu_ctx.vcf_contig_table(names), len(names))
    assert rc == 0 and int(d.status) == 0 and int(d.n_records) == len(recs) == whole["n"]
    run = sort.HipSortOps(gpu_ctx).run_from_columns(d)
    order = np.argsort(whole["key"], kind="stable")
    out = io.BytesIO()
    w = SAMRecordWriter(out, SAMFileHeader(b"\n".join(sam_cases.HEADER), sam_cases.REFS), True, gpu_ctx)
    w.write_device(run.payload, run.offsets, run.n)
    w.close()
    want = ref.render([recs[int(i)] for i in order], names)
    assert len(want["deferred"]) == 1
    assert out.getvalue() == b"".join(ln + b"\n" for ln in sam_cases.HEADER) + b"".join(want["full"])


def test_output_format_sam_reads_back(gpu_ctx, tmp_path):
    """hadoopbam.anysam.output-format=SAM parts without headers merged by merge_sam_into(fmt="SAM"):
    SAMRecordReader reads the file back to the same records."""
    from hadoop_bam import (Configuration, FileSplit, KeyIgnoringAnySAMOutputFormat, SAMFileHeader, SAMRecordReader,
                            merge_sam_into)
    from hadoop_bam.output import get_mergeable_work_file
    recs = [r for r in cases.crafted_records() if not ref.deferred(r)] + [r for r, d in cases.float_records() if not d]
    header = SAMFileHeader(b"\n".join(sam_cases.HEADER), sam_cases.REFS)
    f = KeyIgnoringAnySAMOutputFormat(Configuration({"hadoopbam.anysam.output-format": "SAM",
                                                     "hadoopbam.anysam.write-header": "false"}))
    f.setSAMHeader(header)
    d = tmp_path / "work"
    d.mkdir()
    half = len(recs) // 2
    for task, part in enumerate((recs[:half], recs[half:])):
        w = f.getRecordWriter(get_mergeable_work_file(str(d), "", "", "part", task), ctx=gpu_ctx)
        w.write_encoded(b"".join(part))
        w.close()
    merged = str(tmp_path / "merged.sam")
    merge_sam_into(merged, str(d), "", "", header, "part", ctx=gpu_ctx, fmt="SAM")
    data = open(merged, "rb").read()
    assert data == b"".join(ln + b"\n" for ln in sam_cases.HEADER) + b"".join(ref.line(r, cases.NAMES) for r in recs)
    rr = SAMRecordReader()
    rr.initialize(FileSplit(merged, 0, len(data)))
    back = []
    while rr.nextKeyValue():
        back.append(rr.getCurrentValue().get().toBAMBytes())
    assert back == recs


def test_view(gpu_ctx, tmp_path, monkeypatch):
    """view of small_pe.bam: the whole file against the restatement, two regions against
    IndexedBAMReader.query_region rendered by the restatement, and the plugin's return codes.  The
    windows are made small, so the BAM is streamed in several windows and the SAM file decoded in
    several splits."""
    from hadoop_bam import Configuration, sam_text, view
    from hadoop_bam.formats import context
    from hadoop_bam.index import BAMIndexer, IndexedBAMReader
    monkeypatch.setattr(sam_text, "VIEW_WINDOW_BYTES", 256 << 10)
    monkeypatch.setattr(sam_text, "VIEW_SPLIT_BYTES", 50000)
    data, h, names, recs, want = golden("small_pe.bam")
    header = b"".join(ln + b"\n" for ln in sam_ref.header_text(h.text, h.refs))
    path = str(tmp_path / "in.bam")
    data.tofile(path)
    out = io.BytesIO()
    assert view(path, out=out) == 0  # no index yet: the whole file needs none
    assert out.getvalue() == header + want["text"] and want["deferred"] == []
    assert context().last_stream_stats["windows"] > 4
    out = io.BytesIO()
    assert view(path, out=out, header_only=True) == 0 and out.getvalue() == header
    cut = str(tmp_path / "cut.bam")  # a file cut short: what stands is printed, and the code says so
    data[:2 * len(data) // 3].tofile(cut)
    out = io.BytesIO()
    assert view(cut, out=out) == 4
    assert len(header) + 100000 < len(out.getvalue()) < len(header + want["text"])
    assert (header + want["text"]).startswith(out.getvalue())
    assert view(path, out=io.BytesIO(), fmt="bam") == 1
    assert view(str(tmp_path / "missing.bam"), out=io.BytesIO()) == 4
    assert view(path, ["%s:1-5000" % names[0].decode()], out=io.BytesIO()) == 4  # no index
    BAMIndexer(gpu_ctx).index(path)
    rd = IndexedBAMReader(path, gpu_ctx)
    placed = [f for f in (sam_ref.fields(r) for r in recs[::97]) if f["ref"] >= 0 and not f["flag"] & 4 and f["cigar"]]
    a, b = placed[0], placed[-1]
    n0 = names[a["ref"]].decode()
    regions = ["%s:%d-%d" % (n0, a["pos"] + 1, a["pos"] + 50001), names[b["ref"]].decode()]
    expect = b""
    for r in regions:
        hits = rd.query_region(r)
        assert len(hits) > 0
        expect += b"".join(ref.line(x.toBAMBytes(), names) for x in hits)
    out = io.BytesIO()
    assert view(path, regions, out=out) == 0
    assert out.getvalue() == header + expect
    out = io.BytesIO()  # invalid regions: skipped, 5 once the valid ones are written
    assert view(path, ["nope:1-2", regions[0], "%s:10-5" % n0], out=out) == 5
    assert out.getvalue() == header + b"".join(ref.line(x.toBAMBytes(), names) for x in rd.query_region(regions[0]))
    sam = str(tmp_path / "in.sam")
    with open(sam, "wb") as f:
        f.write(header + b"".join(want["full"][:500]))
    out = io.BytesIO()
    assert view(sam, out=out) == 0 and out.getvalue() == header + b"".join(want["full"][:500])
    assert view(sam, [n0], out=io.BytesIO()) == 4  # regions from a SAM file
    assert view(sam, out=io.BytesIO(), conf=Configuration()) == 0
    # what view printed is a SAM file: SAMRecordReader reads it back to the same records (as lines: the
    # golden file's integer tags are not all of the narrowest width)
    from hadoop_bam import FileSplit, SAMRecordReader
    printed = str(tmp_path / "printed.sam")
    with open(printed, "wb") as f:
        f.write(out.getvalue())
    rr, back = SAMRecordReader(), []
    rr.initialize(FileSplit(printed, 0, len(out.getvalue())))
    while rr.nextKeyValue():
        back.append(ref.line(rr.getCurrentValue().get().toBAMBytes(), names))
    assert back == want["full"][:500]
    for junk in (b"\x1f\x8b\x08\x04 not a BGZF block", b"r1\tnot\ta\tSAM\tline\n"):  # cannot parse
        bad = str(tmp_path / "junk")
        with open(bad, "wb") as f:
            f.write(junk)
        assert view(bad, out=io.BytesIO()) == 4
