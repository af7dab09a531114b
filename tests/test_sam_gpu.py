"""SAM text on the device (hbam_sam.hip through hadoop_bam.sam) against the tests' restatement
(tests/sam_ref.py), the CPU oracle's decode of the same records as BAM, and the existing BAM
pipeline fed the same records."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import sam_cases
import sam_ref
import vcf_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_BAMS = ["small_pe.bam", "edge_uniform_long.bam", "edge_unsorted_l1.bam"]
EUNSUPPORTED, EINVAL, EMORE = sam_ref.HBAM_EUNSUPPORTED, sam_ref.HBAM_EINVAL, sam_ref.HBAM_EMORE


class Sam:
    """A SAM file, what the host parses of it, and the restatement's whole-file decode."""

    def __init__(self, data):
        from hadoop_bam import read_sam_text_header
        self.data = data
        _, self.data_start, self.header = read_sam_text_header(data)
        self.names = [n for n, _ in self.header.refs]
        self.n_ref = len(self.names)
        self.whole = sam_ref.decode_split(data, 0, len(data))

    def table(self, ctx):
        return ctx.vcf_contig_table(self.names)

    def decode(self, ctx, start, length):
        """Through the reader's window policy -> host columns"""
        from hadoop_bam import sam
        from hadoop_bam.formats import SeekableFile
        return sam.read_split_columns(ctx, SeekableFile(self.data), start, length, self.data_start, self.table(ctx),
                                      self.n_ref)[0]

    def expect(self, start, length):
        """The restatement's result for a split, cut from the whole-file decode by the offset rule."""
        w = self.whole
        lo, hi = max(start, self.data_start), start + length
        if w["status"] != 0:  # a failing line: decode this split on its own
            return sam_ref.decode_split(self.data, start, length)
        idx = [i for i, o in enumerate(w["voffset"]) if lo <= int(o) < hi]
        recs = [w["records"][i] for i in idx]
        ro = np.zeros(len(idx) + 1, np.uint64)
        ro[1:] = np.cumsum([len(r) for r in recs])
        return dict(n=len(idx), status=0, ubuf=np.frombuffer(b"".join(recs), np.uint8), rec_off=ro,
                    key=w["key"][idx], voffset=w["voffset"][idx])


def same(got, ref, what=""):
    assert got["n"] == ref["n"], (what, got["n"], ref["n"])
    assert got["status"] == ref["status"], (what, got["status"], ref["status"])
    n = ref["n"]
    assert np.array_equal(got["rec_off"][:n], ref["rec_off"][:n]), (what, "rec_off")
    assert got["ubuf"].tobytes() == ref["ubuf"].tobytes(), (what, "ubuf")
    assert np.array_equal(got["key"][:n], ref["key"]), (what, "key")
    assert np.array_equal(got["voffset"][:n], ref["voffset"]), (what, "voffset")
    assert np.array_equal(got["block_size"][:n].astype(np.int64) + 4, np.diff(ref["rec_off"].astype(np.int64)))


@pytest.fixture(scope="module")
def generated(genbam):
    bam = np.asarray(genbam.generate(records=3000, seed=7, odd_every=97, unplaced_permille=30,
                                     mate_unmapped_permille=30))
    return {"bam": bam, "lf": Sam(sam_cases.sam_of_bam(bam)[0]), "crlf": Sam(sam_cases.sam_of_bam(bam, b"\r\n")[0])}


def _against_oracle(got, bam, oracle_mod):
    h = oracle_mod.read_header(bam)
    ref = oracle_mod.read_split(bam, h["first_voffset"], (len(bam) << 16) | 0xffff)
    assert got["n"] == ref["n"] and got["status"] == ref["status"] == 0
    for k in ("ref_id", "pos", "flag", "mapq", "bin", "l_seq", "next_ref_id", "next_pos", "tlen", "l_read_name",
              "n_cigar"):
        assert np.array_equal(got[k], ref[k]), k
    op = helpers.oracle_pools(ref)
    for k in ("names", "cigars", "seq", "qual"):
        assert np.array_equal(got[k], op[k]), k
    placed = ~(((ref["flag"] & 4) != 0) | (ref["ref_id"] < 0) | (ref["pos"] < -1))
    assert placed.any() and np.array_equal(got["key"][placed], ref["key"][placed])
    return ref


@pytest.mark.parametrize("name", GOLDEN_BAMS)
def test_golden_bam_rendered_as_sam(gpu_ctx, oracle_mod, name):
    """One split over the whole file: the fixed fields, names, CIGARs, SEQ, QUAL and the keys of
    placed records equal the oracle's decode of the BAM; the whole ubuf, every key and voffset equal
    the restatement."""
    bam = np.fromfile(os.path.join(GOLDEN, name), np.uint8)
    s = Sam(sam_cases.sam_of_bam(bam)[0])
    got = s.decode(gpu_ctx, 0, len(s.data))
    _against_oracle(got, bam, oracle_mod)
    same(got, s.whole, name)
    assert got["timing"]["comp_bytes"] == len(s.data) - s.data_start
    assert got["timing"]["ubuf_bytes"] == len(s.whole["ubuf"])


def _pool_bytes(cols):
    tot = {k: int(cols[k + "_off"][cols["n"]]) for k in ("name", "cigar", "seq", "aux")}
    return tot["name"] + 4 * tot["cigar"] + 2 * tot["seq"] + tot["aux"]


def test_timing_of_the_shared_record_tail(gpu_ctx, oracle_mod):
    """The BAM decode and the SAM decode end in one record tail: each call's timing keeps its own
    fields, and pool_bytes is the sum over the offsets that call returned."""
    bam = np.fromfile(os.path.join(GOLDEN, "small_pe.bam"), np.uint8)
    h = oracle_mod.read_header(bam)
    got = gpu_ctx.decode_split(bam, h["first_voffset"], (len(bam) << 16) | 0xffff, n_ref=h["n_ref"])
    assert got["rc"] == 0 and got["n"] > 0
    assert got["timing"]["pool_bytes"] == _pool_bytes(got) > 0
    assert got["timing"]["pools_ms"] > 0 and got["timing"]["n_records"] == got["n"]
    s = Sam(sam_cases.sam_of_bam(bam)[0])
    sam = s.decode(gpu_ctx, 0, len(s.data))
    assert sam["n"] == got["n"]
    t = sam["timing"]
    assert {k for k, v in t.items() if v} == {"scan_ms", "walk_ms", "inflate_ms", "huffman_ms", "resolve_ms", "decode_ms",
                                              "pools_ms", "total_ms", "comp_bytes", "ubuf_bytes", "n_records",
                                              "pool_bytes"}, t
    assert t["pool_bytes"] == _pool_bytes(sam) > 0 and t["n_records"] == sam["n"]


@pytest.mark.parametrize("variant", ["lf", "crlf"])
@pytest.mark.parametrize("size", [4096, 65537, 0])
def test_generated_file_in_splits(gpu_ctx, oracle_mod, generated, variant, size):
    """3000 records with unplaced and mate-unmapped reads: every split equals the restatement, and
    the splits' records concatenate to the single split's."""
    s = generated[variant]
    assert (s.whole["key"] >> 32 == 0x7fffffff).sum() + (s.whole["key"] < 0).sum() > 10
    if size == 0:
        got = s.decode(gpu_ctx, 0, len(s.data))
        _against_oracle(got, generated["bam"], oracle_mod)
        same(got, s.whole, variant)
        return
    ubuf, keys, voff = [], [], []
    for start, length in vcf_ref.file_splits(len(s.data), size):
        if 0 < start < s.data_start:
            continue  # (inside the header: its own test)
        got = s.decode(gpu_ctx, start, length)
        same(got, s.expect(start, length), (variant, size, start))
        ubuf.append(got["ubuf"])
        keys.append(got["key"])
        voff.append(got["voffset"])
    assert np.concatenate(ubuf).tobytes() == s.whole["ubuf"].tobytes()
    assert np.array_equal(np.concatenate(keys), s.whole["key"])
    assert np.array_equal(np.concatenate(voff), s.whole["voffset"])


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_crafted_lines(gpu_ctx, eol):
    """l_seq 0..65 and 3001, names of 1 and 254 bytes, 0 / 1 / 300 CIGAR ops, QUAL '*', lower case and
    '.', every RNEXT form, unknown names, every tag type and array subtype, the integer boundary
    values, floats at halfway points, 64 consecutive unplaced records; whole and in small splits."""
    s = Sam(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines(), eol))
    assert s.whole["status"] == 0 and s.whole["n"] == len(sam_cases.crafted_lines())
    got = s.decode(gpu_ctx, 0, len(s.data))
    same(got, s.whole, "whole")
    assert got["layout_ok"].all()
    tags = [r for r in s.whole["records"] if r[36:41] == b"tags\0"][0]
    aux = dict((t, v) for t, k, v in sam_ref.decode_aux(sam_ref.fields(tags)["aux"]) if k == "Bf")
    want = np.array([w for _, w in sam_cases.HALFWAY], np.float32).view(np.uint32)
    assert np.array_equal(np.array(aux[b"HF"], np.uint32), want)
    seen = 0
    for start, length in vcf_ref.file_splits(len(s.data), 257):
        if 0 < start < s.data_start:
            continue
        g = s.decode(gpu_ctx, start, length)
        same(g, s.expect(start, length), start)
        seen += g["n"]
    assert seen == s.whole["n"]


def _on_the_grid(ends, window_base, shift=0):
    """Every crafted line end lies one before, at or one after its boundary of the structural pass,
    whose grid starts `shift` bytes before the window's first byte."""
    got = sorted((b, (e - window_base + shift) % b) for b, e in ends)
    assert got == sorted((b, r) for b in sam_cases.BOUNDARIES for r in (0, 1, b - 1)), got


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_lines_ending_around_the_structural_boundaries(gpu_ctx, eol):
    """Line ends one before, at and one after a 16-byte, a 1 KiB and a 4 KiB boundary of the
    structural pass, in the three windows a caller can hand in: the reader's window for the split at
    0 (it begins at data_start; a host window is staged on a 16-byte boundary), the whole file as one
    window (text_base 0), and a device-resident window that begins 5 bytes past a 16-byte boundary
    (the grid starts at the boundary below it)."""
    import torch
    data, ends = sam_cases.boundary_file(eol)
    s = Sam(data)
    assert s.whole["n"] == 10 and s.whole["status"] == 0
    _on_the_grid(ends, s.data_start)
    same(s.decode(gpu_ctx, 0, len(data)), s.whole)
    for start, length in vcf_ref.file_splits(len(data), 1000):
        if start == 0 or start >= s.data_start:
            same(s.decode(gpu_ctx, start, length), s.expect(start, length), start)
    # the whole file as the window
    data, ends = sam_cases.boundary_file(eol, base=0)
    s = Sam(data)
    _on_the_grid(ends, 0)
    got = gpu_ctx.sam_decode_split(data, 0, len(data), s.data_start, s.table(gpu_ctx), s.n_ref)
    assert got["rc"] == 0
    same(got, s.whole, "text_base 0")
    # a device window 5 bytes past a 16-byte boundary: positions carry shift = 5
    data, ends = sam_cases.boundary_file(eol, base=-5)
    s = Sam(data)
    _on_the_grid(ends, 0, shift=5)
    t = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8), np.frombuffer(data, np.uint8),
                                         np.zeros(64, np.uint8)])).cuda()
    w = t[5:5 + len(data)]
    assert w.data_ptr() % 16 == 5
    rc, d = gpu_ctx.sam_decode_split_device(w, 0, len(data), s.data_start, s.table(gpu_ctx), s.n_ref)
    assert rc == 0 and d.status == 0 and d.n_records == 10
    r = gpu_ctx.records_to_host(d)
    assert r["ubuf"].tobytes() == s.whole["ubuf"].tobytes()
    assert np.array_equal(r["key"], s.whole["key"]) and np.array_equal(r["voffset"], s.whole["voffset"])


@pytest.mark.parametrize("case", sam_cases.error_cases(), ids=[c[0] for c in sam_cases.error_cases()])
def test_first_failing_line_ends_the_split(gpu_ctx, case):
    name, status, line = case
    for at in (0, 1, 65):
        s = Sam(sam_cases.error_file(line, at))
        assert s.whole["status"] == status and s.whole["n"] == at
        got = s.decode(gpu_ctx, 0, len(s.data))
        same(got, s.whole, (name, at))
        assert got["err_record"] == at


def test_split_that_begins_inside_the_header(gpu_ctx):
    s = Sam(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()[:20]))
    for start in (1, s.data_start - 1):
        r = gpu_ctx.sam_decode_split(s.data, start, 100, s.data_start, s.table(gpu_ctx), s.n_ref)
        assert r["rc"] == EUNSUPPORTED
    from hadoop_bam import FileSplit, SAMRecordReader, SAMUnsupportedException
    with pytest.raises(SAMUnsupportedException):
        SAMRecordReader().initialize(FileSplit("x.sam", 5, 100), data=s.data)
    # a split that begins exactly at data_start, and one at 0 that ends inside the header
    same(s.decode(gpu_ctx, s.data_start, 300), s.expect(s.data_start, 300))
    assert s.decode(gpu_ctx, 0, s.data_start)["n"] == 0


def test_window_over_two_gib_is_refused_before_anything_is_read(gpu_ctx):
    tab, size, names = gpu_ctx.vcf_contig_table(sam_cases.REF_NAMES)
    one = np.zeros(64, np.uint8)
    nm = np.frombuffer(names, np.uint8)
    from hadoop_bam import _lib
    d = _lib.Columns()
    rc = gpu_ctx.L.hbam_sam_decode_split(gpu_ctx.h, C.c_void_p(one.ctypes.data), 0, 0, (1 << 31) + 1, 1 << 32, 0,
                                         1 << 32, 0, C.cast(tab, C.c_void_p), size, C.c_void_p(nm.ctypes.data),
                                         len(names), 4, C.byref(d))
    assert rc == EINVAL and "2 GiB" in gpu_ctx.last_error()


def test_window_cut_inside_the_last_line(gpu_ctx, monkeypatch):
    s = Sam(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()[:40]))
    table = s.table(gpu_ctx)
    off = [int(o) for o in s.whole["voffset"]]
    for cut in (off[30] + 5, off[30] + 1, off[30]):  # inside line 30, and exactly at its first byte
        r = gpu_ctx.sam_decode_split(s.data[:cut], 0, len(s.data), s.data_start, table, s.n_ref,
                                     file_len=len(s.data))
        assert r["rc"] == 0 and r["status"] == EMORE, cut
        assert r["n"] == 30  # lines 0..29 are whole; what follows is withheld, an empty remainder too
        assert r["ubuf"].tobytes() == b"".join(s.whole["records"][:r["n"]])
    from hadoop_bam import sam
    monkeypatch.setattr(sam, "SAM_WINDOW_TAIL", 16)  # the reader's growth recovers from it
    for start, length in ((0, off[20] + 1), (off[10], off[25] - off[10]), (off[39] - 3, 2)):
        same(s.decode(gpu_ctx, start, length), s.expect(start, length), start)


def test_splits_at_and_past_the_end(gpu_ctx):
    s = Sam(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()[:10]))
    n = len(s.data)
    for start, length in ((n, 100), (n + 10, 100), (n - 1, 1), (n - 1, 50)):
        got = s.decode(gpu_ctx, start, length)
        assert got["n"] == 0 and got["status"] == 0, start
    last = int(s.whole["voffset"][-1])
    assert s.decode(gpu_ctx, last, 1)["n"] == 1


def test_device_window_that_does_not_start_on_16_bytes(gpu_ctx):
    import torch
    s = Sam(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()))
    for lead in (3, 13):
        # (64 readable bytes behind the window, as include/hbam.h asks: no padded copy is made)
        t = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), np.frombuffer(s.data, np.uint8),
                                             np.zeros(64, np.uint8)])).cuda()
        w = t[lead:lead + len(s.data)]
        assert w.data_ptr() % 16 == lead
        rc, d = gpu_ctx.sam_decode_split_device(w, 0, len(s.data), s.data_start, s.table(gpu_ctx), s.n_ref)
        assert rc == 0 and d.status == 0 and d.n_records == s.whole["n"]
        r = gpu_ctx.records_to_host(d)
        assert r["ubuf"].tobytes() == s.whole["ubuf"].tobytes()  # hbam_records_to_host: exactly the ubuf
        assert np.array_equal(r["key"], s.whole["key"]) and np.array_equal(r["voffset"], s.whole["voffset"])
        # a window that begins inside the file, at the reader's first byte
        o = int(s.whole["voffset"][40])
        rc, d = gpu_ctx.sam_decode_split_device(w[o - 1:], o, 2000, s.data_start, s.table(gpu_ctx), s.n_ref,
                                                text_base=o - 1, file_len=len(s.data))
        assert rc == 0
        e = s.expect(o, 2000)
        r = gpu_ctx.records_to_host(d)
        assert r["n"] == e["n"] > 0 and r["ubuf"].tobytes() == e["ubuf"].tobytes()


def _read_all(fmt, splits, conf=None):
    from hadoop_bam import SAMRecordReader
    out = []
    for sp in splits:
        rr = fmt.createRecordReader(sp, conf)
        assert 0.0 <= rr.getProgress() <= 1.0
        while rr.nextKeyValue():
            out.append((int(rr.getCurrentKey().get()), rr.getCurrentValue().get().toBAMBytes()))
        assert rr.getProgress() == 1.0 or not isinstance(rr, SAMRecordReader)
        rr.close()
    return out


def test_input_format_and_readers_over_a_file(gpu_ctx, tmp_path):
    from hadoop_bam import SAMInputFormat, SAMRecordReader
    s = Sam(sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines(), b"\r\n", last_eol=False))
    path = str(tmp_path / "reads.sam")
    open(path, "wb").write(s.data)
    fmt = SAMInputFormat()
    splits = fmt.getSplits(path, 3000)
    assert len(splits) > 3 and fmt.isSplitable()
    splits = [sp for sp in splits if sp.getStart() == 0 or sp.getStart() >= s.data_start]
    assert isinstance(fmt.createRecordReader(splits[0]), SAMRecordReader)
    got = _read_all(fmt, splits)
    assert [k for k, _ in got] == [int(k) for k in s.whole["key"]]
    assert [b for _, b in got] == s.whole["records"]


def test_any_sam_input_format_on_sam_and_bam_paths(gpu_ctx, genbam, tmp_path):
    """A placed-only file as .sam and as .bam yields the same keys and records (the BAM's integer tag
    widths made canonical by one pass through the restatement)."""
    from hadoop_bam import AnySAMInputFormat, FileSplit, FileVirtualSplit
    bam = np.asarray(genbam.generate(records=500, seed=3, unplaced_permille=0, mate_unmapped_permille=0))
    text, h = sam_cases.sam_of_bam(bam)
    sp, bp = str(tmp_path / "reads.sam"), str(tmp_path / "reads.bam")
    open(sp, "wb").write(text)
    bam.tofile(bp)
    fmt = AnySAMInputFormat()
    ss = fmt.getSplits([FileSplit(sp, 0, len(text))])
    bs = fmt.getSplits([FileSplit(bp, 0, len(bam))])
    assert isinstance(ss[0], FileSplit) and isinstance(bs[0], FileVirtualSplit)
    a, b = _read_all(fmt, ss), _read_all(fmt, bs)
    names = [n for n, _ in h.refs]
    dic = {n: i for i, n in enumerate(names)}
    canon = [sam_ref.parse_encode(line, dic) for line in sam_ref.render([r for _, r in b], names)]
    assert len(a) == len(b) == 500
    assert [k for k, _ in a] == [k for k, _ in b]
    assert [r for _, r in a] == canon


def test_sam_through_sort_and_the_bam_writer(gpu_ctx, genbam, tmp_path):
    """SAM -> sam_decode_split_device -> HipSortOps.run_from_columns -> BAMRecordWriter gives the
    records, in the order, of the same pipeline fed the same records as BAM (placed reads: the keys
    coincide; integer tag widths canonical beforehand)."""
    import torch
    from hadoop_bam import sort
    from hadoop_bam.output import BAMRecordWriter, EMPTY_GZIP_BLOCK
    src = np.asarray(genbam.generate(records=2000, seed=11, unplaced_permille=0, mate_unmapped_permille=0))
    text, h = sam_cases.sam_of_bam(src)
    s = Sam(text)
    assert s.whole["status"] == 0 and s.whole["n"] == 2000
    bam = np.frombuffer(helpers.bgzf_pack(h.to_bam_bytes() + s.whole["ubuf"].tobytes()), np.uint8)
    ops = sort.HipSortOps(gpu_ctx)

    def write(run, name):
        path = str(tmp_path / name)
        w = BAMRecordWriter(path, h, True, gpu_ctx)
        w.write_device(run.payload, int(run.offsets[-1].item()))
        w.close()
        with open(path, "ab") as f:
            f.write(EMPTY_GZIP_BLOCK)
        out = np.fromfile(path, np.uint8)
        hd = gpu_ctx.parse_header(out)
        return gpu_ctx.decode_split(out, hd["first_voffset"], (len(out) << 16) | 0xffff, n_ref=hd["n_ref"])

    rc, d = gpu_ctx.sam_decode_split_device(torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda(), 0,
                                            len(text), s.data_start, s.table(gpu_ctx), s.n_ref)
    assert rc == 0 and d.status == 0 and d.n_records == 2000
    assert gpu_ctx.records_to_host(d)["ubuf"].tobytes() == s.whole["ubuf"].tobytes()
    from_sam = write(ops.run_from_columns(d), "from_sam.bam")
    hb = gpu_ctx.parse_header(bam)
    rc, d = gpu_ctx.decode_split_device(torch.from_numpy(bam.copy()).cuda(), hb["first_voffset"],
                                        (len(bam) << 16) | 0xffff, hb["n_ref"])
    assert rc == 0 and d.status == 0 and d.n_records == 2000
    from_bam = write(ops.run_from_columns(d), "from_bam.bam")
    assert from_sam["n"] == from_bam["n"] == 2000 and from_sam["status"] == from_bam["status"] == 0
    assert np.array_equal(from_sam["key"], from_bam["key"]) and (np.diff(from_sam["key"]) >= 0).all()
    assert from_sam["ubuf"].tobytes() == from_bam["ubuf"].tobytes()
    order = np.argsort(s.whole["key"], kind="stable")
    assert from_sam["ubuf"].tobytes()[-sum(len(s.whole["records"][i]) for i in order):] == \
        b"".join(s.whole["records"][i] for i in order)
