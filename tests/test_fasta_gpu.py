"""FASTA on the device (hbam_fasta.hip through Context.fasta_decode_split / fasta_sections and
hadoop_bam.fasta) against the hand-derived fixture and the tests' restatement (tests/fasta_ref.py).
The device is never compared with itself."""
import gzip

import numpy as np
import pytest

import fasta_cases as cases
import fasta_ref as ref

pytestmark = pytest.mark.gpu


def as_result(cols, window):
    """Host columns of one device call -> the restatement's result form."""
    assert cols["rc"] == 0, cols
    out = {k: cols[k] for k in ("n", "status", "first_pos", "end_pos", "err_pos")}
    o, n = cols["index_off"], cols["index_len"]
    out["index"] = bytes(window[o:o + n])
    recs = []
    for i in range(cols["n"]):
        r = {"rec_off": int(cols["rec_off"][i]), "pos_after": int(cols["pos_after"][i]),
             "position": int(cols["position"][i]), "line_len": int(cols["line_len"][i])}
        for k in ("key", "seq"):
            r[k] = cols[k][int(cols[k + "_off"][i]):int(cols[k + "_off"][i + 1])].tobytes()
        recs.append(r)
    out["records"] = recs
    assert int(cols["key_off"][0]) == 0 and int(cols["seq_off"][0]) == 0
    assert int(cols["key_off"][-1]) == len(cols["key"]) and int(cols["seq_off"][-1]) == len(cols["seq"])
    return out


def device_window(data, base, stop, shift=0):
    """Device memory that holds data[base:stop] at `shift` bytes past a 16-byte boundary, inside an
    allocation with 64 bytes behind it."""
    import torch
    t = torch.zeros(shift + (stop - base) + 64 + 16, dtype=torch.uint8, device="cuda")
    off = (-t.data_ptr()) % 16 + shift
    if stop > base:
        t[off:off + stop - base] = torch.frombuffer(bytearray(data[base:stop]), dtype=torch.uint8).cuda()
    arg = t[off:off + stop - base]
    assert arg.data_ptr() % 16 == shift % 16
    return arg


def device_run(ctx, data, start, length, window_end=None, shift=None):
    """One device call over the window [start, window_end or the end of the file); shift: the window
    is device memory that begins `shift` bytes past a 16-byte boundary."""
    base = min(start, len(data))
    stop = len(data) if window_end is None else window_end
    window = bytes(data[base:stop])
    # (an empty device tensor has no address: an empty window is passed as host bytes)
    arg = window if shift is None or not window else device_window(data, base, stop, shift)
    cols = ctx.fasta_decode_split(arg, start, length, text_base=base, file_len=len(data))
    return as_result(cols, window)


def assert_same(dev, want, what):
    """Every column, both pools, the positions and the status."""
    assert dev["status"] == want["status"], (what, dev["status"], want["status"])
    assert dev["n"] == want["n"], (what, dev["n"], want["n"])
    assert dev["first_pos"] == want["first_pos"], (what, dev["first_pos"], want["first_pos"])
    if want["index"] is not None:
        assert dev["index"] == want["index"], (what, dev["index"], want["index"])
        assert dev["end_pos"] == want["end_pos"], (what, dev["end_pos"], want["end_pos"])
    if want["err_pos"] is not None:
        assert dev["err_pos"] == want["err_pos"], (what, dev["err_pos"], want["err_pos"])
    for i, (d, w) in enumerate(zip(dev["records"], want["records"])):
        for k in ("rec_off", "pos_after", "position", "line_len", "key", "seq"):
            assert d[k] == w[k], (what, i, k, d[k], w[k])


@pytest.fixture(scope="module")
def expected():
    """The restatement's answer for every crafted case, computed once."""
    return {c[0]: ref.run_fasta(*cases.case_range(c)) for c in cases.CASES}


@pytest.mark.parametrize("split", sorted(cases.FIXTURE_EXPECTED))
def test_hand_derived_fixture(gpu_ctx, split):
    want = cases.FIXTURE_EXPECTED[split]
    got = device_run(gpu_ctx, cases.FIXTURE, *split)
    assert got["status"] == ref.OK
    assert (got["first_pos"], got["end_pos"], got["index"]) == (want["first_pos"], want["end_pos"], want["index"])
    assert [(r["key"], r["position"], r["seq"]) for r in got["records"]] == want["records"]
    if "line_len" in want:
        assert [r["line_len"] for r in got["records"]] == want["line_len"]


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_crafted_cases(gpu_ctx, expected, case):
    data, start, length = cases.case_range(case)
    want = expected[case[0]]
    assert_same(device_run(gpu_ctx, data, start, length), want, "host window")
    assert_same(device_run(gpu_ctx, data, start, length, shift=5), want, "device window")


def test_split_sweep(gpu_ctx):
    """Every start of the three-section file with three lengths each (about 450 device calls)."""
    data = cases.SWEEP
    assert len(ref.get_splits(data)) == 3
    splits = cases.sweep_splits(data)
    assert len(splits) <= 500
    for start, length in splits:
        assert_same(device_run(gpu_ctx, data, start, length), ref.run_fasta(data, start, length), (start, length))


def test_window_cut_inside_the_last_line_read(gpu_ctx):
    data = cases.SWEEP
    want = ref.run_fasta(data, 0, 35)
    assert want["n"] == 2 and want["end_pos"] == 42  # "GGGTTTAAAC\r\n" starts at 30, below the split's end
    for cut in (36, 40, 41):  # inside the line, before its CR, and behind it (undecidable: LF may follow)
        dev = device_run(gpu_ctx, data, 0, 35, window_end=cut)
        assert dev["status"] == ref.EMORE, cut
        dev = device_run(gpu_ctx, data, 0, 35, window_end=cut, shift=3)
        assert dev["status"] == ref.EMORE, cut
    for cut in (42, 60, len(data)):  # the line's LF is inside: enough, the retry matches
        assert_same(device_run(gpu_ctx, data, 0, 35, window_end=cut), want, cut)
        assert_same(device_run(gpu_ctx, data, 0, 35, window_end=cut, shift=3), want, cut)
    # a window that ends inside the header line
    assert device_run(gpu_ctx, data, 0, 35, window_end=10)["status"] == ref.EMORE
    # a CR as the window's last byte, and as the file's
    cr = b">h\rACGT\rAC\r"
    assert device_run(gpu_ctx, cr, 0, len(cr), window_end=8)["status"] == ref.EMORE
    assert_same(device_run(gpu_ctx, cr, 0, len(cr)), ref.run_fasta(cr, 0, len(cr)), "file ends in CR")
    assert_same(device_run(gpu_ctx, cr, 0, 5, window_end=9), ref.run_fasta(cr, 0, 5), "CR inside the window")


@pytest.mark.parametrize("shift", range(18))
def test_device_window_at_any_alignment(gpu_ctx, shift):
    data = cases.profile(7, [(k * 7) % 23 for k in range(300)], b"\r\n")
    want = ref.run_fasta(data, 0, len(data))
    assert_same(device_run(gpu_ctx, data, 0, len(data), shift=shift), want, shift)
    assert_same(device_run(gpu_ctx, cases.FIXTURE, 23, 11, shift=shift), ref.run_fasta(cases.FIXTURE, 23, 11), shift)


def sections(ctx, data, base=0, shift=None):
    arg = bytes(data) if shift is None else device_window(data, 0, len(data), shift)
    res = ctx.fasta_sections(arg, text_base=base)
    assert res["rc"] == 0, res
    return res["offsets"]


def test_sections_against_flatnonzero(gpu_ctx):
    n = 9001
    text = np.full(n, ord("A"), np.uint8)
    text[::61] = ord("\n")
    at = [0, 15, 16, 17, 1023, 1024, 4095, 4096, n - 1]
    text[at] = ord(">")
    files = {"boundaries": text.tobytes(), "none": b"ACGT\n" * 900, "all": b">" * 5000, "empty": b"",
             "one-byte": b">", "fixture": cases.FIXTURE, "sweep": cases.SWEEP}
    for name, data in files.items():
        want = np.flatnonzero(np.frombuffer(data, np.uint8) == ord(">")).astype(np.uint64)
        if name == "boundaries":
            assert list(want) == at
        got = sections(gpu_ctx, data)
        assert got.dtype == np.uint64 and np.array_equal(got, want), name
        assert np.array_equal(sections(gpu_ctx, data, base=1 << 33), want + np.uint64(1 << 33)), name
        for shift in (1, 15, 17) if data else ():
            assert np.array_equal(sections(gpu_ctx, data, shift=shift), want), (name, shift)


def test_sections_capacity_query(gpu_ctx):
    import ctypes as C
    from hadoop_bam import _lib
    data = np.frombuffer(cases.SWEEP, np.uint8)
    out = np.full(4, 77, np.uint64)
    cnt = C.c_uint64(0)
    call = gpu_ctx.L.hbam_fasta_sections
    rc = call(gpu_ctx.h, C.c_void_p(data.ctypes.data), 0, 0, len(data), C.c_void_p(out.ctypes.data), 2, C.byref(cnt))
    assert rc == _lib.HBAM_EMORE and cnt.value == 3 and list(out) == [77] * 4  # nothing written
    rc = call(gpu_ctx.h, C.c_void_p(data.ctypes.data), 0, 0, len(data), C.c_void_p(out.ctypes.data), 3, C.byref(cnt))
    assert rc == 0 and cnt.value == 3 and list(out[:3]) == [s for s, _ in ref.get_splits(cases.SWEEP)] and out[3] == 77


def test_get_splits_through_the_input_format(gpu_ctx, tmp_path, monkeypatch):
    from hadoop_bam import FastaInputFormat, FileSplit, fasta
    informat = FastaInputFormat()
    for name, data in (("fixture.fa", cases.FIXTURE), ("sweep.fa", cases.SWEEP), ("plain.fa", b"ACGT\nAC\n"),
                       ("empty.fa", b""), ("gt-in-header.fa", b"AC\n>a >b\nAC\n>c")):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        got = informat.getSplits([path])
        assert [(s.getStart(), s.getLength()) for s in got] == ref.get_splits(data), name
        assert all(s.getPath() == path for s in got)
        # FileInputFormat's own splits of the file, and windows smaller than the file
        monkeypatch.setattr(fasta, "SECTION_WINDOW", 16)
        third = len(data) // 3
        orig = [FileSplit(path, 0, third), FileSplit(path, third, len(data) - third)]
        got = informat.getSplits(orig)
        assert [(s.getStart(), s.getLength()) for s in got] == ref.get_splits(data), name
        monkeypatch.undo()
    assert [(s.getStart(), s.getLength()) for s in informat.getSplits("x.fa", data=cases.FIXTURE)] == cases.FIXTURE_SPLITS
    with pytest.raises(fasta.IOException):
        informat.getSplits([str(tmp_path / "fixture.fa"), str(tmp_path / "sweep.fa")])


def test_reader_surface(gpu_ctx, tmp_path):
    from hadoop_bam import FastaInputFormat, FileSplit, ReferenceFragment
    path = str(tmp_path / "fixture.fa")
    with open(path, "wb") as f:
        f.write(cases.FIXTURE)
    informat = FastaInputFormat()
    splits = informat.getSplits(path)
    reader = informat.createRecordReader(splits[0], {})
    assert isinstance(reader, FastaInputFormat.FastaRecordReader)
    assert reader.getPos() == 13 and reader.getProgress() == 0.0
    assert reader.makePositionMessage() == "%s:13" % path and reader.makePositionMessage(7) == "%s:7" % path
    assert reader.createKey() == "" and isinstance(reader.createValue(), ReferenceFragment)
    assert reader.nextKeyValue()
    assert reader.getCurrentKey() == "chr1 desc:x1"
    v = reader.getCurrentValue()
    assert (v.getIndexSequence(), v.getPosition(), v.getSequence()) == ("chr1 desc\tx", 1, b"ACGTACdesc\tx")
    assert v.toString() == "chr1 desc\tx\t1\tACGTACdesc\tx"
    assert reader.getPos() == 20
    assert reader.getProgress() == float(np.float32(7) / np.float32(9))  # (pos - start) / (end - start), start moved
    assert reader.next()
    assert (reader.getCurrentKey(), reader.getCurrentValue().getSequence()) == ("chr1 desc:x8", b"GGGTACdesc\tx")
    assert reader.getPos() == 23 and reader.getProgress() == 1.0
    assert reader.nextKeyValue() is False and reader.nextKeyValue() is False
    reader.close()
    # every split of getSplits through the reader against the restatement
    for s in splits:
        want = ref.run_fasta(cases.FIXTURE, s.getStart(), s.getLength())
        reader = informat.createRecordReader(s, {})
        got = []
        while reader.nextKeyValue():
            v = reader.getCurrentValue()
            got.append((reader.getCurrentKey().encode(), v.getPosition(), v.getSequence(), reader.getPos()))
        assert got == [(r["key"], r["position"], r["seq"], r["pos_after"]) for r in want["records"]] and got


def test_reader_exceptions_and_growing_window(gpu_ctx, expected, monkeypatch):
    from hadoop_bam import fasta
    by_id = {c[0]: c for c in cases.CASES}

    def reader(name):
        data, start, length = cases.case_range(by_id[name])
        return fasta.FastaRecordReader({}, fasta.FileSplit(name + ".fa", start, length), data=data)
    with pytest.raises(IndexError):
        reader("header-stored-0-empty-line")
    with pytest.raises(fasta.SeqUnsupportedException):
        reader("header-byte-0x80")
    r = reader("line-consumes-20000")
    assert r.next() and r.next()
    with pytest.raises(fasta.RuntimeException):
        r.next()
    assert r.getPos() == expected["line-consumes-20000"]["end_pos"]
    # the window starts with a 16-byte tail and grows x4 on HBAM_EMORE
    monkeypatch.setattr(fasta, "SEQ_WINDOW_TAIL", 16)
    data = cases.profile(9, [60] * 40 + [13])
    want = ref.run_fasta(data, 0, 700)
    r = fasta.FastaRecordReader({}, fasta.FileSplit("gen.fa", 0, 700), data=data)
    got = []
    while r.nextKeyValue():
        got.append((r.getCurrentKey().encode(), r.getCurrentValue().getSequence(), r.getPos()))
    assert got == [(x["key"], x["seq"], x["pos_after"]) for x in want["records"]] and got


def test_columns_stay_on_the_device(gpu_ctx):
    """read_split_columns_device: the pools are device arrays of the context."""
    import torch  # noqa: F401
    from hadoop_bam import fasta, _lib
    from hadoop_bam.formats import SeekableFile
    data = cases.profile(9, [60] * 40 + [13])
    d, base, window = fasta.read_split_columns_device(gpu_ctx, SeekableFile(data), 0, len(data))
    want = ref.run_fasta(data, 0, len(data))
    assert (int(d.n), int(d.status), int(d.host), base) == (want["n"], _lib.HBAM_OK, 0, 0)
    seq = np.zeros(int(d.seq_len), np.uint8)
    assert gpu_ctx.L.hbam_download(gpu_ctx.h, d.seq, int(d.seq_len), seq.ctypes.data) == 0
    assert seq.tobytes() == b"".join(r["seq"] for r in want["records"])


def test_gz_through_the_input_format(gpu_ctx, tmp_path):
    from hadoop_bam import FastaInputFormat, FileSplit, formats
    informat = FastaInputFormat()
    path = str(tmp_path / "ref.fa.gz")
    with open(path, "wb") as f:
        f.write(gzip.compress(cases.FIXTURE))
    assert ref.run_fasta(cases.FIXTURE, 0, 1, compressed=True)["status"] == ref.ENULL
    reader = informat.createRecordReader(FileSplit(path, 0, 1), {})
    with pytest.raises(formats.NullPointerException):
        reader.nextKeyValue()
    empty = str(tmp_path / "empty.fa.gz")
    with open(empty, "wb") as f:
        f.write(gzip.compress(b""))
    assert informat.createRecordReader(FileSplit(empty, 0, 1), {}).nextKeyValue() is False
