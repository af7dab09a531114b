"""The summarize reduce, SummarySort's reader and writer, and the two plugins end to end on the
device: hbam_summarize_reduce, hbam_summary_keys and hbam_summary_gather_lines against the Python
reading of the Java (tests/summary_ref.py) on every crafted case (tests/summary_cases.py), and
summarize() / summary_sort() on the golden BAM.  Exact bytes everywhere."""
import collections
import importlib
import os
import struct

import numpy as np
import pytest

import summary_cases as SC
import summary_ref as R
from conftest import GOLDEN
from helpers import bam_stream, bgzf_members, bgzf_pack

pytestmark = pytest.mark.gpu

TERMINATOR = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _S():
    return importlib.import_module("hadoop_bam.summarize")  # (the package exports the function under that name)


def _expected(case, sort):
    """first / columns / text / text_off of a reducer case from the reading."""
    r = SC.reading(case)
    first, text_off, cols, text = [0], [0], [], b""
    for name in R.stream_names(case.levels):
        lines = r.outputs[name]
        t = R.stream_text(lines)
        if sort:
            t = R.summary_sort(t)
        cols += [tuple(int(x) for x in l.split(b"\t")) for l in t.splitlines()]
        text += t
        first.append(len(cols))
        text_off.append(len(text))
    c = np.asarray(cols, np.int64).reshape(-1, 4)
    return first, c, text, text_off


@pytest.mark.parametrize("sort", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("case", SC.REDUCER_CASES, ids=repr)
def test_reduce_case(gpu_ctx, case, sort):
    got = gpu_ctx.summarize_reduce(*case.arrays(), case.level_values(), sort_output=sort)
    first, cols, text, text_off = _expected(case, sort)
    assert got["first"].tolist() == first
    for j, k in enumerate(("rid", "beg", "end", "count")):
        assert np.array_equal(got[k], cols[:, j]), k
    assert got["text_off"].tolist() == text_off
    assert got["text"] == text
    assert got["timing"]["n_records"] == len(case.key)


def test_reduce_is_reproducible(gpu_ctx):
    case = [c for c in SC.REDUCER_CASES if c.name == "random_n70001"][0]
    a = gpu_ctx.summarize_reduce(*case.arrays(), case.level_values(), sort_output=True)
    b = gpu_ctx.summarize_reduce(*case.arrays(), case.level_values(), sort_output=True)
    assert a["text"] == b["text"] and a["first"].tolist() == b["first"].tolist()


def test_reduce_rejects_bad_levels(gpu_ctx):
    case = SC.REDUCER_CASES[0]
    for lv in ([], [0], [4, -1]):
        with pytest.raises(RuntimeError, match="hbam_summarize_reduce failed"):
            gpu_ctx.summarize_reduce(*case.arrays(), lv)


def test_reducer_class_mirror(gpu_ctx):
    """The reference's stateful API over the device call: setup, reduce per key, cleanup."""
    from hadoop_bam import consumers
    S = _S()
    case = [c for c in SC.REDUCER_CASES if c.name == "three_segments"][0]
    red = S.SummarizeReducer()
    red.setup(",".join(case.levels))
    for key, vals in R.shuffle(case.key, case.beg, case.end, case.rev):
        red.reduce(key, [consumers.Range(b, e, bool(r)) for b, e, r in vals])
    red.cleanup()
    for name, lines in case.want.items():
        assert red.outputs[name] == R.stream_text(lines)
    rc = red.rangeCounts("summary2r")
    assert [str(x) for x in rc] == case.want["summary2r"]


def test_output_format_writes_members_without_a_terminator(gpu_ctx, tmp_path):
    """SummarizeOutputFormat: RangeCount lines through the device compressor, flushed, not closed."""
    from hadoop_bam import consumers
    S = _S()
    w = S.SummarizeOutputFormat().getRecordWriter(str(tmp_path / "part"))
    vals = [consumers.RangeCount(consumers.Range(10 * i, 10 * i + 5), 3, i % 2 - 1) for i in range(9000)]
    for v in vals:
        w.write(None, v)
    w.close()
    data = (tmp_path / "part").read_bytes()
    assert not data.endswith(TERMINATOR)
    members = bgzf_members(data)
    assert len(members) > 1 and all(ok and isz == len(u) and isz > 0 for u, isz, ok, _ in members)
    assert b"".join(m[0] for m in members) == b"".join(b"%d\t%d\t%d\t3\n" % (i % 2 - 1, 10 * i, 10 * i + 5)
                                                       for i in range(9000))


@pytest.mark.parametrize("case", SC.LINE_CASES, ids=repr)
def test_summary_keys_case(gpu_ctx, case):
    lines, keys, status = R.summary_keys(case.data)
    got = gpu_ctx.summary_keys(case.data)
    assert got["n"] == len(lines) and got["status"] == status == case.status
    assert got["key"].tolist() == keys
    for i, l in enumerate(lines):
        s, n = int(got["start"][i]), int(got["len"][i])
        assert case.data[s:s + n] == l
    assert got["lines"] == R.gathered(lines)
    if status == 0:
        assert gpu_ctx.summary_keys(case.data, sort=True)["lines"] == R.gathered(lines, keys)


def test_summary_keys_device_text_at_an_odd_address(gpu_ctx):
    """A device-resident window that does not start on a 16-byte boundary."""
    from hadoop_bam import _lib
    case = [c for c in SC.LINE_CASES if c.name == "edges"][0]
    buf = gpu_ctx.upload(b"xxxxx" + case.data)
    try:
        view = _lib.DeviceBuffer(gpu_ctx, buf.ptr + 5, len(case.data), False)
        got = gpu_ctx.summary_keys(view, sort=True)
    finally:
        buf.free()
    lines, keys, _ = R.summary_keys(case.data)
    assert got["n"] == len(lines) and got["key"].tolist() == keys
    assert got["lines"] == R.gathered(lines, keys)


# ---- the plugins on the golden BAM --------------------------------------------------------------
LEVELS = ["1", "16", "1000"]


def _inflate(path, terminated=True):
    data = open(path, "rb").read()
    if terminated:
        assert data.endswith(TERMINATOR)
    members = bgzf_members(data)
    for u, isz, crc_ok, bs in members:
        assert crc_ok and isz == len(u) and bs <= 65536
    if terminated:
        assert members[-1][1] == 0
    return b"".join(m[0] for m in members)


def _without_rangeless_records(data):
    """A copy of a BAM without the mapped records whose CIGAR has no M / = / X base: on those
    SummarizeRecordReader raises IndexOutOfBoundsException (ranges.get(0), Summarize.java:715)."""
    u = bam_stream(data)
    p = 8 + struct.unpack_from("<i", u, 4)[0]
    n = struct.unpack_from("<i", u, p)[0]
    p += 4
    for _ in range(n):
        p += 8 + struct.unpack_from("<i", u, p)[0]
    out, dropped = [u[:p]], 0
    while p + 4 <= len(u):
        bs = struct.unpack_from("<i", u, p)[0]
        r = u[p:p + 4 + bs]
        p += 4 + bs
        ref, pos = struct.unpack_from("<ii", r, 4)
        nc, flag = struct.unpack_from("<HH", r, 16)
        if not flag & 4 and ref >= 0 and pos + 1 >= 0:
            cig = struct.unpack_from("<%dI" % nc, r, 36 + r[12])
            if not any((c & 15) in (0, 7, 8) and c >> 4 for c in cig):
                dropped += 1
                continue
        out.append(r)
    return bgzf_pack(b"".join(out)), dropped


# The golden small_pe.bam holds mapped records without a single aligned base (its generator's odd
# records): the reference's job FAILS on it (test_summarize_fails_on_the_golden_bam_as_the_reference_does).
# The file checks therefore run on that BAM without those 26 records, under the same file name (19,974
# records over several splits and windows), and on the unsorted golden BAM, where the shuffle's order
# differs from the file's.
INPUTS = ["small_pe.bam", "edge_unsorted_l1.bam"]


@pytest.fixture(scope="module")
def golden_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inputs")
    clean, dropped = _without_rangeless_records(np.fromfile(os.path.join(GOLDEN, "small_pe.bam"), np.uint8))
    assert 0 < dropped < 100
    (d / "small_pe.bam").write_bytes(clean)
    return {"small_pe.bam": str(d / "small_pe.bam"),
            "edge_unsorted_l1.bam": os.path.join(GOLDEN, "edge_unsorted_l1.bam")}


@pytest.fixture(scope="module")
def golden_ranges(oracle_mod, golden_inputs):
    """oracle.summarize_ranges over each whole input: the map output in input order."""
    o, out = oracle_mod, {}
    for name, path in golden_inputs.items():
        data = np.fromfile(path, np.uint8)
        h = o.read_header(data)
        ref = o.read_split(data, h["first_voffset"], (len(data) << 16) | 0xffff)
        pay, off = o.record_payloads(ref)
        r = o.summarize_ranges(pay, off, ref["status"])
        assert r["status"] == 0 and len(r["key"]) > 5000
        out[name] = r
    assert any(np.any(np.diff(r["key"]) < 0) for r in out.values())  # some input is not in key order
    return out


@pytest.fixture(scope="module")
def golden_reading(golden_ranges):
    return {name: R.run_reducer(g["key"].tolist(), g["beg"].tolist(), g["end"].tolist(), g["rev"].tolist(), LEVELS)
            for name, g in golden_ranges.items()}


@pytest.fixture(scope="module")
def golden_run(tmp_path_factory, golden_inputs):
    """summarize() on each input over several splits and windows: unsorted and sorted, merged."""
    from hadoop_bam import formats
    S = _S()
    d = tmp_path_factory.mktemp("summarize")
    conf = formats.Configuration({S.SPLIT_SIZE_PROPERTY: 400_000, formats.WINDOW_BYTES_PROPERTY: 300_000})
    out = {"dir": d}
    for name, path in golden_inputs.items():
        for sort in (False, True):
            w, o = str(d / ("w%d%s" % (sort, name))), str(d / ("o%d%s" % (sort, name)))
            out[name, sort] = S.summarize(w, ",".join(LEVELS), path, o, sort=sort, conf=conf)
            out[name, sort]["work_dir"] = w
            print("summarize(sort=%s) on %s: %d ranges, %d lines, device ms %s"
                  % (sort, name, out[name, sort]["n_ranges"], out[name, sort]["n_lines"], out[name, sort]["timing"]))
    return out


@pytest.mark.parametrize("sort", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("name", INPUTS)
def test_summarize_golden(golden_run, golden_reading, golden_ranges, name, sort):
    res, ranges, read = golden_run[name, sort], golden_ranges[name], golden_reading[name]
    assert [os.path.basename(p) for p in res["files"]] == [name + "-" + n for n in R.stream_names(LEVELS)]
    assert res["n_ranges"] == len(ranges["key"])
    for p, stream in zip(res["files"], R.stream_names(LEVELS)):
        want = R.stream_text(read.outputs[stream])
        if sort:
            want = R.summary_sort(want)
        assert _inflate(p) == want, stream
    for rev, stream in ((0, "summary1f"), (1, "summary1r")):
        p = res["files"][R.stream_names(LEVELS).index(stream)]
        assert _inflate(p).count(b"\n") == int(np.sum(ranges["rev"] == rev))
    assert not os.listdir(res["work_dir"])  # -o: nothing stays in the work directory


def test_summarize_fails_on_the_golden_bam_as_the_reference_does(oracle_mod, tmp_path):
    """tests/golden/small_pe.bam itself: record 1054 is mapped and has no aligned base, so
    SummarizeRecordReader.nextKeyValue raises IndexOutOfBoundsException there (the oracle's status
    after 1,097 ranges) and the reference's job fails; summarize() raises the same and writes nothing."""
    from hadoop_bam import consumers
    o = oracle_mod
    data = np.fromfile(os.path.join(GOLDEN, "small_pe.bam"), np.uint8)
    h = o.read_header(data)
    ref = o.read_split(data, h["first_voffset"], (len(data) << 16) | 0xffff)
    pay, off = o.record_payloads(ref)
    assert o.summarize_ranges(pay, off, ref["status"])["status"] == R.EINDEX
    with pytest.raises(consumers.IndexOutOfBoundsException):
        _S().summarize(str(tmp_path / "w"), ",".join(LEVELS), os.path.join(GOLDEN, "small_pe.bam"), str(tmp_path / "o"))
    assert not os.path.exists(tmp_path / "w") and not os.path.exists(tmp_path / "o")


def test_summarize_leaves_parts_in_the_work_dir(golden_inputs, golden_reading, tmp_path):
    from hadoop_bam import formats
    S = _S()
    conf = formats.Configuration()  # one split, one window
    res = S.summarize(str(tmp_path), "16", golden_inputs["small_pe.bam"], conf=conf)
    assert sorted(os.listdir(tmp_path)) == ["small_pe.bam-summary16f-000000", "small_pe.bam-summary16r-000000"]
    for p, name in zip(res["files"], ("summary16f", "summary16r")):
        assert not open(p, "rb").read().endswith(TERMINATOR)
        assert _inflate(p, terminated=False) == R.stream_text(golden_reading["small_pe.bam"].outputs[name])


def test_summary_sort_equals_the_sort_leg(golden_run, tmp_path):
    S = _S()
    files = {srt: [p for name in INPUTS for p in golden_run[name, srt]["files"]] for srt in (False, True)}
    for k, (unsorted, srt) in enumerate(zip(files[False], files[True])):
        out = str(tmp_path / ("sorted%d" % k))
        res = S.summary_sort(str(tmp_path / "w"), unsorted, out)
        assert _inflate(out) == _inflate(srt)
        assert res["n"] == _inflate(unsorted).count(b"\n")
    # without an output path: the part, named after the input, no terminator
    res = S.summary_sort(str(tmp_path / "w"), files[False][2])
    assert res["file"] == str(tmp_path / "w" / "small_pe.bam-summary16f-000000")
    assert _inflate(res["file"], terminated=False) == _inflate(files[True][2])


def test_summary_sort_of_a_shuffled_file(golden_run, tmp_path):
    """Unique keys (ties dropped), shuffled, CRLF terminators: sorts back to the same bytes."""
    S = _S()
    lines, keys, status = R.summary_keys(_inflate(golden_run["small_pe.bam", True]["files"][0]))
    assert status == 0
    seen = collections.Counter(keys)
    uniq = [l for l, k in zip(lines, keys) if seen[k] == 1][:3000]
    assert len(uniq) > 1000
    order = np.random.RandomState(5).permutation(len(uniq))
    shuffled = b"".join(uniq[i] + b"\r\n" for i in order)
    src = tmp_path / "shuffled-summary1f"
    src.write_bytes(bgzf_pack(shuffled))
    out = str(tmp_path / "out")
    S.summary_sort(str(tmp_path), str(src), out)
    assert _inflate(out) == b"".join(l + b"\n" for l in uniq)


def test_summary_sort_raises_on_a_bad_line(tmp_path):
    from hadoop_bam import consumers, formats
    S = _S()
    for text, exc in ((b"0\t1\t2\t1\n3\t5\n", consumers.IndexOutOfBoundsException),
                      (b"0\t1\t2\t1\n0\tx\t2\t1\n", formats.NumberFormatException)):
        src = tmp_path / "bad"
        src.write_bytes(bgzf_pack(text))
        with pytest.raises(exc):
            S.summary_sort(str(tmp_path / "w"), str(src), str(tmp_path / "out"))
        assert not os.path.exists(tmp_path / "out") and not os.path.exists(tmp_path / "w")


def _rewritten_bam(edit, keep=120):
    """The golden BAM's header and first `keep` records, each passed through edit(i, record bytes)."""
    u = bam_stream(np.fromfile(os.path.join(GOLDEN, "small_pe.bam"), np.uint8))
    p = 8 + struct.unpack_from("<i", u, 4)[0]
    n = struct.unpack_from("<i", u, p)[0]
    p += 4
    for _ in range(n):
        p += 8 + struct.unpack_from("<i", u, p)[0]
    out = [u[:p]]
    for i in range(keep):
        bs = struct.unpack_from("<i", u, p)[0]
        out.append(bytes(edit(i, bytearray(u[p:p + 4 + bs]))))
        p += 4 + bs
    return bgzf_pack(b"".join(out))


def test_summarize_without_a_mapped_record(tmp_path):
    S = _S()

    def unmap(i, r):
        struct.pack_into("<H", r, 18, struct.unpack_from("<H", r, 18)[0] | 4)
        return r
    bam = tmp_path / "unmapped.bam"
    bam.write_bytes(_rewritten_bam(unmap))
    res = S.summarize(str(tmp_path / "w"), "1,16", str(bam), str(tmp_path / "o"), sort=True)
    assert res["n_ranges"] == 0 and len(res["files"]) == 4
    for p in res["files"]:
        assert open(p, "rb").read() == TERMINATOR


def test_summarize_raises_when_a_reader_fails(tmp_path):
    """A mapped record with a CIGAR op code above 8: SummarizeRecordReader raises
    IllegalArgumentException after the ranges before it; the job fails and writes nothing."""
    from hadoop_bam import formats
    S = _S()
    hit = []

    def bad_op(i, r):
        flag, ref, nc = struct.unpack_from("<H", r, 18)[0], struct.unpack_from("<i", r, 4)[0], struct.unpack_from("<H", r, 16)[0]
        if i >= 60 and not hit and not flag & 4 and ref >= 0 and nc:
            r[36 + r[12]] |= 15
            hit.append(i)
        return r
    bam = tmp_path / "badop.bam"
    bam.write_bytes(_rewritten_bam(bad_op))
    assert hit
    with pytest.raises(formats.IllegalArgumentException):
        S.summarize(str(tmp_path / "w"), "1,16", str(bam), str(tmp_path / "o"))
    assert not os.path.exists(tmp_path / "w") and not os.path.exists(tmp_path / "o")
