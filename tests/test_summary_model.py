"""The summarize reduce and SummarySort, CPU side: the Python reading of the Java
(tests/summary_ref.py) against every crafted case's declaration (tests/summary_cases.py), coverage
assertions that the listed edges really occur in the cases, and summarize()'s LEVELS validation and
file naming, which touch no device."""
import importlib
import os

import pytest

import summary_cases as SC
import summary_ref as R

reading = SC.reading


def sorted_lines(lines):
    """SummarySort over one stream's text, by the reader's reading."""
    return R.summary_sort(R.stream_text(lines)).decode().splitlines()


@pytest.mark.parametrize("case", SC.REDUCER_CASES, ids=repr)
def test_reading_matches_hand_written_lines(case):
    r = reading(case)
    assert R.stream_names(case.levels) == [n for l in case.levels for n in ("summary%sf" % l, "summary%sr" % l)]
    assert sorted(R.stream_names(case.levels)) == sorted(r.outputs)
    if case.want is not None:
        assert r.outputs == case.want
    if case.want_sorted is not None:
        assert {k: sorted_lines(v) for k, v in r.outputs.items()} == case.want_sorted
    # every range is summarized exactly once per level and strand
    for i, l in enumerate(case.levels):
        for rev in (0, 1):
            lines = r.outputs[R.get_summary_name(l, bool(rev))]
            assert sum(int(x.split("\t")[3]) for x in lines) == sum(1 for v in case.rev if v == rev)


def test_level_one_is_the_ranges_themselves():
    case = [c for c in SC.REDUCER_CASES if c.name == "random_n257"][0]
    r = reading(case)
    order = sorted(range(len(case.key)), key=lambda i: case.key[i])
    for rev, name in ((0, "summary1f"), (1, "summary1r")):
        got = [tuple(int(x) for x in l.split("\t")[1:]) for l in r.outputs[name]]
        assert got == [(case.beg[i], case.end[i], 1) for i in order if case.rev[i] == rev]


def test_reducer_cases_cover_the_listed_edges():
    names = {c.name for c in SC.REDUCER_CASES}
    assert {"random_n%d" % n for n in (0, 1, 63, 64, 65, 255, 256, 257)} <= names
    big = [c for c in SC.REDUCER_CASES if len(c.key) >= 70000]
    assert big and set(big[0].levels) == {"1", "2", "3", "64", "100000"}
    levels = {int(l) for c in SC.REDUCER_CASES for l in c.levels}
    assert {1, 2147483647} <= levels
    r = reading(big[0])
    spans = [s for v in r.spans.values() for s in v]
    # groups straddle a wave (64), a workgroup (256), a scan tile (4096) and the sort's tile edges
    for edge in (64, 256, 4096, 65536):
        assert any(a < edge <= b for a, b in spans), edge
    # several segments, the rid = -1 one included, and segments that straddle those edges too
    rids = [R._i32((k & 0xffffffffffffffff) >> 32) for k in sorted(big[0].key)]
    assert rids[0] == -1 and len(set(rids)) == 5
    change = [i for i in range(1, len(rids)) if rids[i] != rids[i - 1]]
    assert len(change) == 4 and any(c % 256 for c in change)
    # equal keys occur, on both strands and across a group boundary of level 2
    keys = sorted(big[0].key)
    assert any(keys[i] == keys[i + 1] for i in range(len(keys) - 1))
    # a level larger than every segment, and one dividing a segment exactly
    c = [c for c in SC.REDUCER_CASES if c.name == "level_sizes"][0]
    assert all(x.endswith("\t2") for x in reading(c).outputs["summary2f"])
    assert len(reading(c).outputs["summary100f"]) == 1
    # a sum past 2^32, a negative inexact quotient
    sums = [s for c in SC.REDUCER_CASES for v in reading(c).sums.values() for s in v]
    assert any(sb >= 1 << 32 for sb, _ in sums)
    tr = reading([c for c in SC.REDUCER_CASES if c.name == "negative_truncation"][0])
    assert tr.sums["summary2r"] == [(-9, -7)] and (-9) % 2 and (-7) % 2
    # every rendered width
    text = "\n".join(x for c in SC.REDUCER_CASES if c.name == "rendered_values"
                     for v in reading(c).outputs.values() for x in v)
    fields = set(text.replace("\n", "\t").split("\t"))
    assert {"-2147483648", "-1", "0", "9", "10", "2147483647"} <= fields
    # a partial group flushed at a segment change is written with the next segment's rid
    ts = reading([c for c in SC.REDUCER_CASES if c.name == "three_segments"][0])
    assert ts.outputs["summary2r"] == ["1\t300\t310\t1"]
    # --sort changes some stream's order, and some stream has a negative beg
    sd = reading([c for c in SC.REDUCER_CASES if c.name == "sort_differs"][0])
    assert sorted_lines(sd.outputs["summary1f"]) != sd.outputs["summary1f"]
    assert any(int(x.split("\t")[1]) < 0 for x in sd.outputs["summary1f"])


@pytest.mark.parametrize("case", SC.LINE_CASES, ids=repr)
def test_line_reading_matches_the_declaration(case):
    lines, keys, status = R.summary_keys(case.data)
    assert status == case.status
    if case.n is not None:
        assert len(lines) == case.n
    if case.keys is not None:
        assert keys == case.keys
    assert all(b"\r" not in l and b"\n" not in l for l in lines)
    assert R.gathered(lines).count(b"\n") == len(lines)


def test_line_cases_cover_the_listed_edges():
    d = [c for c in SC.LINE_CASES if c.name == "edges"][0].data
    assert d[15:16] == b"\n" and d[31:33] == b"\r\n" and d[47:48] == b"\r" and d[48:49] != b"\n"
    assert d[1023:1025] == b"\r\n" and d[4095:4097] == b"\r\n"
    assert d[8191:8192] == b"\r" and d[8192:8193] != b"\n" and d[12287:12288] == b"\n"
    assert not d.endswith((b"\n", b"\r"))
    lines, keys, status = R.summary_keys(d)
    assert status == 0 and len(lines) == 68 and len(set(keys)) == len(keys)
    late = [c for c in SC.LINE_CASES if c.name == "late_error"][0]
    assert late.n >= 4 * 256  # the first error lies in a later workgroup than the clean prefix
    assert R.summary_keys(late.data.split(b"1\t5\n", 1)[1])[2] == R.ENUMBER  # a second, different error follows
    statuses = {c.status for c in SC.LINE_CASES}
    assert statuses == {0, R.EINDEX, R.ENUMBER}
    mixed = [c for c in SC.LINE_CASES if c.name == "mixed_terminators"][0]
    assert R.gathered(*R.summary_keys(mixed.data)[:2]) == b"0\t1\t1\t1\n0\t3\t4\t1\n0\t5\t6\t1\n0\t9\t2\t1\n"
    neg = [c for c in SC.LINE_CASES if c.name == "negative_pos_sorts_first"][0]
    assert R.summary_sort(neg.data) == b"1\t-3\t6\t1\n0\t9\t9\t1\n1\t5\t6\t1\n"


def test_key0_sign_extension():
    assert R.get_key0(2, -7) == -7
    assert R.get_key0(1, 5) == (1 << 32) | 5
    assert R.get_key0(-1, 5) == -(1 << 32) + 5
    assert R.range_key(2, -10, -4) == -7
    assert R.centre_of_mass(-5, -4) == -4  # truncation, not floor


# ---- summarize(): LEVELS and file names (no device) ---------------------------------------------
def test_parse_levels_messages():
    S = importlib.import_module("hadoop_bam.summarize")  # (the package exports the function under that name)
    assert S.parse_levels("1,16,1000") == (["1", "16", "1000"], [1, 16, 1000])
    with pytest.raises(ValueError, match="summary level 'x' is not an integer!"):
        S.parse_levels("1,x")
    with pytest.raises(ValueError, match="summary level '' is not an integer!"):
        S.parse_levels("1,,2")
    with pytest.raises(ValueError, match="summary level '2147483648' is not an integer!"):
        S.parse_levels("2147483648")
    with pytest.raises(ValueError, match="summary level '0' is not positive!"):
        S.parse_levels("4,0")
    with pytest.raises(ValueError, match="summary level '-3' is not positive!"):
        S.parse_levels("-3")
    with pytest.raises(ValueError, match="already"):
        S.parse_levels("5,7,5")
    with pytest.raises(ValueError, match="Named output name"):
        S.parse_levels("+5")  # Integer.parseInt takes it, MultipleOutputs does not
    assert S.parse_levels("2147483647")[1] == [2147483647]


def test_summarize_validates_levels_before_anything_else(tmp_path):
    S = importlib.import_module("hadoop_bam.summarize")  # (the package exports the function under that name)
    with pytest.raises(ValueError, match="not positive"):
        S.summarize(str(tmp_path / "w"), "1,0", str(tmp_path / "missing.bam"))
    assert not os.path.exists(tmp_path / "w")


def test_output_names():
    S = importlib.import_module("hadoop_bam.summarize")  # (the package exports the function under that name)
    assert S.getSummaryName("16", False) == "summary16f" and S.getSummaryName("16", True) == "summary16r"
    got = S.output_paths("/w", ["1", "16"], "/data/in.bam", "/o")
    assert got == ["/o/in.bam-summary1f", "/o/in.bam-summary1r", "/o/in.bam-summary16f", "/o/in.bam-summary16r"]
    got = S.output_paths("/w", ["7"], "/data/in.bam")
    assert got == ["/w/in.bam-summary7f-000000", "/w/in.bam-summary7r-000000"]


def test_summary_group_and_exports():
    import hadoop_bam
    g = hadoop_bam.SummaryGroup(16, "summary16f")
    g.sumBeg, g.count = 5, 2
    g.reset()
    assert (g.level, g.outName, g.sumBeg, g.sumEnd, g.count) == (16, "summary16f", 0, 0, 0)
    for name in ("SummarizeReducer", "SummarizeOutputFormat", "getSummaryName", "summarize", "summary_sort"):
        assert hasattr(hadoop_bam, name)
