"""The FASTA restatement (tests/fasta_ref.py) against the hand-derived fixture and against itself
(the closed-form tail rule equals the Text model; LineReader's buffer size does not matter), and
the host classes of hadoop_bam.fasta that need no device."""
import random

import pytest

import fasta_cases as cases
import fasta_ref as ref


def test_fixture_splits():
    assert ref.get_splits(cases.FIXTURE) == cases.FIXTURE_SPLITS
    assert ref.get_splits(b"") == [(0, 0)]
    assert ref.get_splits(b"ACGT\nAC\n") == [(0, 8)]
    assert ref.get_splits(b"AC\n>a >b\nAC\n>c") == [(3, 2), (6, 5), (12, 2)]  # bytes before the first '>': no split
    # FileInputFormat's own splits of the file change nothing
    assert ref.get_splits(cases.FIXTURE, [(0, 10), (10, 10), (20, 14)]) == cases.FIXTURE_SPLITS


@pytest.mark.parametrize("split", sorted(cases.FIXTURE_EXPECTED))
def test_fixture_records(split):
    want = cases.FIXTURE_EXPECTED[split]
    got = ref.run_fasta(cases.FIXTURE, *split)
    assert got["status"] == ref.OK
    assert (got["first_pos"], got["end_pos"], got["index"]) == (want["first_pos"], want["end_pos"], want["index"])
    assert [(r["key"], r["position"], r["seq"]) for r in got["records"]] == want["records"]
    if "line_len" in want:
        assert [r["line_len"] for r in got["records"]] == want["line_len"]


def stored_lines(data, start, res):
    """The stored header line and the data lines of a run, from the file's own bytes."""
    head = data[start:start + 1 + len(res["index"])]
    return [head] + [data[r["rec_off"]:r["rec_off"] + r["line_len"]] for r in res["records"]]


def test_tail_rule_is_the_per_byte_definition():
    """Byte c of record k past its own length is byte c of the largest j in [-1, k) with L_j > c."""
    rnd = random.Random(5)
    for _ in range(40):
        lines = [cases.line_bytes(k - 1, rnd.randrange(1 if k == 0 else 0, 25)) for k in range(rnd.randrange(2, 60))]
        want, cap = [], len(lines[0])
        for k in range(1, len(lines)):
            cap = max(cap, len(lines[k]))
            seq = bytearray(lines[k])
            for c in range(len(lines[k]), cap):
                seq.append(next(lines[j][c] for j in range(k - 1, -1, -1) if len(lines[j]) > c))
            want.append(bytes(seq))
        assert ref.tail_rule(lines) == want


def test_tail_rule_equals_the_text_model_on_random_lengths():
    rnd = random.Random(11)
    for trial in range(60):
        hdr = rnd.randrange(1, 40)
        top = rnd.choice((3, 20, 80))
        lens = [rnd.randrange(0, top) for _ in range(rnd.randrange(1, 200))]
        data = cases.profile(hdr, lens, rnd.choice((b"\n", b"\r", b"\r\n")))
        res = ref.run_fasta(data, 0, len(data))
        assert res["status"] == ref.OK and res["n"] == len(lens)
        assert [r["line_len"] for r in res["records"]] == lens
        assert [r["seq"] for r in res["records"]] == ref.tail_rule(stored_lines(data, 0, res)), trial
        assert all(b != 0 for r in res["records"] for b in r["seq"])


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_crafted_cases_tail_rule_and_buffer_size(case):
    """Every crafted case: the Text model gives the closed form, and the same records whatever
    LineReader's buffer size (a 1-byte buffer cuts every line at every byte, CRLF included)."""
    data, start, length = cases.case_range(case)
    res = ref.run_fasta(data, start, length)
    if res["index"] is not None:
        assert [r["seq"] for r in res["records"]] == ref.tail_rule(stored_lines(data, start, res))
    sizes = (1, 2, 7) if len(data) < 3000 else (7,)
    for size in sizes:
        assert ref.run_fasta(data, start, length, buffer_size=size) == res, size


def test_buffer_size_on_the_fixture_and_the_sweep_file():
    for data in (cases.FIXTURE, cases.SWEEP):
        for start, length in [(0, len(data))] + ref.get_splits(data):
            want = ref.run_fasta(data, start, length, buffer_size=65536)
            for size in (1, 2, 7):
                assert ref.run_fasta(data, start, length, buffer_size=size) == want, (start, size)


def test_expected_statuses_of_the_crafted_cases():
    by_id = {c[0]: c for c in cases.CASES}

    def run(name):
        return ref.run_fasta(*cases.case_range(by_id[name]))
    for name in ("header-stored-0-empty-line", "header-stored-0-length-0", "header-stored-0-end-of-file"):
        assert (run(name)["status"], run(name)["n"]) == (ref.EINDEX, 0), name
    assert run("header-byte-0x80")["status"] == ref.EUNSUPPORTED
    assert run("header-byte-0x80-behind-the-cut")["status"] == ref.OK
    assert run("header-stored-1")["index"] == b"" and run("header-stored-1")["records"][0]["key"] == b"1"
    cut = run("header-cut-by-the-split")
    assert (cut["index"], cut["first_pos"], cut["n"]) == (b"chr1", 23, 0)
    assert run("split-ends-behind-the-header")["n"] == 1
    big = run("header-20500")
    assert len(big["index"]) == 19999 and big["status"] == ref.OK and len(big["records"][1]["seq"]) == 20000
    assert (run("line-consumes-19999")["status"], run("line-consumes-19999")["n"]) == (ref.OK, 3)
    over = run("line-consumes-20000")
    assert (over["status"], over["n"], over["err_pos"], over["end_pos"]) == (ref.ERUNTIME, 2, 10, 20010)
    assert run("line-consumes-20001-crlf")["status"] == ref.ERUNTIME
    assert run("line-consumes-20000-unterminated")["status"] == ref.ERUNTIME
    assert run("gt-inside-the-header")["index"] == b"b c"


def test_compressed_path_of_the_restatement():
    assert ref.run_fasta(b">h\nAC\n", 0, 1, compressed=True)["status"] == ref.ENULL
    assert ref.run_fasta(b"\n", 0, 1, compressed=True)["status"] == ref.ENULL
    empty = ref.run_fasta(b"", 0, 1, compressed=True)
    assert (empty["status"], empty["n"], empty["end_pos"]) == (ref.OK, 0, 0)
    assert ref.run_fasta(b"A" * 20000, 0, 1, compressed=True)["status"] == ref.ERUNTIME


def test_reference_fragment():
    from hadoop_bam import ReferenceFragment
    from hadoop_bam.formats import IllegalArgumentException
    f = ReferenceFragment()
    assert (f.getSequence(), f.getPosition(), f.getIndexSequence()) == (b"", None, None)
    assert f.toString() == "null\tnull\t"
    f.setSequence(b"ACGT")
    f.setPosition(8)
    f.setIndexSequence("chr1 desc\tx")
    assert f.toString() == "chr1 desc\tx\t8\tACGT" == str(f)
    g = ReferenceFragment()
    assert f != g and not g.equals(None)
    g.setSequence(b"ACGT")
    g.setPosition(8)
    g.setIndexSequence("chr1 desc\tx")
    assert f == g and f.equals(g)
    g.setPosition(9)
    assert f != g
    for setter in (f.setSequence, f.setPosition, f.setIndexSequence):
        with pytest.raises(IllegalArgumentException):
            setter(None)
    f.clear()
    assert (f.getSequence(), f.getPosition(), f.getIndexSequence()) == (b"", None, None)


def test_input_format_without_a_device(tmp_path):
    import gzip
    from hadoop_bam import FastaInputFormat, FileSplit, fasta, formats
    informat = FastaInputFormat()
    assert informat.isSplitable(None, "ref.fa") and not informat.isSplitable(None, "ref.fa.gz")
    assert FastaInputFormat.FastaRecordReader.MAX_LINE_LENGTH == 20000
    with pytest.raises(formats.IOException):
        informat.getSplits(["a.fa", "b.fa"], data=b">a\nAC\n")
    # a .gz file never reaches the device: no header line is read, the first line raises
    path = str(tmp_path / "ref.fa.gz")
    with open(path, "wb") as f:
        f.write(gzip.compress(cases.FIXTURE))
    reader = informat.createRecordReader(FileSplit(path, 0, 5), {})
    assert reader.getPos() == 0 and reader.getProgress() < 1e-9
    with pytest.raises(formats.NullPointerException):
        reader.nextKeyValue()
    assert reader.getPos() == 13
    with pytest.raises(fasta.RuntimeException):
        informat.createRecordReader(FileSplit(path, 3, 5), {})
    empty = str(tmp_path / "empty.fa.gz")
    with open(empty, "wb") as f:
        f.write(gzip.compress(b""))
    reader = informat.createRecordReader(FileSplit(empty, 0, 5), {})
    assert reader.nextKeyValue() is False and reader.getPos() == 0
    big = str(tmp_path / "big.fa.gz")
    with open(big, "wb") as f:
        f.write(gzip.compress(b"A" * 19999 + b"\nAC\n"))
    with pytest.raises(fasta.RuntimeException):
        informat.createRecordReader(FileSplit(big, 0, 5), {}).next()
