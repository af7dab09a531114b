"""SAM text input, CPU side: the tests' restatement (tests/sam_ref.py) round-trips the golden BAMs,
its split rule partitions a file, its float rounding and integer widths follow the rules of
include/hbam.h, and the host classes of hadoop_bam.sam parse headers and formats."""
import os
import random
import struct
from fractions import Fraction

import numpy as np
import pytest

import bai_ref
import sam_cases
import sam_ref
import vcf_ref
from conftest import GOLDEN

GOLDEN_BAMS = ["small_pe.bam", "edge_uniform_long.bam", "edge_unsorted_l1.bam"]


def test_import_exports_the_sam_classes():
    import hadoop_bam
    assert hadoop_bam.SAMInputFormat and hadoop_bam.SAMRecordReader and hadoop_bam.SAMFormat
    assert hadoop_bam.read_sam_text_header


@pytest.mark.parametrize("name", GOLDEN_BAMS)
def test_render_then_parse_encode_round_trips_every_record(name):
    """parse_encode(render(r)) against r for every record: the fixed fields, name, CIGAR, SEQ and
    QUAL byte for byte, the aux as (tag, value) pairs (the files' integer widths need not be the
    narrowest), bin against bai_ref's region-to-bin."""
    h, recs = sam_cases.bam_header_and_records(np.fromfile(os.path.join(GOLDEN, name), np.uint8))
    names = [n for n, _ in h.refs]
    dic = {n: i for i, n in enumerate(names)}
    lines = sam_ref.render(recs, names)
    assert len(lines) == len(recs) > 0
    for r, line in zip(recs, lines):
        e = sam_ref.parse_encode(line, dic)
        assert not isinstance(e, int), (e, line[:100])
        a, b = sam_ref.fields(r), sam_ref.fields(e)
        for k in ("ref", "pos", "l_read_name", "mapq", "n_cigar", "flag", "l_seq", "nref", "npos", "tlen", "name",
                  "cigar", "seq", "qual"):
            assert a[k] == b[k], (k, line[:100])
        assert sam_ref.decode_aux(a["aux"]) == sam_ref.decode_aux(b["aux"])
        reflen = sum(w >> 4 for w in b["cigar"] if (w & 15) in (0, 2, 3, 7, 8))
        end = 0 if b["flag"] & 4 else b["pos"] + reflen
        if end <= 0:
            end = b["pos"] + 1
        assert b["bin"] == bai_ref.reg2bin(b["pos"], end) & 0xffff


def _partition_file(eol, last_eol):
    return sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()[:60], eol, last_eol)


@pytest.mark.parametrize("eol,last_eol", [(b"\n", True), (b"\r\n", True), (b"\n", False)])
@pytest.mark.parametrize("size", [61, 64, 257, 4096, 0])
def test_splits_partition_the_lines(size, eol, last_eol):
    """The union of the splits' lines is every line, each exactly once."""
    data = _partition_file(eol, last_eol)
    whole = sam_ref.all_lines(data)
    assert len(whole) == 60 and whole[0][0] == sam_ref.data_start(data)
    got = []
    for start, length in vcf_ref.file_splits(len(data), size or len(data)):
        got += sam_ref.read_split(data, start, length)
    assert got == whole
    assert sam_ref.read_split(data, 0, sam_ref.data_start(data)) == []  # the documented divergence
    assert sam_ref.read_split(data, len(data), 100) == []


def _nearest_is(value, bits):
    """bits is the float32 nearest to the Fraction `value`, a tie going to the even mantissa."""
    def f(b):
        m, e = (b & 0x7fffff) | 0x800000, ((b >> 23) & 0xff) - 150
        return Fraction(m) * Fraction(2) ** e
    mag = bits & 0x7fffffff
    d = abs(abs(value) - f(mag))
    for other in (mag - 1, mag + 1):
        do = abs(abs(value) - f(other))
        if do < d or (do == d and (mag & 1)):
            return False
    return True


def test_float_rounding_at_halfway_points():
    for text, want in sam_cases.HALFWAY:
        bits = sam_ref.float32_bits(text)
        assert bits == struct.unpack("<I", struct.pack("<f", want))[0], text
    rng = random.Random(3)
    for _ in range(3000):  # in the domain: the result is the nearest float32, by exact comparison
        digits = rng.randint(1, 9)
        m = rng.randint(10 ** (digits - 1), 10 ** digits - 1)
        point = rng.randint(0, digits)
        exp = rng.randint(-20 + point, 20 + point - (0 if m % 10 else 9))
        s = str(m)
        text = ("%s.%se%d" % (s[:digits - point], s[digits - point:], exp)).encode()
        bits = sam_ref.float32_bits(text)
        e = exp - point
        if bits is None:
            t = m
            while t % 10 == 0:
                t //= 10
                e += 1
            assert not -20 <= e <= 20, text
            continue
        assert _nearest_is(Fraction(m) * Fraction(10) ** e, bits), text
    for text in (b"1.234567891", b"1e21", b"1e-21", b"nan", b"inf", b"0x10", b"1e", b".", b"", b"1.2.3", b"--1"):
        assert sam_ref.float32_bits(text) is None, text
    assert sam_ref.float32_bits(b"-0.0") == 0x80000000 and sam_ref.float32_bits(b"0e99") == 0


def test_integer_tag_widths():
    for v, t in zip(sam_cases.INT_BOUNDS, sam_cases.INT_TYPES):
        ty, raw = sam_ref.int_tag(v)
        assert ty == t, v
        rec = sam_ref.parse_encode(sam_cases.good_line(1) + b"\tXX:i:%d" % v, sam_cases.DICT)
        assert rec.endswith(b"XX" + t.encode() + raw)
        assert sam_ref.decode_aux(b"XX" + t.encode() + raw) == [(b"XX", "i", v)]


def test_error_cases_have_their_status():
    for name, status, line in sam_cases.error_cases():
        assert sam_ref.parse_encode(line, sam_cases.DICT) == status, name
    assert all(not isinstance(sam_ref.parse_encode(x, sam_cases.DICT), int) for x in sam_cases.crafted_lines())


def test_key_chain_is_seeded():
    """The key of an unplaced line chains the four hashes through their seeds; a placed one is
    ref << 32 | pos."""
    lines = sam_cases.crafted_lines()
    placed = sam_ref.parse_line(lines[14], sam_cases.DICT)
    assert sam_ref.key(placed) == placed["ref"] << 32 | placed["pos"]
    p = sam_ref.parse_line([x for x in lines if x.startswith(b"unpl07")][0], sam_cases.DICT)
    k = sam_ref.key(p)
    assert k >> 32 in (0x7fffffff, -1)  # the low int is sign-extended over the high one
    from hadoop_bam.formats import murmurhash3_bytes, murmurhash3_chars, _i32
    h = _i32(murmurhash3_chars(p["name"].decode(), 0))
    h = _i32(murmurhash3_bytes(p["bases"], h))
    h = _i32(murmurhash3_bytes(p["quals"], h))
    h = _i32(murmurhash3_chars("*", h))
    assert k & 0xffffffff == h & 0xffffffff
    rng = np.random.default_rng(1)
    for n in list(range(0, 36)) + [200]:
        b = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        for seed in (0, 5, -9):
            assert sam_ref.murmur_bytes(b, seed) == murmurhash3_bytes(b, seed)


def test_sam_format_and_text_header(tmp_path):
    from hadoop_bam import AnySAMInputFormat, Configuration, SAMFormat, read_sam_text_header
    assert SAMFormat.inferFromFilePath("/x/a.bam") == "BAM" and SAMFormat.inferFromFilePath("a.sam") == "SAM"
    assert SAMFormat.inferFromFilePath("a.txt") is None
    assert SAMFormat.inferFromData(b"\x1f\x8b") == "BAM" and SAMFormat.inferFromData(b"@HD") == "SAM"
    assert SAMFormat.inferFromData(b"r1\t0") is None
    data = sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines()[:5], b"\r\n")
    text, data_start, header = read_sam_text_header(data)
    assert data_start == sam_ref.data_start(data) and text == data[:data_start]
    assert header.refs == sam_cases.REFS
    # a header longer than the first prefix read, and a file that is only a header
    big = [b"@CO\t" + b"x" * 1000] * 100
    data2 = sam_ref.sam_file(sam_cases.HEADER + big, [b"r"])
    assert read_sam_text_header(data2)[1] == len(data2) - 2
    only = sam_ref.sam_file(sam_cases.HEADER, [])
    assert read_sam_text_header(only)[1] == len(only)
    p = tmp_path / "lying.sam"
    p.write_bytes(b"\x1f\x8b")
    assert AnySAMInputFormat().getFormat(str(p)) == "SAM"
    assert AnySAMInputFormat().getFormat(str(p), Configuration({"hadoopbam.anysam.trust-exts": "false"})) == "BAM"


def test_device_line_rules_on_the_cpu_match_the_restatement(tmp_path):
    """csrc/sam_line.h is host-and-device C++: tools/sam_line_host.cpp, a stand-alone program built
    here with the address and undefined-behaviour sanitizers, runs every line through the rules the
    kernels run (both passes, SEQ and QUAL unit by unit, the seeded byte hash) and must give the
    status and the record bytes of the restatement: a golden BAM rendered as SAM, the crafted lines,
    every error case, the boundary files, and a zero written with more than 10,000 digits."""
    import subprocess
    root = os.path.dirname(GOLDEN[:-len("/golden")])
    exe = str(tmp_path / "sam_line_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "hadoop-bam_amd", "csrc"),
                    "-o", exe, os.path.join(root, "tools", "sam_line_host.cpp")], check=True)
    zero = sam_cases.good_line(5) + b"\tZF:f:-0." + b"0" * 10500 + b"e7\tZG:f:" + b"0" * 10500 + b"\tZH:f:0e123456"
    late = sam_cases.good_line(6) + b"\tZF:f:0." + b"0" * 10500 + b"1"  # out of the domain
    files = {
        "golden": sam_cases.sam_of_bam(np.fromfile(os.path.join(GOLDEN, "edge_unsorted_l1.bam"), np.uint8))[0],
        "crafted": sam_ref.sam_file(sam_cases.HEADER, sam_cases.crafted_lines() + [zero, late] +
                                    [c[2] for c in sam_cases.error_cases()], b"\r\n", last_eol=False),
        "boundary": sam_cases.boundary_file()[0],
    }
    assert sam_ref.parse_encode(late, sam_cases.DICT) == sam_ref.HBAM_EUNSUPPORTED
    assert sam_ref.decode_aux(sam_ref.fields(sam_ref.parse_encode(zero, sam_cases.DICT))["aux"])[-3:] == [
        (b"ZF", "f", 0x80000000), (b"ZG", "f", 0), (b"ZH", "f", 0)]
    for name, data in files.items():
        src, out = str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bin"))
        with open(src, "wb") as f:
            f.write(data)
        subprocess.run([exe, src, out], check=True)
        got = open(out, "rb").read()
        dic, p = sam_ref.dictionary(data), 0
        lines = sam_ref.all_lines(data)
        assert len(lines) > 5
        for off, line in lines:
            st, sz, mh = struct.unpack_from("<iIq", got, p)
            rec = got[p + 16:p + 16 + sz]
            p += 16 + sz
            want = sam_ref.parse_encode(line, dic)
            assert mh == sam_ref.murmur_bytes(line, -7), (name, off)
            if isinstance(want, int):
                assert st == want and sz == 0, (name, off, st, want, line[:80])
            else:
                assert st == 0 and rec == want, (name, off, st, line[:80])
        assert p == len(got)
