"""Text VCF without a GPU: the tests' restatement (tests/vcf_ref.py) against the reference's fixture
(tests/golden/test.vcf = the reference's src/test/resources/test.vcf, what TestVCFInputFormat
reads), the format dispatch and the host-side header parse."""
import os

import pytest

import vcf_ref
from conftest import GOLDEN

FIXTURE_KEYS = [14369, 17329, 1110695, 1230236, 1234566]


@pytest.fixture(scope="module")
def fixture_vcf():
    data = open(os.path.join(GOLDEN, "test.vcf"), "rb").read()
    assert len(data) == 1645
    return data


def test_restatement_reads_the_reference_fixture(fixture_vcf):
    from hadoop_bam import vcf
    header, contig, data_start = vcf_ref.parse_header(fixture_vcf)
    assert contig == {b"20": 0} and fixture_vcf[data_start:data_start + 9] == b"20\t14370\t"
    assert vcf.read_vcf_header(fixture_vcf, "test.vcf") == (header, [b"20"], data_start)  # the product's parse
    r = vcf_ref.read_split(fixture_vcf, 0, len(fixture_vcf))
    assert r["n"] == 5 and r["status"] == 0
    assert r["key"] == FIXTURE_KEYS
    first = r["lines"][0].split(b"\t")
    assert first[0] == b"20" and first[1] == b"14370" and first[3] == b"G" and first[4] == b"A"
    second = r["lines"][1].split(b"\t")
    assert second[1] == b"17330" and second[3] == b"T" and second[4] == b"A"


def test_split_rule_loses_the_line_at_end_minus_one(fixture_vcf):
    """A line beginning exactly at start + length - 1 of a split with start != 0 is read by no split
    (the next split discards it as its incomplete line): the reference's behaviour."""
    assert vcf_ref.lost_lines(fixture_vcf, 77) == [1462]
    assert vcf_ref.lost_lines(fixture_vcf, 229) == [1144]
    assert vcf_ref.lost_lines(fixture_vcf, 311) == [1554]
    for size in (64, 512, 1645):
        assert vcf_ref.lost_lines(fixture_vcf, size) == []
    # the same over the splits the drop-in's getSplits hands out for a .vcf path
    from hadoop_bam import bcf
    fmt = bcf.VCFInputFormat()

    def splits(size):
        return [(s.getStart(), s.getLength()) for s in fmt.getSplits("test.vcf", size, data=fixture_vcf)]
    lossy = {size: vcf_ref.lost_lines(fixture_vcf, size, splits(size)) for size in range(60, 1646)}
    assert sorted(s for s, lost in lossy.items() if lost) == [77, 133, 209, 229, 251, 269, 311]
    assert all(len(lost) <= 1 for lost in lossy.values())


def test_two_murmur_restatements_agree():
    from hadoop_bam import formats
    base = "chrUn_gl000220_random|é/0123456789abcdefghijkl"
    assert len(base) >= 40
    for n in range(41):
        s = base[:n]
        assert vcf_ref.murmur_chars(s) == formats.murmurhash3_chars(s), n
    assert any(vcf_ref.murmur_chars(base[:n]) < 0 for n in range(41))


def test_format_dispatch():
    from hadoop_bam import bcf, vcf
    F = vcf.VCFFormat
    assert F.inferFromFilePath("/a/b/x.vcf") == F.VCF
    assert F.inferFromFilePath("x.bcf") == F.BCF
    assert F.inferFromFilePath("x.vcf.gz") is None and F.inferFromFilePath("vcf") is None
    assert F.inferFromData(b"\x1f\x8b\x08\x04") == F.BCF
    assert F.inferFromData(b"BCF\x02\x01") == F.BCF
    assert F.inferFromData(b"##fileformat=VCFv4.1\n") == F.VCF
    assert F.inferFromData(b"20\t1\n") is None and F.inferFromData(b"") is None
    fmt = bcf.VCFInputFormat()
    text = b"##fileformat=VCFv4.1\n"
    # extensions are trusted by default: the data is not looked at
    assert fmt.getFormat("x.vcf", None, b"BCF\x02\x01") == F.VCF
    assert fmt.getFormat("x.bcf", None, text) == F.BCF
    assert fmt.getFormat("x.txt", None, text) == F.VCF
    assert fmt.getFormat("x.txt", None, b"BCF\x02\x01") == F.BCF
    assert fmt.getFormat("x.txt", None, b"hello") is None
    conf = {vcf.TRUST_EXTS_PROPERTY: "false"}
    assert fmt.getFormat("x.bcf", conf, text) == F.VCF
    assert fmt.getFormat("x.vcf", conf, b"\x1f\x8b") == F.BCF


def test_vcf_splits_are_the_plain_file_splits(fixture_vcf):
    from hadoop_bam import bcf
    sp = bcf.VCFInputFormat().getSplits("t.vcf", 512, data=fixture_vcf)
    assert [(s.getStart(), s.getLength()) for s in sp] == vcf_ref.file_splits(1645, 512)
    assert [(s.getStart(), s.getLength()) for s in sp] == [(0, 512), (512, 512), (1024, 512), (1536, 109)]


HEAD = (b"##fileformat=VCFv4.1\n"
        b"##contig=<ID=a,length=5>\n"
        b"##contig=<length=7,assembly=\"x, y\",ID=b,species=\"Homo, sapiens\">\n"
        b"##contig=<ID=a,length=9>\n"
        b"##contig=<ID=\"q,r\",length=1>\n"
        b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"ID=zz, depth\">\n")
CHROM = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def test_header_parse():
    from hadoop_bam import vcf
    data = HEAD + CHROM + b"a\t1\t.\tA\tC\t.\t.\t.\n"
    header, contigs, data_start = vcf.read_vcf_header(data)
    assert header == HEAD + CHROM and data_start == len(HEAD + CHROM)
    assert contigs == [b"a", b"b", b"a", b"q,r"]
    d = {}
    for i, c in enumerate(contigs):
        d[c] = i
    assert d == {b"a": 2, b"b": 1, b"q,r": 3} == vcf_ref.parse_header(data)[1]
    assert vcf_ref.parse_header(data)[2] == data_start
    # \r\n line ends, and a #CHROM line that ends the file
    crlf = (HEAD + CHROM).replace(b"\n", b"\r\n")
    assert vcf.read_vcf_header(crlf)[1:] == (contigs, len(crlf))
    assert vcf.read_vcf_header((HEAD + CHROM)[:-1])[2] == len(HEAD + CHROM) - 1
    # a header longer than the first prefix read
    big = HEAD + b"".join(b"##contig=<ID=c%d,length=1>\n" % i for i in range(6000)) + CHROM + b"x\n"
    assert len(big) > (1 << 16)
    h = vcf.read_vcf_header(big)
    assert len(h[1]) == 6004 and h[2] == len(big) - 2


def test_header_missing_or_followed_by_nothing():
    from hadoop_bam import formats, vcf
    with pytest.raises(formats.IOException, match="No VCF header found"):
        vcf.read_vcf_header(HEAD + b"a\t1\t.\tA\tC\t.\t.\t.\n", "f.vcf")
    with pytest.raises(formats.IOException, match="No VCF header found"):
        vcf.read_vcf_header(HEAD, "f.vcf")
    with pytest.raises(vcf_ref.NoHeader):
        vcf_ref.parse_header(HEAD + b"a\t1\t.\tA\tC\t.\t.\t.\n")
    # a '#' line after #CHROM, or nothing at all: "Empty VCF file" from the reader of the split at 0
    for tail in (b"#late\na\t1\t.\tA\tC\t.\t.\t.\n", b""):
        data = HEAD + CHROM + tail
        with pytest.raises(formats.IOException, match="Empty VCF file"):
            vcf.VCFRecordReader().initialize(formats.FileSplit("f.vcf", 0, len(data)), data=data)
        with pytest.raises(vcf_ref.EmptyFile):
            vcf_ref.read_split(data, 0, len(data))


def test_struct_layouts_match_the_header(tmp_path):
    """hbam_vcf_columns / hbam_vcf_contig as compiled C have the ctypes binding's layout, and the
    structs pinned earlier keep their sizes."""
    import ctypes as C
    import subprocess
    from conftest import ROOT
    from hadoop_bam import _lib
    src = tmp_path / "l.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "hbam.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hbam_vcf_columns), offsetof(hbam_vcf_columns, host),
         offsetof(hbam_vcf_columns, line_off), offsetof(hbam_vcf_columns, key), offsetof(hbam_vcf_columns, text_len),
         sizeof(hbam_vcf_contig), offsetof(hbam_vcf_contig, ordinal), sizeof(hbam_columns),
         sizeof(hbam_bcf_columns));
  return 0;
}''')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True).stdout.split()]
    V, K = _lib.VcfColumnsC, _lib.VcfContigC
    assert got[:5] == [C.sizeof(V), V.host.offset, V.line_off.offset, V.key.offset, V.text_len.offset]
    assert got[5:7] == [C.sizeof(K), K.ordinal.offset] == [12, 8]
    assert got[7] == 240 and got[8] == C.sizeof(_lib.BcfColumnsC)


def test_contig_table_layout():
    """The open-addressing table the kernel probes: a power of two of at least twice the IDs, every
    ID reachable from its FNV-1a slot before an empty one, duplicates keeping the later ordinal."""
    from hadoop_bam import _lib
    names = [b"chr%d" % i for i in range(30)] + [b"chr3", b""]
    tab, size, blob = _lib.Context.vcf_contig_table(names)
    assert size == 64 and size >= 2 * 31
    want = {n: i for i, n in enumerate(names)}
    assert want[b"chr3"] == 30
    for name, ordinal in want.items():
        h = 2166136261
        for b in name:
            h = ((h ^ b) * 16777619) & 0xffffffff
        h &= size - 1
        while True:
            e = tab[h]
            assert e.ordinal >= 0, name
            if blob[e.name_off:e.name_off + e.name_len] == name:
                assert e.ordinal == ordinal
                break
            h = (h + 1) & (size - 1)
    assert sum(1 for e in tab if e.ordinal >= 0) == len(want)
