"""BAI index build on the device and indexed region queries (hadoop_bam/index.py,
csrc/hbam_bai.hip) against tests/bai_ref.py: a plain-Python restatement of the indexing rules over
the CPU oracle's decode, a .bai parser and a brute-force overlap query.

Inputs: the committed fixtures, generated sorted files of at most 30,000 records (small BGZF
blocks with straddling records; three references of which only the first has reads; reads of
70-90 kb that span several 16 KiB windows; no EOF terminator) and files crafted record by record
(gaps in the linear index, several references, an empty one, placed-unmapped reads, reads without
coordinates, and the records the indexer must refuse).  tests/golden/edge_htslib_empty.bam holds
1,381 readable records before its first empty block (tests/golden/expected.json), so the
no-record case is a crafted header-only file."""
import functools
import os

import numpy as np
import pytest

import bai_ref
import helpers
from conftest import GOLDEN

N_REGIONS = 200


# ---- inputs ---------------------------------------------------------------------------------
def _op(n, code):
    return n << 4 | "MIDNSHP=X".index(code)


REFS4 = [(b"chrA", 3000000), (b"chrB", 2000000), (b"chrEmpty", 50000), (b"chrD", 900000)]


def _crafted_multi():
    """Sorted, four references (the third without reads), 4 KiB BGZF blocks: clusters with gaps of
    several 16 KiB windows, reads of 40 kb, placed-unmapped reads, reads without coordinates."""
    rng = np.random.default_rng(5)
    recs = []
    for ref, clusters in ((0, (100, 70000, 70500, 400000)), (1, (16384, 16385, 250000)), (3, (5, 820000))):
        for base in clusters:
            pos = np.sort(rng.integers(base, base + 3000, 60))
            for k, p in enumerate(pos):
                if k % 17 == 5:
                    recs.append(dict(ref=ref, pos=int(p), flag=4 | 1 | 8 << 2, l_seq=30))  # placed, unmapped
                elif k % 23 == 7:
                    recs.append(dict(ref=ref, pos=int(p), cigar=[_op(40000, "M")], l_seq=8))
                elif k % 11 == 3:
                    recs.append(dict(ref=ref, pos=int(p), cigar=[_op(5, "S"), _op(40, "M"), _op(700, "N"), _op(50, "=")],
                                     l_seq=95))
                else:
                    recs.append(dict(ref=ref, pos=int(p), cigar=[_op(100, "M")], l_seq=100))
    recs += [dict(ref=-1, pos=-1, flag=4, l_seq=50) for _ in range(25)]
    return bai_ref.craft_bam(REFS4, recs, block=4096)


def _crafted_odd():
    """Records the CIGAR walk must survive: n_cigar = 0 on a mapped read, an op code above 8, a
    variable block shorter than its fixed lengths claim (layout_ok = 0), a read at position 0."""
    recs = [dict(ref=0, pos=0, cigar=[], l_seq=10),
            dict(ref=0, pos=10, cigar=[_op(50, "M")], l_seq=50),
            dict(ref=0, pos=16384, cigar=[], l_seq=10),
            dict(ref=0, pos=16390, cigar=[20 << 4 | 11, _op(30, "M"), 9 << 4 | 15], l_seq=30),
            dict(ref=0, pos=40000, cigar=[_op(60, "M")], l_seq=60, stored_l_seq=100000),
            dict(ref=0, pos=40010, cigar=[_op(60, "M")], l_seq=60, n_cigar=5000),
            dict(ref=1, pos=7, cigar=[_op(33000, "D"), _op(2, "M")], l_seq=2),
            dict(ref=-1, pos=-1, flag=4, l_seq=5)]
    return bai_ref.craft_bam(REFS4, recs)


@functools.lru_cache(maxsize=None)
def _data(name):
    import genbam
    genbam.lib()
    if name.endswith(".bam"):
        return np.fromfile(os.path.join(GOLDEN, name), np.uint8)
    gen = {
        "gen_small_blocks": dict(records=30000, seed=21, payload=2048, straddle=1, threads=4),
        "gen_nref3": dict(records=20000, seed=22, n_ref=3, threads=4),
        "gen_long": dict(records=20000, seed=23, long_every=997, threads=4),
        "gen_no_eof": dict(records=6000, seed=24, terminator=0, threads=4),
    }
    if name in gen:
        return np.asarray(genbam.generate(**gen[name])).copy()
    return {"crafted_multi": _crafted_multi, "crafted_odd": _crafted_odd,
            "header_only": lambda: bai_ref.craft_bam(REFS4, [])}[name]()


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(decode, (status, err_record, bai, facts)) of the restatement, computed once per input."""
    rec = bai_ref.decode(_data(name))
    return rec, bai_ref.build(rec)


PARITY = ["small_pe.bam", "edge_uniform_long.bam", "edge_htslib_empty.bam", "gen_small_blocks", "gen_nref3",
          "gen_long", "gen_no_eof", "crafted_multi", "crafted_odd", "header_only"]
QUERY = ["small_pe.bam", "crafted_multi"]


def _regions(rec, seed=9, k=N_REGIONS):
    """k seeded regions (ref, beg, end) around the records, then the edge regions."""
    rng = np.random.default_rng(seed)
    placed = np.nonzero(rec["pos"] >= 0)[0]
    out = []
    for _ in range(k):
        i = int(placed[rng.integers(len(placed))])
        r = int(rec["ref_id"][i]) if rng.integers(10) else int(rng.integers(rec["n_ref"]))
        beg = max(1, int(rec["start1"][i]) + int(rng.integers(-3000, 3000)))
        out.append((r, beg, beg + int(rng.choice([0, 1, 99, 4999, 49999])) ))
    i = int(placed[len(placed) // 2])
    r, s = int(rec["ref_id"][i]), int(rec["start1"][i])
    e = int(rec["end1"][i]) or s
    out += [(r, 0, 0), (r, s, s), (r, max(1, s - 50), s - 1), (r, max(1, s - 50), s), (r, e, e + 10),
            (r, e + 1, e + 10), (r, 0, s), (r, s, 0)]
    un = np.nonzero((rec["pos"] >= 0) & ((rec["flag"] & 4) != 0))[0]
    if len(un):
        out.append((int(rec["ref_id"][un[0]]), int(rec["start1"][un[0]]), int(rec["start1"][un[0]])))
    empty = sorted(set(range(rec["n_ref"])) - set(int(x) for x in rec["ref_id"][placed]))
    if empty:
        out.append((empty[0], 0, 0))
    return out


# ---- CPU ------------------------------------------------------------------------------------
def test_inputs_exercise_the_rules():
    """Asserted on the restatement's output: without these the byte parity proves little."""
    facts = [_ref(n)[1][3] for n in PARITY]
    assert all(_ref(n)[1][0] == 0 for n in PARITY)
    for k in ("multi_chunk_bin", "extended_across_block", "multi_window_record", "filled_slot",
              "empty_reference", "placed_unmapped"):
        assert any(f[k] for f in facts), k
    assert any(f["n_no_coor"] > 0 for f in facts)
    # the listed generated inputs do what they were chosen for
    assert _ref("gen_small_blocks")[1][3]["extended_across_block"] and _ref("gen_small_blocks")[1][3]["multi_chunk_bin"]
    assert _ref("gen_long")[1][3]["multi_window_record"]
    refs, _ = bai_ref.parse(_ref("gen_nref3")[1][2])
    assert refs[0]["bins"] and not refs[2]["bins"] and not refs[2]["lin"]
    refs, nnc = bai_ref.parse(_ref("header_only")[1][2])
    assert all(not r["bins"] and not r["lin"] for r in refs) and nnc == 0


def test_generated_bins_are_reg2bin():
    """Guards the inputs: the generator's stored bin is reg2bin(pos, end) for mapped reads."""
    for name in ("small_pe.bam", "gen_long", "crafted_multi"):
        rec = _ref(name)[0]
        m = np.nonzero((rec["pos"] >= 0) & ((rec["flag"] & 4) == 0) & (rec["reflen"] > 0))[0]
        assert len(m) > 100
        want = [bai_ref.reg2bin(int(rec["pos"][i]), int(rec["pos"][i] + rec["reflen"][i])) for i in m]
        assert np.array_equal(rec["bin"][m], np.array(want, np.uint16)), name


@pytest.mark.parametrize("name", QUERY + ["gen_long"])
def test_span_overlapping_holds_every_hit(name):
    """The product's host code over the restatement's .bai: every brute-force hit lies inside a
    returned chunk; the chunks are sorted and disjoint."""
    from hadoop_bam.index import BAMIndex
    rec, (st, _, bai, _) = _ref(name)
    assert st == 0
    idx = BAMIndex(bai)
    voff = rec["voffset"].astype(np.uint64)
    share = []
    for r, beg, end in _regions(rec):
        chunks = idx.span_overlapping(r, beg, end)
        for (a, b), (c, d) in zip(chunks, chunks[1:]):
            assert a < b < c < d, (r, beg, end, chunks)
        hits = bai_ref.overlapping(rec, r, beg, end)
        cb = np.array([c[0] for c in chunks], np.uint64)
        ce = np.array([c[1] for c in chunks], np.uint64)
        k = np.searchsorted(cb, voff[hits], side="right").astype(np.int64) - 1
        assert np.all(k >= 0) and np.all(voff[hits] < ce[k]), (r, beg, end)
        covered = sum(int(np.searchsorted(voff, b) - np.searchsorted(voff, a)) for a, b in chunks)
        share.append(covered / max(1, rec["n"]))
    print("%s: chunks of a region cover %.4f of the file's records on average (max %.4f)"
          % (name, float(np.mean(share)), float(np.max(share))))


def test_bamindex_roundtrip_and_rejects():
    from hadoop_bam.formats import SAMFormatException
    from hadoop_bam.index import BAMIndex
    for name in ("crafted_multi", "gen_nref3", "header_only"):
        bai = _ref(name)[1][2]
        idx = BAMIndex(bai)
        assert idx.to_bytes() == bai
        refs, nnc = bai_ref.parse(bai)
        assert idx.n_no_coor == nnc and len(idx.refs) == len(refs)
        for a, b in zip(idx.refs, refs):
            want = {k: [tuple(c) for c in v] for k, v in b["bins"].items() if k != bai_ref.META_BIN}
            assert a.bins == want and list(a.linear) == b["lin"]
            assert (a.meta is not None) == (bai_ref.META_BIN in b["bins"])
        old = BAMIndex(bai[:-8])  # written without the trailing n_no_coor
        assert old.n_no_coor is None and old.to_bytes() == bai[:-8]
    bai = _ref("crafted_multi")[1][2]
    for cut in (3, 6, 8, 11, 30, len(bai) // 2, len(bai) - 9, len(bai) - 3):
        with pytest.raises(SAMFormatException):
            BAMIndex(bai[:cut])
    with pytest.raises(SAMFormatException):
        BAMIndex(b"BAI\x02" + bai[4:])
    with pytest.raises(SAMFormatException):
        BAMIndex(b"")


def test_parse_region_follows_view():
    from hadoop_bam.formats import IllegalArgumentException
    from hadoop_bam.index import parse_region
    from hadoop_bam.output import SAMFileHeader
    h = SAMFileHeader(b"", [(b"chr1", 1000), (b"7", 500), (b"chrX", 10)])
    assert parse_region(h, "chr1") == (0, 0, 0)
    assert parse_region(h, "chrX:5-9") == (2, 5, 9)
    assert parse_region(h, "chr1:0-0") == (0, 0, 0)
    assert parse_region(h, "chr1:7-7") == (0, 7, 7)
    assert parse_region(h, "chr1:+3-4") == (0, 3, 4)      # Integer.parseInt takes a sign
    assert parse_region(h, "chr1:") == (0, 0, 0)          # StringTokenizer yields one token
    assert parse_region(h, "7") == (1, 0, 0)              # a name wins over an index
    assert parse_region(h, "2:1-2") == (2, 1, 2)          # index fallback
    assert parse_region(h, "0") == (0, 0, 0)
    assert parse_region(h, "-1") == (1, 0, 0)             # '-' is a delimiter: the token is "1"
    for bad in ("chr1:10-5",          # cannot end before start
                "chr1:10",            # no end: parsed as -1, refused
                "chr1:1,000-2,000",   # parseCoordinate is Integer.parseInt: no separators
                "chr1:a-b", "chr1:1-2147483648", "nope", "3", "", ":"):
        with pytest.raises(IllegalArgumentException):
            parse_region(h, bad)


# ---- GPU ------------------------------------------------------------------------------------
def _device_decode(ctx, data):
    h = ctx.parse_header(data)
    rc, d = ctx.decode_split_device(data, h["first_voffset"], (len(data) << 16) | 0xffff, h["n_ref"])
    assert rc == 0, ctx.last_error()
    return h, d


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_bai_bytes_equal_the_restatement(gpu_ctx, name):
    test_inputs_exercise_the_rules()
    data = _data(name)
    rec, (st, _, want, _) = _ref(name)
    assert st == 0
    rc, got, err = gpu_ctx.bai_index(data)
    assert rc == 0, (rc, err, gpu_ctx.last_error())
    assert got == want
    if name == "gen_no_eof":
        assert rec["end_voffset"] == len(data) << 16
        _, d = _device_decode(gpu_ctx, data)
        rc, got, _ = gpu_ctx.bai_build(d, rec["n_ref"], len(data) << 16)
        assert rc == 0 and got == want


@pytest.mark.gpu
def test_unsorted_file_raises_where_the_restatement_does(gpu_ctx):
    data = _data("edge_unsorted_l1.bam")
    rec, (st, err, want, _) = _ref("edge_unsorted_l1.bam")
    rc, got, gerr = gpu_ctx.bai_index(data)
    if st == 0:  # never steps a reference backwards: then the bytes, and a file that does
        assert rc == 0 and got == want
        small = _data("gen_no_eof")
        data = helpers.regroup_bam(small, lambda t: t, lambda i, v: v, ref_fn=lambda i, r: 1 if i < 3000 else 0)
        rec = bai_ref.decode(data)
        st, err, want, _ = bai_ref.build(rec)
        rc, got, gerr = gpu_ctx.bai_index(data)
    assert st == bai_ref.EDATA
    assert (rc, gerr) == (st, err)


@pytest.mark.gpu
def test_refused_records(gpu_ctx):
    """A position past 2^29 -> HBAM_EINDEX at that record; a reference outside the dictionary handed
    to the build, or a step back to a smaller reference -> HBAM_EDATA; never a fault."""
    ok = dict(ref=0, pos=100, cigar=[_op(50, "M")], l_seq=50)
    cases = [
        ([ok, dict(ref=0, pos=(1 << 29) + 5, cigar=[_op(10, "M")], l_seq=10), ok], None, bai_ref.EINDEX, 1),
        ([ok, dict(ref=0, pos=(1 << 29) - 20, cigar=[_op(50, "M")], l_seq=50)], None, bai_ref.EINDEX, 1),
        ([ok, dict(ref=0, pos=(1 << 29) - 20, cigar=[_op(10, "M")], l_seq=10)], None, 0, None),
        ([ok, dict(ref=0, pos=0x7fffffff, flag=4, l_seq=10)], None, bai_ref.EINDEX, 1),
        ([ok, dict(ref=1, pos=5, cigar=[_op(10, "M")], l_seq=10), dict(ref=3, pos=5, l_seq=10)], 2, bai_ref.EDATA, 2),
        ([dict(ref=1, pos=5, l_seq=10), dict(ref=-1, pos=-1, flag=4, l_seq=3), ok,
          dict(ref=0, pos=(1 << 29) + 5, l_seq=10)], None, bai_ref.EDATA, 2),
    ]
    for recs, n_ref, want_st, want_err in cases:
        data = bai_ref.craft_bam(REFS4, recs)
        rec = bai_ref.decode(data)
        n_ref = rec["n_ref"] if n_ref is None else n_ref
        st, err, want, _ = bai_ref.build(rec, n_ref=n_ref)
        assert (st, err) == (want_st, want_err)
        _, d = _device_decode(gpu_ctx, data)
        rc, got, gerr = gpu_ctx.bai_build(d, n_ref, rec["end_voffset"])
        assert (rc, gerr, got) == (st, err, want)


@pytest.mark.gpu
def test_odd_cigars_index_as_the_restatement(gpu_ctx):
    """n_cigar = 0, op codes above 8, layout_ok = 0: statuses and bytes as the restatement."""
    rec, (st, _, want, _) = _ref("crafted_odd")
    assert st == 0 and list(rec["layout_ok"]) == [1, 1, 1, 1, 0, 0, 1, 1]
    assert list(rec["reflen"]) == [0, 50, 0, 30, 0, 0, 33002, 0]
    rc, got, _ = gpu_ctx.bai_index(_data("crafted_odd"))
    assert rc == 0 and got == want


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUERY + ["crafted_odd"])
def test_overlap_filter_equals_brute_force(gpu_ctx, name):
    data = _data(name)
    rec = _ref(name)[0]
    _, d = _device_decode(gpu_ctx, data)
    assert int(d.n_records) == rec["n"]
    regions = _regions(rec, seed=4, k=40)
    hit = False
    for r, beg, end in regions:
        for contained in (False, True):
            got = gpu_ctx.overlap_indices(d, r, beg, end, contained)
            want = bai_ref.overlapping(rec, r, beg, end, contained)
            assert np.array_equal(got, want.astype(np.uint32)), (r, beg, end, contained)
            hit |= len(want) > 0
    assert hit
    # the edge regions around one read, spelled out
    i = int(np.nonzero((rec["pos"] > 100) & (rec["end1"] > 0))[0][3])
    r, s, e = int(rec["ref_id"][i]), int(rec["start1"][i]), int(rec["end1"][i])
    assert i not in gpu_ctx.overlap_indices(d, r, s - 50, s - 1) and i in gpu_ctx.overlap_indices(d, r, s - 50, s)
    assert i in gpu_ctx.overlap_indices(d, r, e, e + 9) and i not in gpu_ctx.overlap_indices(d, r, e + 1, e + 9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUERY)
def test_query_overlapping_equals_brute_force(gpu_ctx, name):
    """Set and order of the returned records (indices, raw bytes, voffsets) equal brute force over
    the full oracle decode.  Every query narrower than a tenth of its reference (the length in the
    header's dictionary) decodes fewer compressed bytes than the file holds; the ratio is logged,
    and on its own line the ratio of the queries narrower than a tenth of what the reads span (the
    reads of these files span far less than a reference)."""
    from hadoop_bam.index import IndexedBAMReader
    data = _data(name)
    rec, (st, _, bai, _) = _ref(name)
    rc, got_bai, _ = gpu_ctx.bai_index(data)
    assert rc == 0 and got_bai == bai
    rd = IndexedBAMReader(data, gpu_ctx, index=got_bai)
    voff = rec["voffset"]
    placed = rec["pos"][rec["pos"] >= 0]
    span_tenth = (int(placed.max()) - int(placed.min())) // 10
    ref_len = [ln for _, ln in rd.header.getSequenceDictionary()]
    ratios, span_ratios, widened = [], [], 0
    for r, beg, end in _regions(rec):
        got = rd.query_overlapping(r, beg, end)
        widened += rd.last_query["widened"]
        want = bai_ref.overlapping(rec, r, beg, end)
        gv = np.array([g.voffset for g in got], np.uint64)
        assert np.array_equal(gv, voff[want]), (r, beg, end)
        assert np.array_equal(np.searchsorted(voff, gv), want)
        assert [g.toBAMBytes() for g in got] == bai_ref.record_bytes(rec, want)
        if end > 0 and end - beg < ref_len[r] // 10:
            assert rd.last_query["comp_bytes"] < len(data), (r, beg, end, rd.last_query)
            ratios.append(rd.last_query["comp_bytes"] / len(data))
            if end - beg < span_tenth:
                span_ratios.append(ratios[-1])
    assert len(ratios) > N_REGIONS // 2
    print("%s: compressed bytes decoded per query / file size, queries narrower than a tenth of the reference: "
          "mean %.4f max %.4f over %d queries; %d chunk windows widened"
          % (name, float(np.mean(ratios)), float(np.max(ratios)), len(ratios), widened))
    print("%s: the same, queries narrower than a tenth of what the reads span: mean %.4f max %.4f over %d queries"
          % (name, float(np.mean(span_ratios)), float(np.max(span_ratios)), len(span_ratios)))
    r0 = int(rec["ref_id"][0])
    want = bai_ref.overlapping(rec, r0, 1000, 60000, contained=True)
    got = rd.query_contained(rd.names[r0], 1000, 60000)
    assert [g.voffset for g in got] == [int(v) for v in voff[want]] and len(want) > 0


@pytest.mark.gpu
def test_indexer_writes_the_bai_next_to_the_file(gpu_ctx, tmp_path):
    from hadoop_bam.formats import IOException
    from hadoop_bam.index import BAMIndexer, IndexedBAMReader
    data = _data("crafted_multi")
    rec, (st, _, want, _) = _ref("crafted_multi")
    path = str(tmp_path / "in.bam")
    data.tofile(path)
    with pytest.raises(IOException):
        IndexedBAMReader(path, gpu_ctx)
    assert BAMIndexer(gpu_ctx).index(path) == want
    assert open(path + ".bai", "rb").read() == want
    rd = IndexedBAMReader(path, gpu_ctx)
    got = rd.query_region("chrB:16000-17000")
    hits = bai_ref.overlapping(rec, 1, 16000, 17000)
    assert len(hits) > 0 and [g.voffset for g in got] == [int(v) for v in rec["voffset"][hits]]
    other = str(tmp_path / "elsewhere.bai")
    assert BAMIndexer(gpu_ctx).index(data, out_path=other) == want and open(other, "rb").read() == want


@pytest.mark.gpu
def test_raised_types_are_the_readers(gpu_ctx):
    """The mirror raises the classes the other readers raise for the same codes."""
    from hadoop_bam.consumers import IndexOutOfBoundsException
    from hadoop_bam.formats import (IllegalArgumentException, IOException, JavaRuntimeException,
                                    SAMFormatException, _EXC as EXC)
    from hadoop_bam.index import BAMIndexer, IndexedBAMReader
    ix = BAMIndexer(gpu_ctx)
    with pytest.raises(JavaRuntimeException):  # HBAM_EDATA: "Unexpected reference"
        ix.index(_data("edge_unsorted_l1.bam"))
    far = bai_ref.craft_bam(REFS4, [dict(ref=0, pos=(1 << 29) + 5, cigar=[_op(10, "M")], l_seq=10)])
    with pytest.raises(IndexOutOfBoundsException):
        ix.index(far)
    data = _data("crafted_multi")
    bai = _ref("crafted_multi")[1][2]
    with pytest.raises(IOException):
        IndexedBAMReader(data, gpu_ctx)  # bytes and no index
    with pytest.raises(SAMFormatException):
        IndexedBAMReader(data, gpu_ctx, index=bai[:40])
    rd = IndexedBAMReader(data, gpu_ctx, index=bai)
    for bad in ("chrNope", 4, -1):
        with pytest.raises(IllegalArgumentException):
            rd.query_overlapping(bad, 1, 100)
    with pytest.raises(IllegalArgumentException):
        rd.query_region("chrA:10-5")
    # a file cut inside the BGZF block of chrD's last read: a query that needs the block raises what a
    # reader of the whole cut file raises there, a query that does not need it is answered
    rec = _ref("crafted_multi")[0]
    last = int(np.nonzero(rec["ref_id"] == 3)[0][-1])
    short = data[:(int(rec["voffset"][last]) >> 16) + 20].copy()
    whole = gpu_ctx.decode_split(short, rec["header"]["first_voffset"], (len(short) << 16) | 0xffff, rec["n_ref"])
    assert whole["rc"] == 0 and whole["status"] not in (0, -12) and whole["n"] < rec["n"]
    cut = IndexedBAMReader(short, gpu_ctx, index=bai)
    assert len(cut.query_overlapping("chrA", 1, 5000)) == len(rd.query_overlapping("chrA", 1, 5000)) > 0
    with pytest.raises(EXC[whole["status"]]):
        cut.query_overlapping("chrD", 820000, 830000)
