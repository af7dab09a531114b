"""VCF text output on the device (hbam_vcf_render, hbam_vcftext.hip): every text is compared byte for
byte with the rule restatement (tests/vcftext_ref.py), never with render_record."""
import os
import struct

import numpy as np
import pytest

import bcf_records
import vcftext_cases as C
import vcftext_ref as R
from helpers import bgzf_pack

pytestmark = pytest.mark.gpu


def host_header(e):
    from hadoop_bam.vcf_text import VCFHeader
    return VCFHeader(e.text.encode())


def render(ctx, e, recs, device=False, perm=None):
    H = host_header(e)
    data, off = C.pack(recs)
    n = len(recs) if perm is None else len(perm)
    if not device:
        return ctx.vcf_render(data, len(data), off, n, H.counts, H.meta(), on_device=False)
    d = ctx.upload(data + bytes(64))
    o = ctx.upload(off.tobytes() or bytes(8))
    p = None if perm is None else ctx.upload(np.asarray(perm, np.uint32).tobytes() or bytes(4))
    try:
        return ctx.vcf_render(d.ptr, len(data), o.ptr, n, H.counts, H.meta(), perm=None if p is None else p.ptr,
                              on_device=True)
    finally:
        for b in (d, o, p):
            if b is not None:
                b.free()


def assert_same(got, ref):
    assert got["rc"] == 0, got
    assert (got["status"], got["n"]) == (ref["status"], ref["n"])
    assert got["err_record"] == (ref["n"] if ref["status"] else 0)
    assert list(got["deferred"]) == ref["deferred"]
    assert list(got["line_off"]) == ref["line_off"]
    assert got["text"] == ref["text"]


def test_crafted_records_host_arrays(gpu_ctx):
    e, crafted = C.crafted()
    recs = [r for _, r in crafted]
    ref = R.render_stream(recs, e.hdr)
    got = render(gpu_ctx, e, recs)
    assert_same(got, ref)
    assert ref["status"] == R.OK and 0 < len(ref["deferred"]) < len(recs)
    me, mrec = C.crafted_many_fields()
    assert_same(render(gpu_ctx, me, [mrec]), R.render_stream([mrec], me.hdr))
    ge, grecs = C.golden_records()
    got = render(gpu_ctx, ge, grecs)
    assert got["text"] == C.GOLDEN_EXPECTED and len(got["deferred"]) == 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_tile_edges(gpu_ctx, n):
    e = C.craft_encoder()
    recs = C.varied_records(e, n)
    ref = R.render_stream(recs, e.hdr)
    if n == 129:
        assert len(set(o % 16 for o in ref["line_off"])) == 16  # lines start at every offset mod 16
    assert_same(render(gpu_ctx, e, recs), ref)
    assert_same(render(gpu_ctx, e, recs, device=True), ref)
    rev = list(range(n))[::-1]
    assert_same(render(gpu_ctx, e, recs, device=True, perm=rev), R.render_stream(recs, e.hdr, rev))
    rep = [(7 * k) % max(n // 2, 1) for k in range(n)]  # indices repeat
    assert_same(render(gpu_ctx, e, recs, device=True, perm=rep), R.render_stream(recs, e.hdr, rep))


@pytest.mark.parametrize("ns", [0, 1, 3, 63, 64, 65, 130])
def test_sample_counts(gpu_ctx, ns):
    """63 and fewer: a lane per record; 64 and more: a wave per record (HBAM_VCF_WAVE_SAMPLES)"""
    e, recs = C.sample_records(ns)
    ref = R.render_stream(recs, e.hdr)
    assert ref["status"] == R.OK and ref["deferred"] == [] and ref["n"] == 8
    assert_same(render(gpu_ctx, e, recs), ref)
    rev = list(range(8))[::-1]
    assert_same(render(gpu_ctx, e, recs, device=True, perm=rev), R.render_stream(recs, e.hdr, rev))


def test_wave_path_statuses_and_deferral(gpu_ctx):
    """the per-sample failures and the deferral that only the samples decide, found by the wave pass"""
    ns = 70
    e = C.craft_encoder(samples=tuple("N%d" % i for i in range(ns)))
    M8 = C.MISS[C.INT8]
    gt = [[2, 4]] * ns
    ok = e.record(pos=1, fmt=[("GT", C.INT8, 2, gt), ("DP", C.INT8, 1, [[s % 100] for s in range(ns)])])
    bad_allele = e.record(pos=2, fmt=[("GT", C.INT8, 2, gt[:68] + [[2, 8]] + gt[69:])])
    null_gt = e.record(pos=3, fmt=[("GT", C.INT8, 2, gt[:66] + [[M8, M8]] + gt[67:])])
    g_null = e.record(pos=4, fmt=[("GT", C.INT8, 2, gt), ("XG", C.INT8, 3, [[1, 2, 3]] * 65 + [[M8] * 3] + [[4, 5, 6]] * 4)])
    fl = e.record(pos=5, fmt=[("GT", C.INT8, 2, gt), ("XF", C.FLOAT, 1, [[0.5]] * ns)])
    for recs in ([ok, g_null, fl, ok], [ok, bad_allele, ok], [g_null, ok, null_gt]):
        ref = R.render_stream(recs, e.hdr)
        assert_same(render(gpu_ctx, e, recs), ref)
    assert R.render_stream([ok, g_null, fl, ok], e.hdr)["deferred"] == [1, 2]


STATUS_ENC, STATUS = C.status_cases()


@pytest.mark.parametrize("at", [0, 63, 64, 129])
@pytest.mark.parametrize("name", [n for n, _, _ in STATUS])
def test_status_cases(gpu_ctx, name, at):
    rec, status = [(r, s) for n, r, s in STATUS if n == name][0]
    recs = C.varied_records(STATUS_ENC, 130)
    recs[at] = rec
    ref = R.render_stream(recs, STATUS_ENC.hdr)
    assert (ref["status"], ref["n"]) == (status, at)
    assert_same(render(gpu_ctx, STATUS_ENC, recs), ref)


@pytest.mark.parametrize("case", C.stop_streams(), ids=[c[0] for c in C.stop_streams()])
def test_stop_among_deferred_records(gpu_ctx, case):
    """a failing record with deferred records before and behind it and another failing record behind
    it, found by the lane pass (3 samples) and by the wave pass's sizes half (70 samples)"""
    name, e, recs, n, status, deferred = case
    ref = R.render_stream(recs, e.hdr)
    assert (ref["n"], ref["status"], ref["deferred"]) == (n, status, deferred)
    assert_same(render(gpu_ctx, e, recs), ref)
    assert_same(render(gpu_ctx, e, recs, device=True), ref)


# ---- end to end -----------------------------------------------------------------------------------------
def decode_and_render(ctx, file_bytes):
    from hadoop_bam.vcf_text import read_vcf_header_from
    h = ctx.bcf_parse_header(file_bytes[:1 << 20])
    assert isinstance(h, dict), h
    H = read_vcf_header_from(file_bytes, ctx)
    if h["bgzf"]:
        rc, d = ctx.bcf_decode_split_device(file_bytes, h, h["first_voffset"], (len(file_bytes) << 16) | 0xffff)
    else:
        rc, d = ctx.bcf_decode_split_device(file_bytes, h, 0, len(file_bytes))
    assert rc == 0 and int(d.status) == 0
    got = ctx.vcf_render(d.data, int(d.data_len), d.rec_off, int(d.n_records), H.counts, H.meta(), on_device=True)
    return H, int(d.n_records), got


@pytest.mark.parametrize("packed", [True, False])
def test_end_to_end(gpu_ctx, packed):
    """bcf_stream(2000, hom_ref=1.0): see test_vcftext.test_stream_deferred_share for why not the
    generator's default, which test_end_to_end_default_stream renders."""
    stream = bcf_records.bcf_stream(2000, hom_ref=1.0)
    text, recs = C.split_stream(stream)
    ref = R.render_stream(recs, C.Enc(text).hdr)
    H, n, got = decode_and_render(gpu_ctx, bgzf_pack(stream) if packed else stream)
    assert H.text == text.encode() and n == 2000
    assert_same(got, ref)
    assert 0 < len(got["deferred"]) / 2000.0 < 0.05


def test_end_to_end_default_stream(gpu_ctx):
    """the generator's default calls name alleles the records do not have: the first one ends the output"""
    stream = bcf_records.bcf_stream(2000)
    text, recs = C.split_stream(stream)
    ref = R.render_stream(recs, C.Enc(text).hdr)
    assert (ref["status"], ref["n"]) == (R.ERUNTIME, 0)
    _, n, got = decode_and_render(gpu_ctx, stream)
    assert n == 2000
    assert_same(got, ref)


def shuffled_stream(n=600, seed=5):
    stream = bcf_records.bcf_stream(n, hom_ref=1.0)
    text, recs = C.split_stream(stream)
    lt = struct.unpack_from("<I", stream, 5)[0]
    order = np.random.default_rng(seed).permutation(n)
    recs = [recs[i] for i in order]
    for i in range(0, n, 50):  # equal keys, which must keep their input order
        recs[i + 1] = recs[i + 1][:8] + recs[i][8:16] + recs[i + 1][16:]
    return text, recs, stream[:9 + lt] + b"".join(recs)


def test_vcf_sort_bcf_input(gpu_ctx, tmp_path):
    from hadoop_bam import FileSplit
    from hadoop_bam.bcf import VCFInputFormat, record_keys
    from hadoop_bam.vcf import VCFRecordReader, vcf_sort
    text, recs, stream = shuffled_stream()
    hdr = C.Enc(text).hdr
    keys = np.array([struct.unpack_from("<ii", r, 8) for r in recs], np.int64)
    keys = keys[:, 0] << 32 | keys[:, 1]
    assert len(set(keys.tolist())) < len(keys)
    order = np.argsort(keys, kind="stable")
    lines = [R.render(recs[i], hdr) for i in order]
    assert all(st == R.OK for st, _, _ in lines)
    want = text.encode() + b"".join(ln for _, ln, _ in lines)
    for name, blob in (("in_bgzf.bcf", bgzf_pack(stream)), ("in_plain.bcf", stream)):
        src, out = str(tmp_path / name), str(tmp_path / (name + ".out.vcf"))
        with open(src, "wb") as f:
            f.write(blob)
        res = vcf_sort(src, out)
        assert res["n"] == len(recs) and res["deferred"] == sum(d for _, _, d in lines)
        assert open(out, "rb").read() == want
    rr = VCFRecordReader()
    rr.initialize(FileSplit(out, 0, os.path.getsize(out)))
    got_keys, exc = record_keys(rr)
    assert exc is None
    fmt = VCFInputFormat()
    bkeys = []
    for sp in fmt.getSplits(src, 1 << 30):
        k, exc = record_keys(fmt.createRecordReader(sp))
        assert exc is None
        bkeys.append(k)
    assert np.array_equal(got_keys, np.sort(np.concatenate(bkeys), kind="stable"))
    with pytest.raises(NotImplementedError):
        vcf_sort(src, str(tmp_path / "out.bcf"))


def test_vcf_sort_text_input_unchanged(gpu_ctx, tmp_path):
    """the text-VCF path: tests/golden/test.vcf is in key order, so its sorted output is the file itself"""
    from hadoop_bam.vcf import vcf_sort
    src = os.path.join(C.HERE, "golden", "test.vcf")
    out = str(tmp_path / "sorted.vcf")
    res = vcf_sort(src, out)
    assert res["n"] == 5 and set(res) == {"n", "sort_ms", "gather_ms"}
    assert open(out, "rb").read() == open(src, "rb").read()


def test_key_ignoring_output_format_parts(gpu_ctx, tmp_path):
    from hadoop_bam.formats import Configuration
    from hadoop_bam.vcf import VCFFormat
    from hadoop_bam.vcf_text import WRITE_HEADER_PROPERTY, KeyIgnoringVCFOutputFormat
    e, crafted = C.crafted()
    recs = [r for _, r in crafted]
    want = e.text.encode() + b"".join(R.render_stream(recs, e.hdr)["lines"])
    f = KeyIgnoringVCFOutputFormat(VCFFormat.VCF)
    f.setHeader(host_header(e))
    one = str(tmp_path / "one.vcf")
    w = f.getRecordWriter(one, ctx=gpu_ctx)
    w.write_encoded(b"".join(recs))
    w.close()
    assert open(one, "rb").read() == want
    parts = []
    conf = Configuration({WRITE_HEADER_PROPERTY: "false"})
    for k, chunk in enumerate((recs[:31], recs[31:])):
        p = str(tmp_path / ("part-%d" % k))
        w = f.getRecordWriter(p, conf, ctx=gpu_ctx)
        for r in chunk:
            w.write_encoded(r)
        w.close()
        parts.append(open(p, "rb").read())
    assert e.text.encode() + b"".join(parts) == want


def test_writer_stops_at_the_first_failing_record(gpu_ctx, tmp_path):
    """whether the device found it (a status) or the host renderer did (a deferred record is checked on
    the device like any other, so here the two agree): nothing behind that record is written"""
    import io

    from hadoop_bam.bcf import BCFDecodeRuntimeException
    from hadoop_bam.vcf_text import VCFRecordWriter
    e, crafted = C.crafted()
    good = [r for _, r in crafted][:40]
    bad = [r for n, r, _ in C.status_cases()[1] if n == "gt_range"][0]
    out = io.BytesIO()
    w = VCFRecordWriter(out, host_header(e), False, gpu_ctx)
    w.write_encoded(b"".join(good + [bad] + good))
    with pytest.raises(BCFDecodeRuntimeException):
        w.close()
    assert out.getvalue() == b"".join(R.render_stream(good, e.hdr)["lines"])
