"""Empty BGZF blocks against tribble's 512,000-byte fills (BCF).

BCFRecordReader reads a BGZF split through a PositionalBufferedStream whose fills are
BlockCompressedInputStream reads (through BGZFLimitingStream: at most vEnd & 0xffff bytes each), and
such a read returns -1 when it starts exactly at an empty block.  A fill whose first read begins
there ends the stream; a later read of a fill that begins there ends that fill short, so the
following fills start elsewhere; inside a read an empty block changes nothing.
bcf_stream_end (csrc/hbam_bcf_api.hip) replays the fills over the block table; here the replay meets
empty blocks at, next to and away from the fill boundaries, and must equal the oracle (n, status,
keys).  FILL files: dict name -> (file bytes, split start, split end)."""
import numpy as np
import pytest

import bcf_records
import chain_craft as cc

FILL = 512000
BLOCK = 65280
N_REC = 13000


def _pack(u, at=(), extra_cuts=()):
    """65280-byte members, a cut at each stream offset of `at` / `extra_cuts`, an empty member before
    the member that starts at each offset of `at` (an offset given twice: two empty members)."""
    cuts = sorted(set(cc.even_cuts(len(u), BLOCK)) | set(at) | set(extra_cuts))
    data = cc.bgzf_pack_at(u, cuts, [cuts.index(a) + 1 for a in at])
    return data


@pytest.fixture(scope="module")
def fills():
    import oracle
    u = bcf_records.bcf_stream(N_REC, seed=3)
    h = dict(oracle.bcf_header(u), bgzf=True)
    r0 = h["header_len"]
    assert len(u) > r0 + 2 * FILL + 50000
    p, starts = r0, []
    while p < len(u):
        starts.append(p)
        p += 8 + int.from_bytes(u[p:p + 4], "little") + int.from_bytes(u[p + 4:p + 8], "little")
    assert len(starts) == N_REC and p == len(u)
    inside = next(s for s in starts if s > r0 + 200000) + 10  # mid-fill, inside a record
    f = {}

    def whole(name, data):
        f[name] = (data, r0, len(data) << 16 | 0xffff)

    whole("none", _pack(u, extra_cuts=[r0 + FILL]))
    whole("at_fill", _pack(u, [r0 + FILL]))
    whole("at_fill_minus_1", _pack(u, [r0 + FILL - 1]))
    whole("at_fill_plus_1", _pack(u, [r0 + FILL + 1]))
    whole("at_second_fill", _pack(u, [r0 + 2 * FILL]))
    whole("two_at_fill", _pack(u, [r0 + FILL, r0 + FILL]))
    whole("mid_fill_in_record", _pack(u, [inside]))
    whole("mid_fill_then_old_boundary", _pack(u, [inside, r0 + FILL]))
    # the fill's reads are 65535 bytes long (vEnd & 0xffff): its second read starts at r0 + 65535
    whole("at_second_read", _pack(u, [r0 + 65535]))
    whole("at_second_read_then_old_boundary", _pack(u, [r0 + 65535, r0 + FILL]))
    whole("at_second_read_then_new_boundary", _pack(u, [r0 + 65535, r0 + 65535 + FILL]))
    whole("before_eof", cc.bgzf_pack_at(u, cc.even_cuts(len(u), BLOCK), [len(cc.even_cuts(len(u), BLOCK)) + 1]))
    # an empty first member; the split starts in it (the reader seeks to the next block)
    whole("first_member", cc.bgzf_pack_at(u, cc.even_cuts(len(u), BLOCK), [0]))
    # ... and a split that starts at an empty member in the middle of the file (a window from there)
    rs = next(s for s in starts if s > 150000)
    data = _pack(u, [rs])
    coff, uoff = cc.bgzf_layout(data)
    k = uoff.index(rs)
    assert uoff[k + 1] == rs  # member k is the empty one
    f["start_at_empty"] = (data, coff[k] << 16, len(data) << 16 | 0xffff)
    # a split whose end lies in the block after an empty one
    data = _pack(u, [r0 + 300000])
    coff, uoff = cc.bgzf_layout(data)
    k = uoff.index(r0 + 300000)
    f["v_end_after_empty"] = (data, r0, coff[k + 1] << 16 | 100)
    data = _pack(u, [r0 + FILL])
    coff, uoff = cc.bgzf_layout(data)
    k = uoff.index(r0 + FILL)
    f["v_end_after_empty_at_fill"] = (data, r0, coff[k + 1] << 16 | 100)
    return dict(files=f, h=h, starts=starts, u=u)


NAMES = ["none", "at_fill", "at_fill_minus_1", "at_fill_plus_1", "at_second_fill", "two_at_fill",
         "mid_fill_in_record", "mid_fill_then_old_boundary", "at_second_read", "at_second_read_then_old_boundary",
         "at_second_read_then_new_boundary", "before_eof", "first_member", "start_at_empty",
         "v_end_after_empty", "v_end_after_empty_at_fill"]


def test_oracle_ends_at_an_empty_block_on_a_fill_boundary(fills, oracle_mod):
    """The edge is one byte wide: a fill that starts exactly at an empty block ends the stream (the
    record cut there fails: TribbleException), one byte to either side the file reads whole.  The
    first 9000 records of the stream are bcf_stream(9000, seed=3), for which n = 5995 was recorded."""
    h = fills["h"]
    res = {}
    for name in NAMES:
        data, a, b = fills["files"][name]
        r = oracle_mod.read_bcf_split(data, a, b, h)
        res[name] = (r["n"], r["status"])
    assert res["none"] == (N_REC, 0)
    assert res["at_fill"] == (5995, -14)
    assert fills["starts"][5995] < h["header_len"] + FILL < fills["starts"][5996]
    assert res["at_fill_minus_1"] == res["at_fill_plus_1"] == (N_REC, 0)
    assert res["two_at_fill"] == (5995, -14)
    assert res["at_second_fill"][0] < N_REC and res["at_second_fill"][1] != 0
    assert res["mid_fill_in_record"] == res["before_eof"] == res["first_member"] == (N_REC, 0)
    # an empty block inside a read leaves the fills where they were ...
    assert res["mid_fill_then_old_boundary"] == (5995, -14)
    # ... one where a later read of the fill starts ends the fill there: the next one starts after it
    assert res["at_second_read"] == res["at_second_read_then_old_boundary"] == (N_REC, 0)
    assert res["at_second_read_then_new_boundary"][0] < N_REC and res["at_second_read_then_new_boundary"][1] == -14
    n_before = sum(1 for s in fills["starts"] if s < 150000)
    assert res["start_at_empty"] == (N_REC - n_before, 0)
    assert 0 < res["v_end_after_empty"][0] < N_REC and res["v_end_after_empty_at_fill"][0] == 5995


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_replays_the_fills(gpu_ctx, oracle_mod, fills, name):
    data, a, b = fills["files"][name]
    h = fills["h"]
    ref = oracle_mod.read_bcf_split(data, a, b, h)
    base = a >> 16
    got = gpu_ctx.bcf_decode_split(data[base:], h, a, b, comp_base=base, file_len=len(data))
    assert got["rc"] == 0, got
    assert (got["n"], got["status"]) == (ref["n"], ref["status"])
    assert np.array_equal(got["key"], ref["key"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["at_fill", "at_fill_plus_1", "v_end_after_empty_at_fill", "start_at_empty"])
def test_mirror_reads_what_the_oracle_reads(oracle_mod, fills, tmp_path, name):
    """BCFRecordReader (the mirror) over the same splits: the same keys, the oracle's exception, and
    a window no longer than the split's own bytes plus the first tail."""
    from hadoop_bam import bcf
    from hadoop_bam.formats import FileVirtualSplit
    data, a, b = fills["files"][name]
    ref = oracle_mod.read_bcf_split(data, a, b, fills["h"])
    path = tmp_path / "f.bcf"
    path.write_bytes(data)
    rr = bcf.VCFInputFormat().createRecordReader(FileVirtualSplit(str(path), a, b, []))
    keys, exc = bcf.record_keys(rr)
    assert np.array_equal(keys, ref["key"])
    if ref["status"] == 0:
        assert exc is None
    else:
        assert ref["status"] == -14 and isinstance(exc, bcf.TribbleException)
    assert rr.window_bytes <= min(len(data), (b >> 16) + bcf.BCF_WINDOW_TAIL) - (a >> 16)
