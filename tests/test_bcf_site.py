"""The BCF2 site decode against stated answers (tests/bcf_site_cases.py): the oracle on the CPU,
bcf_site / bcf_typed (csrc/hbam_bcf.hip) through hbam_bcf_decode_split on the device.

The answers follow the rules listed at the top of oracle/hbam_oracle_bcf.c, which restate a subset of
htsjdk's BCF2Codec.  htsjdk itself is not available here, so this table pins both implementations to
the stated rules, not to htsjdk: parity of the site decode with htsjdk remains unpinned."""
import numpy as np
import pytest

import bcf_site_cases as S
import chain_craft as cc

H = dict(n_contig=S.N_CONTIG, n_sample=S.N_SAMPLE, n_dict=S.N_DICT, header_len=S.HEADER_LEN)
CASE = pytest.mark.parametrize("label,record,status", S.CASES, ids=S.LABELS)


def test_table_header_is_the_stated_one(oracle_mod):
    h = oracle_mod.bcf_header(S.HEAD)
    assert {k: h[k] for k in H} == H and not h["bgzf"]
    for t in (0, 4, 6, 8, 15):  # the table has every kind of row the decode distinguishes
        assert "type_%d_count_1" % t in S.LABELS
    assert {st for _, _, st in S.CASES} == {S.OK, S.TRIBBLE, S.RUNTIME}


@CASE
def test_oracle_gives_the_stated_answer(oracle_mod, label, record, status):
    u, off = S.stream(record)
    h = dict(H, bgzf=False)
    ref = oracle_mod.read_bcf_split(u, 0, len(u), h)
    assert (ref["n"], ref["status"]) == S.expected(label, status)
    assert list(ref["rel"][:S.K + 1]) == (list(_starts(u)) + [off])[:ref["n"]]


def _starts(u):
    p = S.HEADER_LEN
    for _ in range(S.K):
        yield p
        p += 8 + int.from_bytes(u[p:p + 4], "little") + int.from_bytes(u[p + 4:p + 8], "little")


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "bgzf"])
@CASE
def test_device_gives_the_stated_answer(gpu_ctx, oracle_mod, label, record, status, packed):
    u, off = S.stream(record)
    h = dict(H, bgzf=packed)
    if packed:
        data = cc.bgzf_pack_at(u, [off + max(1, min(5, len(record) - 1))])  # a cut inside the crafted record
        start, end = S.HEADER_LEN, len(data) << 16 | 0xffff
    else:
        data, start, end = u, 0, len(u)
    got = gpu_ctx.bcf_decode_split(data, h, start, end)
    assert got["rc"] == 0, got
    assert (got["n"], got["status"]) == S.expected(label, status)
    ref = oracle_mod.read_bcf_split(data, start, end, h)
    for k in ("rel", "chrom", "pos", "key"):
        assert np.array_equal(got[k], ref[k]), k
