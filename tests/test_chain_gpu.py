"""The crafted chain-walk cases (tests/chain_cases.py; their structure is asserted on the CPU in
test_chain_model.py) on the device: hbam_decode_split and hbam_bcf_decode_split must report exactly
the oracle's records whatever the entry finder guessed, and the split guessers must see through the
same decoys."""
import numpy as np
import pytest

import chain_cases as C
import chain_craft as cc
from helpers import assert_same_split

pytestmark = pytest.mark.gpu
V = pytest.mark.parametrize("fmt,kind", C.VARIANTS)

BCF_COLS = ("rel", "chrom", "pos", "key", "l_shared", "l_indiv", "rlen", "qual", "n_allele_info", "n_fmt_sample")


def same_bcf(got, ref):
    assert got["rc"] == 0, got
    assert (got["n"], got["status"]) == (ref["n"], ref["status"])
    for k in BCF_COLS:
        assert np.array_equal(got[k], ref[k]), k
    recs = b"".join(bytes(got["data"][int(o):int(o) + 8 + int(ls) + int(li)])
                    for o, ls, li in zip(got["rec_off"], got["l_shared"], got["l_indiv"]))
    assert recs == ref["bytes"]


def check(ctx, oracle, case):
    """The device's records of the case's split equal the oracle's: every column, the pools (BAM),
    the record bytes (BCF)."""
    if case.fmt == "bam":
        ref = oracle.read_split(case.data, case.v_start, case.v_end)
        got = ctx.decode_split(case.data, case.v_start, case.v_end)
        assert got["rc"] == 0, got
        assert_same_split(got, ref)
    else:
        ref = oracle.read_bcf_split_ex(case.data, case.v_start, case.v_end, case.h)
        got = ctx.bcf_decode_split(case.data, case.h, case.v_start, case.v_end, keep_data=True)
        same_bcf(got, ref)
    return ref


@V
def test_a_decoy_at_block_start(gpu_ctx, oracle_mod, fmt, kind):
    assert check(gpu_ctx, oracle_mod, C.case_a(fmt, kind))["status"] == 0


@V
def test_b_record_over_many_blocks(gpu_ctx, oracle_mod, fmt, kind):
    assert check(gpu_ctx, oracle_mod, C.case_b(fmt, kind))["status"] == 0


@V
def test_c_consistent_false_chain(gpu_ctx, oracle_mod, fmt, kind):
    assert check(gpu_ctx, oracle_mod, C.case_c(fmt, kind))["status"] == 0


@V
def test_d_stale_exit(gpu_ctx, oracle_mod, fmt, kind):
    """Whether the parallel pass walked block 3 from the stale exit or the fresh one cannot be
    seen from outside; the records must be the oracle's either way."""
    assert check(gpu_ctx, oracle_mod, C.case_d(fmt, kind))["status"] == 0


@pytest.mark.parametrize("fmt", ["bam", "bcf"])
def test_e_many_runs(gpu_ctx, oracle_mod, fmt):
    assert check(gpu_ctx, oracle_mod, C.case_e(fmt))["status"] == 0


@V
@pytest.mark.parametrize("hops", [1, 2, 3])
def test_f_decoy_reaches_the_end(gpu_ctx, oracle_mod, fmt, kind, hops):
    assert check(gpu_ctx, oracle_mod, C.case_f(fmt, kind, hops))["status"] == 0


@V
@pytest.mark.parametrize("missing", [1, 7, 35, 37])
def test_f_cut_stream(gpu_ctx, oracle_mod, fmt, kind, missing):
    ref = check(gpu_ctx, oracle_mod, C.case_f_cut(fmt, kind, missing))
    assert ref["n"] == 69 and ref["status"] != 0


def test_g_full_block_bcf_plain(gpu_ctx, oracle_mod):
    ref = check(gpu_ctx, oracle_mod, C.case_g_plain())
    assert ref["n"] == len(C.case_g_plain().starts)


@pytest.mark.parametrize("fmt", ["bam", "bcf"])
@pytest.mark.parametrize("which", ["full", "counts"])
def test_g_full_block_bgzf(gpu_ctx, oracle_mod, fmt, which):
    case = C.case_g_full(fmt) if which == "full" else C.case_g_counts(fmt)
    ref = check(gpu_ctx, oracle_mod, case)
    assert (ref["n"], ref["status"]) == (len(case.starts), 0)


@pytest.mark.parametrize("fmt", ["bam", "bcf"])
def test_h_size_field_split(gpu_ctx, oracle_mod, fmt):
    assert check(gpu_ctx, oracle_mod, C.case_h_bgzf(fmt))["status"] == 0


@pytest.mark.parametrize("k", list(range(-1, 8)))
def test_h_size_field_split_plain(gpu_ctx, oracle_mod, k):
    assert check(gpu_ctx, oracle_mod, C.case_h_plain(k))["status"] == 0


@pytest.mark.parametrize("fmt,kind,what", C.I_VARIANTS)
def test_i_unframeable_record(gpu_ctx, oracle_mod, fmt, kind, what):
    case = C.case_i(fmt, kind, what)
    ref = check(gpu_ctx, oracle_mod, case)
    assert ref["n"] == case.n_before and ref["status"] != 0


# ---- j: the same files read from a window that starts after the file's start ----------------------------
@V
@pytest.mark.parametrize("which", ["a", "c"])
def test_j_windowed_decode(gpu_ctx, oracle_mod, fmt, kind, which):
    case = (C.case_a if which == "a" else C.case_c)(fmt, kind, lead=(kind == "bgzf"))
    data = case.data
    if case.bgzf:
        # the window starts at the block before the decoy's; the split at the first record in it
        b = case.block_of(case.decoys[0]) - 1
        assert b >= 0
        first = min(x for x in case.starts if x >= case.uoff[b] and x >= case.header_len)
        assert first < case.uoff[b + 1]
        base = case.coff[b]
        assert base > 0
        m = cc.model(case.fmt_model(), case.uoff[b:], first, len(case.u))
        assert m["guess"][1] == case.decoys[0] and m["wrong"][1]  # the window's second block starts on the decoy
        v_start = base << 16 | (first - case.uoff[b])
        if fmt == "bam":
            ref = oracle_mod.read_split(data, v_start, case.v_end)
            got = gpu_ctx.decode_split(data[base:], v_start, case.v_end, n_ref=cc.N_REF, comp_base=base,
                                       file_len=len(data))
            assert got["rc"] == 0, got
            assert_same_split(got, ref)
        else:
            ref = oracle_mod.read_bcf_split_ex(data, v_start, case.v_end, case.h)
            got = gpu_ctx.bcf_decode_split(data[base:], case.h, v_start, case.v_end, comp_base=base,
                                           file_len=len(data), keep_data=True)
            same_bcf(got, ref)
        n_skipped = sum(1 for x in case.starts if x < first)
    else:
        # segments are cut relative to the window, so the decoys now sit in the middle of one
        base = 10007
        first = min(x for x in case.starts if x >= base)
        assert all((d - base) % 65536 > 1000 for d in case.decoys)
        ref = oracle_mod.read_bcf_split_ex(data, first, len(data) - first, case.h)
        got = gpu_ctx.bcf_decode_split(data[base:], case.h, first, len(data) - first, comp_base=base,
                                       file_len=len(data), keep_data=True)
        same_bcf(got, ref)
        n_skipped = sum(1 for x in case.starts if x < first)
    assert (ref["n"], ref["status"]) == (len(case.starts) - n_skipped, 0)


# ---- the split guessers over the decoys --------------------------------------------------------------------
def _guess_offsets(case):
    """beg at each decoy, one byte before and one after: file offsets (BGZF: the decoy sits at the
    start of its block)."""
    out = []
    for d in case.decoys:
        if case.bgzf:
            b = case.block_of(d)
            p = case.coff[b] if case.uoff[b] == d else None
            if p is None:
                continue
        else:
            p = d
        out += [p - 1, p, p + 1]
    assert out
    return np.array(out, np.int64)


@V
@pytest.mark.parametrize("which", ["a", "c"])
def test_guessers_reject_the_decoys(gpu_ctx, oracle_mod, fmt, kind, which):
    """The decoys pass the guessers' candidate scans and must fall to their verification decode:
    every guess equals the oracle's."""
    case = (C.case_a if which == "a" else C.case_c)(fmt, kind)
    data, n = case.data, len(case.data)
    beg = _guess_offsets(case)
    for end in (np.full(len(beg), n, np.int64), np.minimum(beg + 3000, n)):
        if fmt == "bam":
            wl = [gpu_ctx.guess_window_len(n, int(b), int(e)) for b, e in zip(beg, end)]
        else:
            wl = [gpu_ctx.guess_bcf_window_len(n, int(b), int(e), case.bgzf) for b, e in zip(beg, end)]
        off = np.zeros(len(beg) + 1, np.uint64)
        off[1:] = np.cumsum(wl)
        w = b"".join(bytes(data[int(b):int(b) + k]) for b, k in zip(beg, wl))
        if fmt == "bam":
            rc, out, err = gpu_ctx.guess_windows(w, off, n, beg, end, cc.N_REF)
        else:
            rc, out, err = gpu_ctx.guess_bcf_windows(w, off, n, beg, end, case.h)
        assert rc == 0, gpu_ctx.last_error()
        for i in range(len(beg)):
            if fmt == "bam":
                g, e = oracle_mod.guess_bam_record_start(data, int(beg[i]), int(end[i]), cc.N_REF)
            else:
                g, e = oracle_mod.guess_bcf_record_start(data, int(beg[i]), int(end[i]), case.h)
            assert (int(out[i]), int(err[i])) == (g, e), (i, int(beg[i]), int(end[i]))
