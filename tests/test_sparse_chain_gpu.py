"""The sparse chain build on the device over the crafted files of tests/sparse_chain_cases.py (their
structure is asserted on the CPU in test_sparse_chain_model.py).  For every case: the block table
of a context that tries the sparse form (HBAM_CHAIN_SEG = the case's segment size) equals the
table of a context forced onto the dense path (HBAM_CHAIN_DENSE=1) in every field, both equal the
oracle's block list, the sparse form was taken or left exactly as the model says (and for the
model's reason), and the split decodes to the same columns through both."""
import os
import struct

import numpy as np
import pytest

import chain_craft as cc
import sparse_chain_cases as S

pytestmark = pytest.mark.gpu

KNOBS = ("HBAM_CHAIN_SEG", "HBAM_CHAIN_MIN", "HBAM_CHAIN_DENSE")


def make_ctx(**env):
    """A context created under the given chain knobs (read once, at creation)."""
    import torch  # noqa: F401  (its HIP runtime opens the device before libhbam's)
    from hadoop_bam import _lib
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        return _lib.Context(0)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def dense_ctx():
    c = make_ctx(HBAM_CHAIN_DENSE=1)
    yield c
    c.close()


def same_table(a, b):
    assert (a["nb"], a["end_pos"], a["end_code"]) == (b["nb"], b["end_pos"], b["end_code"])
    for k in ("coff", "clen", "isize", "crc"):
        assert np.array_equal(a[k], b[k]), k


def same_decode(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "timing":
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_sparse_equals_dense_equals_oracle(dense_ctx, oracle_mod, name):
    c = S.by_name()[name]
    m = c.model()
    sparse_ctx = make_ctx(HBAM_CHAIN_SEG=c.seg)
    try:
        ts = sparse_ctx.chain_table(c.window, c.start, c.file_end)
        td = dense_ctx.chain_table(c.window, c.start, c.file_end)
        # which path answered, and why
        assert (ts["sparse"], ts["fallback_flags"]) == (int(m["sparse"]), m["flags"])
        assert (td["sparse"], td["fallback_flags"]) == (0, 0)
        same_table(ts, td)
        # the true chain: a plain walk from the start, and the oracle's block list
        coff, end_pos = c.truth()
        w = c.window
        assert ts["coff"].tolist() == coff and ts["end_pos"] == end_pos
        clen = [struct.unpack_from("<H", w, p + 16)[0] + 1 for p in coff]
        assert ts["clen"].tolist() == clen
        assert ts["crc"].tolist() == [struct.unpack_from("<I", w, p + n - 8)[0] for p, n in zip(coff, clen)]
        assert ts["isize"].tolist() == [struct.unpack_from("<I", w, p + n - 4)[0] for p, n in zip(coff, clen)]
        ref = oracle_mod.scan_blocks(np.frombuffer(w[c.start:], np.uint8))
        if isinstance(ref, dict):
            assert end_pos == len(w) and (ref["coff"] + np.uint64(c.start)).tolist() == coff
            for k in ("clen", "isize", "crc"):
                assert np.array_equal(ref[k], ts[k]), k
            assert ts["end_code"] == (S.HBAM_EEOF if c.file_end else S.HBAM_EMORE)
        else:
            assert c.start + ref[1] == end_pos
            assert ts["end_code"] != S.HBAM_EEOF
        if not c.file_end:
            assert ts["end_code"] == S.HBAM_EMORE
        # the decode of the split through both
        a = (c.window, c.v_start, c.v_end)
        kw = dict(n_ref=cc.N_REF, comp_base=c.comp_base, file_len=c.file_len)
        gs, gd = sparse_ctx.decode_split(*a, **kw), dense_ctx.decode_split(*a, **kw)
        same_decode(gs, gd)
        # one chain build by chain_table, one by the decode
        assert sparse_ctx.chain_counters() == ((2, 0) if m["sparse"] else (0, 2))
        if m["sparse"] and name not in ("truncated_body", "truncated_header", "truncated_member"):
            assert gs["rc"] == 0 and gs["n"] > 0
            assert gs["status"] == (0 if c.file_end else S.HBAM_EMORE)
    finally:
        sparse_ctx.close()


def test_default_context_keeps_small_windows_dense(gpu_ctx):
    """Without the knobs only windows of 256 MiB and more try the sparse form."""
    c = S.case_boundary("exact")
    t = gpu_ctx.chain_table(c.window)
    assert (t["sparse"], t["fallback_flags"]) == (0, 0) and t["coff"].tolist() == c.truth()[0]


def test_min_knob_applies_beside_the_segment_knob():
    c = S.case_boundary("exact")
    ctx = make_ctx(HBAM_CHAIN_SEG=c.seg, HBAM_CHAIN_MIN=len(c.window) + 1)
    try:
        assert ctx.chain_table(c.window)["sparse"] == 0
    finally:
        ctx.close()
    ctx = make_ctx(HBAM_CHAIN_SEG=c.seg, HBAM_CHAIN_MIN=len(c.window))
    try:
        assert ctx.chain_table(c.window)["sparse"] == 1
    finally:
        ctx.close()
