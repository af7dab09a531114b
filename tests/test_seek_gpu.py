"""The crafted seek cases (tests/seek_cases.py; their structure is asserted on the CPU in
test_seek_model.py) on the device: whichever way BlockCompressedInputStream.seek(vStart) goes,
hbam_decode_split and hbam_bcf_decode_split report the oracle's (n, status) and records."""
import pytest

import chain_craft as cc
import seek_cases as S
from helpers import assert_same_split
from test_chain_gpu import same_bcf

pytestmark = pytest.mark.gpu


def _params():
    return [pytest.param(fmt, i, id="%s-%d-%s" % (fmt, c.exit_no, c.name))
            for fmt in S.FMTS for i, c in enumerate(S.cases(fmt))]


@pytest.mark.parametrize("fmt,i", _params())
def test_seek_outcome(gpu_ctx, oracle_mod, fmt, i):
    case = S.cases(fmt)[i]
    if fmt == "bam":
        ref = oracle_mod.read_split(case.data, case.v_start, case.v_end, n_ref=cc.N_REF)
        # a call that ends in the seek leaves no columns (hbam_columns_to_host refuses the empty
        # struct): (n, status) from the device struct, the records where there are columns
        rc, d = gpu_ctx.decode_split_device(case.data, case.v_start, case.v_end, cc.N_REF)
        assert rc == 0, gpu_ctx.last_error()
        assert (int(d.n_records), int(d.status)) == (ref["n"], ref["status"])
        if case.exit_no == 8:
            got = gpu_ctx.decode_split(case.data, case.v_start, case.v_end, n_ref=cc.N_REF)
            assert got["rc"] == 0, got
            assert_same_split(got, ref)
    else:
        ref = oracle_mod.read_bcf_split_ex(case.data, case.v_start, case.v_end, case.h)
        got = gpu_ctx.bcf_decode_split(case.data, case.h, case.v_start, case.v_end, keep_data=True)
        same_bcf(got, ref)
    if case.exit_no == 8:
        assert (ref["n"], ref["status"]) == (S.N_RECORDS[case.name], 0)
    else:
        assert ref["n"] == 0
