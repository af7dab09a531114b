"""The crafted consumer cases (tests/consumer_cases.py; what they declare and reach is asserted on the
CPU in test_consumer_model.py) on the device: hbam_summarize_ranges, hbam_name_order and hbam_fixmate
driven through the C ABI over hand-made hbam_columns and device tensors, against the oracle and against
each case's declaration, byte for byte, per case and over the product runs.

The input payload is the test's own tensor (test_merge_gpu.Split): the 64 spare bytes the kernels may
read behind it are there, filled with a pattern, and compared after every call with the payload itself:
the consumers read their input and never write it.  Not covered: guard bytes behind the outputs, which
the library allocates; every output element is compared, so a store onto a neighbour is seen.

The malformed-aux and overrun cases are refusals reported as a status.  Every read of f4_ranges, f4_end
and f4_encode is bounded by the record's block_size (f4_cigar_ok before the CIGAR walk, k_layout_check
before any name, CIGAR, sequence or aux read of FixMate, aux_len and f4_aux_vsize's avail inside the aux
walk), so these are ordinary inputs."""
import numpy as np
import pytest

import consumer_cases as K
from test_merge_gpu import Split, same

pytestmark = pytest.mark.gpu

SUM = K.cached(K.summarize_cases) + K.cached(K.summarize_product)
NAME = K.cached(K.name_cases) + K.cached(K.name_product)
FM = K.cached(K.fixmate_cases) + K.cached(K.fixmate_product)
NO_MATE = 0xffffffff


def by_id(cases, cid):
    return next(c for c in cases if c.id == cid)


def untouched(s, what):
    same(s.get("ubuf"), s.host, what + ": the input payload and the bytes behind it")
    same(s.get("rec_off").view(np.uint64), s.off, what + ": rec_off")


@pytest.mark.parametrize("cid", [c.id for c in SUM])
def test_summarize(gpu_ctx, oracle_mod, cid):
    case = by_id(SUM, cid)
    s = Split(case.recs)
    s.d.status = case.split_status
    got = gpu_ctx.summarize_ranges(s.d)
    # HBAM_EMORE is the ABI's own "not the split's last window": the reader raises nothing
    want = oracle_mod.summarize_ranges(s.pay, s.off, 0 if case.split_status == K.EMORE else case.split_status)
    for k in ("key", "beg", "end", "rev", "record"):
        same(got[k], want[k], "%s %s" % (cid, k))
    assert got["status"] == want["status"] == case.status
    assert list(zip(got["key"].tolist(), got["beg"].tolist(), got["end"].tolist(), got["rev"].tolist(), got["record"].tolist())) == case.ranges
    untouched(s, cid)


@pytest.mark.parametrize("cid", [c.id for c in NAME])
def test_name_order(gpu_ctx, oracle_mod, cid):
    import torch
    case = by_id(NAME, cid)
    s = Split(case.recs())
    perm = torch.full((s.n + 1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.name_order(s.t["ubuf"].data_ptr(), s.t["rec_off"].data_ptr(), s.n, perm.data_ptr() if s.n else 0)
    got = perm.cpu().numpy().view(np.uint32)
    same(got[:s.n], oracle_mod.name_order(s.pay, s.off), cid + " permutation")
    assert got[:s.n].tolist() == case.perm
    assert got[s.n] == 0x5a5a5a5a, "the element behind the permutation"
    untouched(s, cid)


@pytest.mark.parametrize("cid", [c.id for c in FM])
def test_fixmate(gpu_ctx, oracle_mod, cid):
    d = by_id(FM, cid).declared()
    s = Split(d["recs"])
    got = gpu_ctx.fixmate(s.t["ubuf"].data_ptr(), s.t["rec_off"].data_ptr(), s.n)
    want = oracle_mod.fixmate(s.pay, s.off)
    assert got["status"] == want["status"] == d["status"]
    same(got["src"], want["src"], cid + " src")
    same(got["offsets"], want["offsets"], cid + " offsets")
    same(got["payload"], want["payload"], cid + " payload")
    assert got["n_groups"] == d["n_groups"]
    assert got["src"].tolist() == [p[0] for p in d["plan"]]
    assert got["mate"].tolist() == [NO_MATE if p[1] is None else p[1] for p in d["plan"]]
    assert bytes(got["payload"]) == b"".join(d["outs"])
    untouched(s, cid)
