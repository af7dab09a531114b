"""The crafted BAM field cases (tests/bam_field_cases.py; their structure is asserted on the CPU in
test_bam_fields_model.py) on the device: hbam_decode_split's fixed columns, keys, layout flags, pool
offset columns (k_scan4_*) and pools (both loops of k_decode_pools) against the builder's own
pieces and against the oracle, and hbam_gather_records' payloads against the builder's record bytes.

Not covered: guard bytes behind the pools.  The library owns those allocations, so a store just
past a pool's end stays invisible here; a store inside a pool that lands on a neighbour's bytes is
seen, since every pool byte is compared."""
import numpy as np
import pytest

import bam_field_cases as B
import chain_craft as cc
from helpers import assert_same_split

pytestmark = pytest.mark.gpu


def first_diff(got, want):
    if got.shape != want.shape:
        return "length %d, expected %d" % (len(got), len(want))
    d = np.flatnonzero(got != want)
    return "%d elements differ, the first at %d: %s, expected %s" % (len(d), d[0], got[d[0]:d[0] + 8], want[d[0]:d[0] + 8])


def same(got, want, what):
    assert np.array_equal(got, want), "%s: %s" % (what, first_diff(np.asarray(got), np.asarray(want)))


@pytest.mark.parametrize("case_id", B.ALL_IDS)
def test_decode(gpu_ctx, oracle_mod, case_id):
    case = B.get(case_id)
    e = case.expect
    ref = oracle_mod.read_split(case.data, case.v_start, case.v_end)
    got = gpu_ctx.decode_split(case.data, case.v_start, case.v_end)
    assert got["rc"] == 0, got
    assert (got["n"], got["status"]) == (e["n"], 0)
    # the builder's expectation, directly
    for k in B.FIXED:
        same(got[k], e[k], k)
    same(got["key"], e["key"], "key")
    same(got["layout_ok"], e["layout_ok"], "layout_ok")
    for k in B.OFFS:                       # the running sums, the total at the end included
        assert got[k].dtype == np.uint64 and len(got[k]) == e["n"] + 1
        same(got[k], e[k], k)
    for k, dt in B.POOLS:
        assert got[k].dtype == dt
        same(got[k], e[k], "pool " + k)
    # and the oracle's
    assert_same_split(got, ref)


def test_key_edges_by_name(gpu_ctx):
    """Each edge's key against the value spelled out in the case."""
    case = B.key_edges()
    got = gpu_ctx.decode_split(case.data, case.v_start, case.v_end)
    assert got["rc"] == 0, got
    for label, (i, want) in case.notes["edges"].items():
        assert int(got["key"][i]) == want, (label, hex(int(got["key"][i]) & (1 << 64) - 1), hex(want & (1 << 64) - 1))
    e = case.notes["edges"]
    assert int(got["key"][e["twin_a"][0]]) == int(got["key"][e["twin_b"][0]])


def _orders(n):
    return [("reversed", np.arange(n - 1, -1, -1)), ("shuffled", np.random.default_rng(1360).permutation(n)),
            ("every_third", np.arange(0, n, 3))]


@pytest.mark.parametrize("case_id", ["length_grid", "unit_boundary-65535-lane32"])
def test_gather(gpu_ctx, case_id):
    """k_gather_records_tile: the records' SAMRecordWritable bytes in three orders."""
    case = B.get(case_id)
    rc, d = gpu_ctx.decode_split_device(case.data, case.v_start, case.v_end, cc.N_REF)
    assert rc == 0, gpu_ctx.last_error()
    n = int(d.n_records)
    assert (n, int(d.status)) == (len(case.recs), 0)
    for label, order in _orders(n):
        idx = gpu_ctx.upload(np.ascontiguousarray(order, np.uint32).view(np.uint8))
        try:
            voff, payload, off = gpu_ctx.gather_to_host(d, idx.ptr, len(order))
        finally:
            idx.free()
        want, want_off = case.payload(order)
        same(off, want_off, label + " offsets")
        same(payload, np.frombuffer(want, np.uint8), label + " payload")
        assert len(voff) == len(order)
