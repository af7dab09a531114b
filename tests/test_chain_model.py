"""The crafted chain-walk cases on the CPU: every case has the structure it claims (checked with
the host model of the entry finder, the walk and the stitch check, tests/chain_craft.py), the
model's repaired chain is the stream's real record chain, and the oracle reads what the builder
wrote.  The same cases run on the device in test_chain_gpu.py."""
import struct

import numpy as np
import pytest

import chain_cases as C
import chain_craft as cc
from helpers import bgzf_members

V = pytest.mark.parametrize("fmt,kind", C.VARIANTS)


def oracle_read(case, oracle):
    if case.fmt == "bam":
        return oracle.read_split(case.data, case.v_start, case.v_end)
    return oracle.read_bcf_split(case.data, case.v_start if case.bgzf else 0, case.v_end, case.h)


def check_truth(case, oracle, n=None, status=0):
    """The model's repaired chain is the plain sequential chain; the oracle reads the builder's
    records."""
    m = case.model()
    f = case.fmt_model()
    seq, r = [], case.r0
    while r not in (cc.CHAIN_STOP,) and r < len(case.u):
        seq.append(r)
        r = f.next(r, len(case.u))
    assert m["chain"] == seq
    ref = oracle_read(case, oracle)
    assert (ref["n"], ref["status"]) == (len(case.starts) if n is None else n, status), (ref["n"], ref["status"])
    assert m["chain"][:ref["n"]] == case.starts[:ref["n"]]
    return m, ref


def test_bgzf_pack_at_members():
    u = bytes(range(256)) * 40
    z = cc.bgzf_pack_at(u, [100, 5000, 5001], empties=(0, 2, 2, 4))
    mem = bgzf_members(z)
    assert [m[1] for m in mem] == [0, 100, 4900, 0, 0, 1, len(u) - 5001, 0, 0]
    assert all(m[2] for m in mem) and b"".join(m[0] for m in mem) == u
    coff, uoff = cc.bgzf_layout(z)
    assert uoff == [0, 0, 100, 5000, 5000, 5000, 5001, len(u), len(u), len(u)] and len(coff) == 9


def test_model_predicates_on_true_records():
    """Every true record of both builders is plausible (the guess of a block that starts on one
    is that record), minimum-size records are not."""
    for fmt in ("bam", "bcf"):
        s = C._stream(fmt)
        s.add_trues(100)
        u = s.bytes()
        f = cc.BamModel(u) if fmt == "bam" else cc.BcfModel(u)
        assert all(f.plausible(x, len(u)) for x in s.starts[:-3])
        assert all(f._cand[x] for x in s.starts[:-3])
        assert cc._entry(f, s.starts[5], s.starts[9], len(u)) == s.starts[5]
        assert cc._entry(f, s.starts[5] + 1, s.starts[9], len(u)) == s.starts[6]
    u = cc.bcf_header() + b"".join(cc.bcf_min_record(i) for i in range(10))
    assert not any(cc.BcfModel(u).plausible(x, len(u)) for x in range(len(u) - 40))
    u = cc.bam_header() + b"".join(cc.bam_min_record(i) for i in range(10))
    assert not any(cc.BamModel(u).plausible(x, len(u)) for x in range(len(u) - 40))


@V
def test_a_decoy_at_block_start(oracle_mod, fmt, kind):
    case = C.case_a(fmt, kind)
    m, _ = check_truth(case, oracle_mod)
    assert m["guess"][1] == case.decoys[0] and m["wrong"][1] and m["marked"][1]
    assert m["exit0"][1] == cc.CHAIN_STOP and m["count0"][1] == 6  # five decoys and the bytes that stop the chain
    assert m["marked"][2] and not m["wrong"][2]
    assert len(case.data) < 1 << 20


@V
def test_b_record_over_many_blocks(oracle_mod, fmt, kind):
    case = C.case_b(fmt, kind)
    m, _ = check_truth(case, oracle_mod)
    assert m["guess"][1:4] == [cc.NO_ENTRY] * 3 and m["count"][1:4] == [0, 0, 0]
    # the block the record ends in guesses the first plausible record, eight records too late
    assert m["guess"][4] == case.starts[case.starts.index(case.host_end) + 8] and m["marked"][4] and m["wrong"][4]
    assert m["entry"][4] == case.host_end == m["exit0"][0]


@V
def test_c_consistent_false_chain(oracle_mod, fmt, kind):
    case = C.case_c(fmt, kind)
    m, _ = check_truth(case, oracle_mod)
    assert m["marked"][1] and m["wrong"][1] and m["guess"][1] == case.decoys[0]
    assert m["guess"][2] == case.decoys[1] == m["exit0"][1]
    assert not m["marked"][2] and m["wrong"][2]          # unmarked but wrong
    assert not m["marked"][3] and not m["wrong"][3]      # the false chain lands on a true record
    assert m["heads"][0] == 1 and m["count0"][2] > 0 and m["count"][2] > 0


@V
def test_d_stale_exit(oracle_mod, fmt, kind):
    case = C.case_d(fmt, kind)
    m, _ = check_truth(case, oracle_mod)
    assert m["marked"][1] and m["wrong"][1]
    assert not m["marked"][2] and m["wrong"][2]
    # block 3 heads a run of its own; its predecessor's first (false) exit is a decoy chain in it
    assert m["marked"][3] and m["guess"][3] == case.decoys[2] and m["exit0"][2] == case.decoys[3]
    assert m["heads"][:2] == [1, 3]
    f = case.fmt_model()
    stale, ex = cc._walk(f, case.uoff[3], case.uoff[4], m["exit0"][2], len(case.u))
    assert len(stale) == 6 and ex == cc.CHAIN_STOP       # what a walk from the stale exit frames
    assert m["entry"][3] not in (m["guess"][3], m["exit0"][2])


@pytest.mark.parametrize("fmt", ["bam", "bcf"])
def test_e_many_runs(oracle_mod, fmt):
    case = C.case_e(fmt)
    m, _ = check_truth(case, oracle_mod)
    sizes = np.diff(case.uoff[1:-2])
    assert len(sizes) >= 200 and sizes.min() >= 512 and sizes.max() <= 1024, (len(sizes), sizes.min(), sizes.max())
    assert len(m["heads"]) > 64
    d = set(case.decoys)
    assert sum(1 for b in range(1, len(case.uoff) - 1) if m["guess"][b] in d and m["wrong"][b]) == len(d) == 110


@V
@pytest.mark.parametrize("hops", [1, 2, 3])
def test_f_decoy_reaches_the_end(oracle_mod, fmt, kind, hops):
    case = C.case_f(fmt, kind, hops)
    m, _ = check_truth(case, oracle_mod)
    assert m["guess"][1] == case.decoys[0] and m["wrong"][1] and m["marked"][1]
    assert m["exit0"][1] == len(case.u) and m["count0"][1] == hops


@V
@pytest.mark.parametrize("missing", [1, 7, 35, 37])
def test_f_cut_stream_model(oracle_mod, fmt, kind, missing):
    case = C.case_f_cut(fmt, kind, missing)
    m = case.model()
    assert m["chain"][:70] == case.starts
    ref = oracle_read(case, oracle_mod)
    assert ref["n"] == 69 and ref["status"] != 0


def test_g_full_block_bcf_plain(oracle_mod):
    case = C.case_g_plain()
    m, _ = check_truth(case, oracle_mod)
    assert m["guess"][1:] == [cc.NO_ENTRY] * 3                 # no entry guess in any block
    assert max(m["count"]) == 1873 <= cc.WALK_CAP and min(m["count"][1:3]) >= 1872
    assert len(case.u) <= 4 * 65536


@pytest.mark.parametrize("fmt", ["bam", "bcf"])
def test_g_full_block_bgzf(oracle_mod, fmt):
    case = C.case_g_full(fmt)
    m, _ = check_truth(case, oracle_mod)
    assert all(g == cc.NO_ENTRY for g in m["guess"][1:])
    assert case.uoff[1] - case.uoff[0] == 65536
    assert m["count"][0] == (1821 if fmt == "bam" else 1873)
    case = C.case_g_counts(fmt)
    m, _ = check_truth(case, oracle_mod)
    counts = C.g_counts(fmt)
    assert m["count"][:len(counts)] == counts and max(counts) * C._min_size(fmt) <= 65536 < (max(counts) + 1) * C._min_size(fmt)
    assert set(range(1, 9)) <= set(counts) and {n % 8 for n in counts if n > 8} == set(range(8))


@pytest.mark.parametrize("fmt", ["bam", "bcf"])
def test_h_size_field_split(oracle_mod, fmt):
    case = C.case_h_bgzf(fmt)
    check_truth(case, oracle_mod)
    nb = 4 if fmt == "bam" else 8
    inside = sorted(c - max(s for s in case.starts if s <= c) for c in case.cuts)
    assert inside[:nb] == list(range(nb)) and len(inside) == nb + 1   # offsets 0..nb-1, and the last byte of a record
    assert any(c + 1 in case.starts for c in case.cuts)


@pytest.mark.parametrize("k", list(range(-1, 8)))
def test_h_size_field_split_plain(oracle_mod, k):
    case = C.case_h_plain(k)
    check_truth(case, oracle_mod)
    assert (65536 - k) in case.starts


@pytest.mark.parametrize("fmt,kind,what", C.I_VARIANTS)
def test_i_unframeable_record(oracle_mod, fmt, kind, what):
    case = C.case_i(fmt, kind, what)
    m = case.model()
    ref = oracle_read(case, oracle_mod)
    assert ref["n"] == case.n_before and ref["status"] != 0
    b = case.block_of(case.bad)
    assert b == 1 and m["guess"][1] == case.decoys[0] and m["wrong"][1]
    # the first walk never reaches the bad record; the repaired chain ends at it
    assert m["chain"][-1] == case.bad and m["chain"][:-1] == case.starts[:case.n_before]
    assert m["exit"][1] == cc.CHAIN_STOP
    assert all(e == cc.CHAIN_STOP and n == 0 for e, n in zip(m["entry"][2:], m["count"][2:]))
    # ... although the later blocks have good guesses
    later = [g for g in m["guess"][2:] if g != cc.NO_ENTRY]
    assert later and all(g in case.starts for g in later)


def test_struct_sizes():
    assert len(cc.bam_min_record(0)) == 36 and len(cc.bcf_min_record(0)) == 35
    assert len(cc.bam_decoy()) == 38 and len(cc.bcf_decoy(43)) == 43
    assert struct.unpack_from("<i", cc.bam_decoy(100), 0)[0] == 96
