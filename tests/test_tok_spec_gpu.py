"""The specialised symbol loop of the Huffman lane pass (k_inflate_tokens, inflate_tok.h tok_symbols)
on the device: the crafted blocks of tests/deflate_craft.py (every stream vouched for by zlib) through
Context.inflate(check_crc=True) with the lane pass forced (HBAM_WAVE_MAX_BLOCKS=0), once as is and
once with HBAM_TOK_GENERIC=1.  Bytes must be zlib's and statuses the same in both runs.

A wave takes the specialised body only when every lane that enters the loop fits, so besides one
call with every case in order (a mixed wave: the generic body), calls of 130 blocks (two full waves
and a tail) hold one wave of fitting blocks only (the specialised body runs, also over the two
corrupted copies) and one wave of fitting blocks with exactly one lane that does not fit, at lane 0,
31 or 63 (the whole wave must take the generic body)."""
import zlib

import numpy as np
import pytest

import deflate_craft as craft

pytestmark = pytest.mark.gpu

FIT = ["ll_min3", "ll_min4", "ll_max14", "ll_max15", "d_max9", "d_max10", "d_max11", "dyn_then_fixed",
       "dyn_then_stored"]
UNFIT = {0: "ll_min1", 31: "d_max12", 63: "d_single"}


def _call(members):
    """[(raw, inflated bytes or None, crc)] -> (file bytes, block table, expected bytes per block)"""
    data, blocks, want = b"", {"coff": [], "clen": [], "isize": [], "crc": []}, []
    for raw, u, crc, isize in members:
        m = craft.bgzf(raw, b"\0" * isize, crc=crc)
        blocks["coff"].append(len(data))
        blocks["clen"].append(len(m))
        blocks["isize"].append(isize)
        blocks["crc"].append(crc)
        data += m
        want.append(u)
    return (np.frombuffer(data + b"\0" * 64, np.uint8)[:len(data)],
            {k: np.array(v, np.uint64 if k == "coff" else np.uint32) for k, v in blocks.items()}, want)


@pytest.fixture(scope="module")
def runs():
    import torch  # noqa: F401  (its HIP runtime opens the device before libhbam's)
    from hadoop_bam import _lib
    cs = craft.cases()
    mem = {k: (raw, u, zlib.crc32(u), len(u)) for k, (raw, u, _) in cs.items()}
    base = cs["ll_min3"]
    soft, soft_u = craft.flipped(base[0], want_error=False)
    hard, _ = craft.flipped(base[0], want_error=True)
    mem["soft"] = (soft, soft_u, zlib.crc32(soft_u), len(soft_u))  # still DEFLATE: zlib's bytes for it
    mem["hard"] = (hard, None, zlib.crc32(base[1]), len(base[1]))  # zlib rejects it
    calls = {"cases": list(cs) + ["soft", "hard"]}
    for lane, bad in UNFIT.items():
        w0 = [FIT[i % len(FIT)] for i in range(64)]
        w0[5], w0[6] = "soft", "hard"
        w1 = [FIT[(i + 3) % len(FIT)] for i in range(64)]
        w1[lane] = bad
        calls["lane%d" % lane] = w0 + w1 + ["d_min2", "ll_min3"]
    built = {c: _call([mem[k] for k in names]) for c, names in calls.items()}
    mp = pytest.MonkeyPatch()
    got = {}
    try:
        mp.setenv("HBAM_WAVE_MAX_BLOCKS", "0")
        for gen in ("0", "1"):
            mp.setenv("HBAM_TOK_GENERIC", gen)
            ctx = _lib.Context(0)
            try:
                for c, (data, blocks, _) in built.items():
                    got[gen, c] = ctx.inflate(data, blocks, check_crc=True)
            finally:
                ctx.close()
    finally:
        mp.undo()
    return calls, built, got


@pytest.mark.parametrize("call", ["cases", "lane0", "lane31", "lane63"])
def test_crafted_blocks_inflate_to_zlib_bytes_in_both_bodies(runs, call):
    calls, built, got = runs
    names, (_, blocks, want) = calls[call], built[call]
    assert len(names) == (130 if call != "cases" else len(names))
    res = {}
    for gen in ("0", "1"):
        rc, u, off, st = got[gen, call]
        assert rc == 0
        for i, k in enumerate(names):
            if want[i] is None:
                assert int(st[i]) != 0, (call, gen, i, k)  # the flip zlib rejects
            else:
                assert int(st[i]) == 0, (call, gen, i, k, int(st[i]))
                assert u[int(off[i]):int(off[i + 1])].tobytes() == want[i], (call, gen, i, k)
        res[gen] = (np.asarray(st).copy(), np.asarray(off).copy())
    assert np.array_equal(res["0"][0], res["1"][0]) and np.array_equal(res["0"][1], res["1"][1])
