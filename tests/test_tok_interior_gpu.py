"""The interior body of the specialised symbol loop (k_inflate_tokens, inflate_tok.h tok_symbols) on
the device: the crafted blocks of tests/tok_interior_craft.py (every stream vouched for by zlib)
through Context.inflate(check_crc=True) with the lane pass forced (HBAM_WAVE_MAX_BLOCKS=0), three
ways: as is, with HBAM_TOK_INTERIOR=0 and with HBAM_TOK_GENERIC=1.  Bytes must be zlib's and
statuses and output offsets the same in all three.

A wave leaves the interior body as soon as one running lane comes near an end and returns to it
when that lane has ended, so besides one call with every case in order (lanes leave at different
iterations, packets pending in the others), calls of exactly one wave hold 63 long blocks and one
short block at lane 0, 31 or 63 (the wave leaves while 63 lanes are mid-block, and comes back), and
the reverse, one long lane among short ones."""
import zlib

import numpy as np
import pytest

import deflate_craft as craft
import tok_interior_craft as ic

pytestmark = pytest.mark.gpu

WAYS = {"asis": {}, "no_interior": {"HBAM_TOK_INTERIOR": "0"}, "generic": {"HBAM_TOK_GENERIC": "1"}}
SHORT = {0: "n1", 31: "n259", 63: "n263"}
CALLS = ["cases", "short0", "short31", "short63", "long17"]


def _call(members):
    """[(raw, inflated bytes or None, crc, isize)] -> (file bytes, block table, expected bytes per block)"""
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
    cs = ic.cases()
    mem = {k: (raw, u, zlib.crc32(u), len(u)) for k, (raw, u) in cs.items()}
    (soft, soft_u), (hard, _) = ic.corrupted(cs["far"][0])
    mem["soft"] = (soft, soft_u, zlib.crc32(soft_u), len(soft_u))  # still DEFLATE: zlib's bytes for it
    mem["hard"] = (hard, None, zlib.crc32(cs["far"][1]), len(cs["far"][1]))  # zlib rejects it
    calls = {"cases": list(cs) + ["soft", "hard"]}
    for lane, short in SHORT.items():
        w = ["n4096"] * 64
        w[lane] = short
        calls["short%d" % lane] = w
    shorts = ["n1", "n259", "n260", "n261", "n262", "n263", "hand_mark", "tail1"]
    w = [shorts[i % len(shorts)] for i in range(64)]
    w[17] = "n4096"
    calls["long17"] = w
    built = {c: _call([mem[k] for k in names]) for c, names in calls.items()}
    mp = pytest.MonkeyPatch()
    got = {}
    try:
        mp.setenv("HBAM_WAVE_MAX_BLOCKS", "0")
        for way, env in WAYS.items():
            mp.delenv("HBAM_TOK_INTERIOR", raising=False)
            mp.delenv("HBAM_TOK_GENERIC", raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            ctx = _lib.Context(0)
            try:
                for c, (data, blocks, _) in built.items():
                    got[way, c] = ctx.inflate(data, blocks, check_crc=True)
            finally:
                ctx.close()
    finally:
        mp.undo()
    return calls, built, got


@pytest.mark.parametrize("call", CALLS)
def test_crafted_blocks_inflate_to_zlib_bytes_three_ways(runs, call):
    calls, built, got = runs
    names, (_, blocks, want) = calls[call], built[call]
    assert call == "cases" or len(names) == 64
    res = {}
    for way in WAYS:
        rc, u, off, st = got[way, call]
        assert rc == 0
        for i, k in enumerate(names):
            if want[i] is None:
                assert int(st[i]) != 0, (call, way, i, k)  # the flip zlib rejects
            else:
                assert int(st[i]) == 0, (call, way, i, k, int(st[i]))
                assert u[int(off[i]):int(off[i + 1])].tobytes() == want[i], (call, way, i, k)
        res[way] = (np.asarray(st).copy(), np.asarray(off).copy())
    for way in ("no_interior", "generic"):
        assert np.array_equal(res["asis"][0], res[way][0]) and np.array_equal(res["asis"][1], res[way][1]), way
