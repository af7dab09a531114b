"""The bit-cursor reader of the Huffman lane pass (k_inflate_tokens, inflate_tok.h EIn, ein_window)
on the device: the crafted streams of tests/tok_window_craft.py (every one vouched for by zlib)
through Context.inflate(check_crc=True) with the lane pass forced (HBAM_WAVE_MAX_BLOCKS=0), three
ways: as is, with HBAM_TOK_INTERIOR=0 and with HBAM_TOK_GENERIC=1.  Bytes must be zlib's, a stream
zlib cannot finish must fail, and statuses and output offsets must be the same in all three.

Every call is exactly one wave of 64 members.  The whole set goes in file order, 64 members a call,
filler members of chosen lengths in front of the streams that need their first byte at a given
address mod 16, and 4 KiB members in the lanes left over; then the widest iterations sit at lane 0,
31 and 63 among 63 long members (the lane stalls and comes back while the others run on), and
one long lane sits among short ones."""
import zlib

import numpy as np
import pytest

import deflate_craft as craft
import tok_window_craft as wc

pytestmark = pytest.mark.gpu

WAYS = {"asis": {}, "no_interior": {"HBAM_TOK_INTERIOR": "0"}, "generic": {"HBAM_TOK_GENERIC": "1"}}


def _layout():
    """call name -> [(case name / None for a filler / "long", raw, bytes or None, ISIZE)], 64 each"""
    cs = wc.cases()
    lraw, lu = wc.long_member()
    long_ = ("long", lraw, lu, len(lu))
    calls, names, k = {}, list(cs), 0
    while names:
        # as many cases as fit in 64 members with their fillers; the file starts at a 16-byte edge
        take = len(names)
        while True:
            placed = wc.place(names[:take], lambda i, pos: pos + 18, lambda n: n + 26)
            if len(placed) <= 64:
                break
            take -= 1
        mem = [(n, raw, u, len(u) if n is None else cs[n][2]) for n, raw, u in placed]
        calls["set%d" % k] = mem + [long_] * (64 - len(mem))
        names, k = names[take:], k + 1
    for lane in (0, 31, 63):
        for name in ("wide_generic", "wide_spec"):
            w = [long_] * 64
            w[lane] = (name,) + cs[name][:3]
            calls["%s_lane%d" % (name, lane)] = w
    shorts = ["short2", "short17", "short40", "end_on", "bits1", "pad0", "cut1", "stored_ph4"]
    w = [(n,) + cs[n][:3] for n in (shorts[i % len(shorts)] for i in range(64))]
    w[17] = long_
    calls["long17"] = w
    return calls


CALLS = _layout()


def _file(members):
    data, blocks = b"", {"coff": [], "clen": [], "isize": [], "crc": []}
    for _, raw, u, isize in members:
        crc = zlib.crc32(u) if u is not None else 0
        m = craft.bgzf(raw, b"\0" * isize, crc=crc)
        blocks["coff"].append(len(data))
        blocks["clen"].append(len(m))
        blocks["isize"].append(isize)
        blocks["crc"].append(crc)
        data += m
    return (np.frombuffer(data + b"\0" * 64, np.uint8)[:len(data)],
            {k: np.array(v, np.uint64 if k == "coff" else np.uint32) for k, v in blocks.items()})


@pytest.fixture(scope="module")
def runs():
    import torch  # noqa: F401  (its HIP runtime opens the device before libhbam's)
    from hadoop_bam import _lib
    built = {c: _file(m) for c, m in CALLS.items()}
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
                for c, (data, blocks) in built.items():
                    got[way, c] = ctx.inflate(data, blocks, check_crc=True)
            finally:
                ctx.close()
    finally:
        mp.undo()
    return built, got


def test_every_case_is_in_a_call_at_its_phase():
    cs, seen = wc.cases(), set()
    for c, members in CALLS.items():
        assert len(members) == 64, c
        pos = 0
        for name, raw, _, _ in members:
            if name in cs:
                seen.add(name)
                if c.startswith("set") and cs[name][4] is not None:
                    assert (pos + 18) % 16 == cs[name][4], (c, name)
            pos += len(raw) + 26
    assert seen == set(cs)


@pytest.mark.parametrize("call", list(CALLS))
def test_streams_inflate_to_zlib_bytes_three_ways(runs, call):
    built, got = runs
    res = {}
    for way in WAYS:
        rc, u, off, st = got[way, call]
        assert rc == 0
        for i, (name, _, want, _) in enumerate(CALLS[call]):
            if want is None:
                assert int(st[i]) != 0, (call, way, i, name)  # zlib cannot finish it either
            else:
                assert int(st[i]) == 0, (call, way, i, name, int(st[i]))
                assert u[int(off[i]):int(off[i + 1])].tobytes() == want, (call, way, i, name)
        res[way] = (np.asarray(st).copy(), np.asarray(off).copy())
    for way in ("no_interior", "generic"):
        assert np.array_equal(res["asis"][0], res[way][0]) and np.array_equal(res["asis"][1], res[way][1]), way
