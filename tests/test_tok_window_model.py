"""The bit-cursor reader of the Huffman lane pass (inflate_tok.h EIn, ein_window) on the CPU model
(tools/cpu_model, one lane, a stand-alone program under MemorySanitizer): the crafted streams of
tests/tok_window_craft.py, every one vouched for by zlib, each decoded three ways: as is, with
HBAM_TOK_INTERIOR=0 and with HBAM_TOK_GENERIC=1.  Bytes must be zlib's, status and produced count
zlib's and the same in all three.  The model puts block b at address b mod 16, so the cases that
need a start phase are placed by their index (fillers in between)."""
import os
import re
import struct
import subprocess
import sys
import zlib

import pytest

import tok_window_craft as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("HBAM_MODEL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
WAYS = {"asis": {}, "no_interior": {"HBAM_TOK_INTERIOR": "0"}, "generic": {"HBAM_TOK_GENERIC": "1"}}
RC = {"ok": 0, "short": 1, "data": 2}  # INF_OK / INF_SHORT / INF_DATA
NAMES = list(wc.cases())


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ with MemorySanitizer")
    d = tmp_path_factory.mktemp("tok_window_model")
    sys.path.insert(0, os.path.join(ROOT, "tools/cpu_model"))
    import build as model_build
    exe = model_build.build(str(d), "cur")
    cs = wc.cases()
    placed = wc.place(NAMES, lambda i, pos: i, lambda n: 0)
    for i, (name, _, _) in enumerate(placed):
        assert name is None or cs[name][4] is None or cs[name][4] == i % 16, name
    path = str(d / "blocks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x4d544248, len(placed)))
        for name, raw, u in placed:
            isize = len(u) if name is None else cs[name][2]
            f.write(struct.pack("<II", len(raw), isize) + raw + (u if u is not None else b"\0" * isize))
    runs = {}
    for way, env in WAYS.items():
        e = {k: v for k, v in os.environ.items() if k not in ("HBAM_TOK_INTERIOR", "HBAM_TOK_GENERIC")}
        r = subprocess.run([exe, path, "-i"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                           env=dict(e, **env))
        assert "MemorySanitizer" not in r.stderr, r.stderr[-4000:]
        rows = [tuple(int(x) for x in m.groups()) for m in re.finditer(
            r"^block (\d+) rc (-?\d+) produced (\d+) ok (\d) generic (\d+) specialised (\d+)$", r.stdout, re.M)]
        its = [tuple(int(x) for x in m.groups()) for m in re.finditer(
            r"^iterations (\d+) generic (\d+) specialised (\d+) interior (\d+)$", r.stdout, re.M)]
        stalls = [tuple(int(x) for x in m.groups()) for m in re.finditer(
            r"^stalls (\d+) generic (\d+) specialised (\d+) interior (\d+)$", r.stdout, re.M)]
        assert len(rows) == len(placed) == len(its), r.stdout[-2000:]
        at = {name: i for i, (name, _, _) in enumerate(placed) if name is not None}
        runs[way] = ({k: rows[i] for k, i in at.items()}, {k: its[i] for k, i in at.items()},
                     {k: stalls[i] for k, i in at.items()} if len(stalls) == len(placed) else None,
                     [rows[i] for i, p in enumerate(placed) if p[0] is None])
    return cs, runs


@pytest.mark.parametrize("name", NAMES)
def test_stream_decodes_as_zlib_three_ways(model, name):
    cs, runs = model
    raw, u, isize, kind, _ = cs[name]
    for way in WAYS:
        _, rc, produced, ok, _, _ = runs[way][0][name]
        assert rc == RC[kind], (name, way, rc)
        if kind == "ok":
            assert (produced, ok) == (isize, 1), (name, way)  # ok: the bytes equal zlib's
        else:
            assert ok == 0 and produced < isize, (name, way)
        assert (rc, produced) == runs["asis"][0][name][1:3], (name, way)
    if kind == "short":  # as many bytes as zlib gives before it asks for more input
        assert runs["asis"][0][name][2] == len(zlib.decompressobj(-15).decompress(raw)), name


def test_fillers_decode(model):
    for way in WAYS:
        assert all(r[1] == 0 and r[3] == 1 for r in model[1][way][3]), way


def test_loops_the_cases_are_meant_for(model):
    """bits1 and wide_generic run in the generic loop, wide_spec and the start streams in the
    specialised one; the same iterations whichever body runs them."""
    cs, runs = model
    for name in NAMES:
        if cs[name][3] != "ok":
            continue
        _, gen, spec, inner = runs["asis"][1][name]
        if name in ("bits1", "wide_generic"):
            assert gen > 0 and spec + inner == 0, name
        if name == "wide_spec" or name.startswith("start"):
            assert gen == 0 and inner > 0, name
        assert runs["no_interior"][1][name][1:] == (gen, spec + inner, 0), name
        assert runs["generic"][1][name][1:] == (gen + spec + inner, 0, 0), name
    # 640 literals at two an iteration at the most, and one (the careful symbol) in the last 64 bits
    assert 320 <= runs["asis"][1]["bits1"][1] <= 320 + 64


def test_wide_iterations_outrun_the_banks(model):
    """70 iterations of b = 56 / 63 bits read 70 b bits.  The two banks hold 256 and an epoch, every
    TOK_K = 4 loop iterations, brings 128, so the 70 take at least (70 b - 256) / 32 loop iterations:
    130 for b = 63 and 115 for b = 56.  What exceeds 70 the lane skips (the stall path), and it
    comes back each time: the bytes are zlib's (above)."""
    cs, runs = model
    assert runs["asis"][2] is not None, "the model prints no stalls"
    for name, col, least in (("wide_generic", 1, 130 - 70), ("wide_spec", 3, 115 - 70)):
        assert runs["asis"][2][name][col] >= least, (name, runs["asis"][2][name])
