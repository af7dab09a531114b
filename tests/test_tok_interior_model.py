"""The interior body of the specialised symbol loop (inflate_tok.h tok_symbols) on the CPU model
(tools/cpu_model, one lane, a stand-alone program under MemorySanitizer): the crafted blocks of
tests/tok_interior_craft.py, every stream vouched for by zlib, each decoded three ways: as is, with
HBAM_TOK_INTERIOR=0 (the specialised loop without the interior body) and with HBAM_TOK_GENERIC=1
(the generic loop).  Bytes, status and produced count must be the same in all three and zlib's;
the model's per-body iteration counters (-i) must show that the interior body runs where a lane is
far from both ends and nowhere else."""
import os
import re
import struct
import subprocess
import sys

import pytest

import tok_interior_craft as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("HBAM_MODEL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
WAYS = {"asis": {}, "no_interior": {"HBAM_TOK_INTERIOR": "0"}, "generic": {"HBAM_TOK_GENERIC": "1"}}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ with MemorySanitizer")
    d = tmp_path_factory.mktemp("tok_interior_model")
    sys.path.insert(0, os.path.join(ROOT, "tools/cpu_model"))
    import build as model_build
    exe = model_build.build(str(d), "cur")
    cs = ic.cases()
    names = list(cs)
    recs = [cs[k] for k in names]
    (soft, soft_u), (hard, _) = ic.corrupted(cs["far"][0])
    recs += [(soft, soft_u), (hard, cs["far"][1])]
    path = str(d / "blocks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x4d544248, len(recs)))
        for raw, u in recs:
            f.write(struct.pack("<II", len(raw), len(u)) + raw + u)
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
        assert len(rows) == len(recs) == len(its), r.stdout
        runs[way] = (rows, its)
    return cs, names, runs


@pytest.mark.parametrize("name", list(ic.cases()))
def test_block_inflates_to_zlib_bytes_three_ways(model, name):
    cs, names, runs = model
    i = names.index(name)
    nblocks = 2 if name in ic.TWO else 1  # Huffman-coded DEFLATE blocks
    for way in WAYS:
        _, rc, produced, ok, gen, spec = runs[way][0][i]
        assert (rc, produced, ok) == (0, len(cs[name][1]), 1), (name, way)  # ok: bytes equal zlib's
        assert (gen, spec) == ((nblocks, 0) if way == "generic" else (0, nblocks)), (name, way)


def test_interior_body_runs_far_from_the_ends_only(model):
    cs, names, runs = model
    for i, name in enumerate(names):
        isize = len(cs[name][1])
        _, gen, spec, inner = runs["asis"][1][i]
        assert gen == 0, name
        if isize < ic.ITER_OUT:
            assert inner == 0 and spec > 0, (name, spec, inner)
        if name == "n4096":
            assert inner > 0 and spec > 0, (name, spec, inner)  # and the loop's last iterations outside it
        # the same iterations in all, wherever they run
        _, gen0, spec0, inner0 = runs["no_interior"][1][i]
        assert (gen0, inner0) == (0, 0) and spec0 == spec + inner, name
        _, gen1, spec1, inner1 = runs["generic"][1][i]
        assert (spec1, inner1) == (0, 0) and gen1 == spec + inner, name


def test_hand_over_happens_at_the_crafted_iteration(model):
    """The pending-packet cases leave the interior body after exactly 151 iterations (150 of two
    literals and the one whose packet crosses); the bit cases leave it on the stream's end while
    the output is still far from its own."""
    cs, names, runs = model
    for name in ("hand_mark", "hand_plain"):
        assert runs["asis"][1][names.index(name)][3] == 151, name
    for name in ("bits63", "bits64", "bits65"):
        toks_tops = ic.iteration_tops(ic._bits_case(int(name[4:])))
        _, _, spec, inner = runs["asis"][1][names.index(name)]
        assert 0 < inner < len(toks_tops) and spec > 0, (name, spec, inner)


def test_first_of_two_blocks_ends_in_the_interior_body(model):
    """two_blocks: every iteration of the first block is an interior one, the last (a literal and the
    end-of-block symbol) at op = ISIZE - 260 exactly, and the 259 bytes of the second block have none.
    two_long: the second block goes back into the interior body.  The counts follow from the token
    lists (two_block_interior_iterations), asserted there before the stream is built."""
    cs, names, runs = model
    for name in ic.TWO:
        n1, n2 = ic.two_block_interior_iterations(name)
        assert n1 > 0 and (n2 == 0 if name == "two_blocks" else n2 > 0), (name, n1, n2)
        _, _, spec, inner = runs["asis"][1][names.index(name)]
        assert inner == n1 + n2 and spec > 0, (name, spec, inner, n1, n2)


def test_corrupted_copies_end_the_same_three_ways(model):
    cs, names, runs = model
    n = len(names)
    soft, hard = runs["asis"][0][n], runs["asis"][0][n + 1]
    assert soft[1:4] == (0, len(cs["far"][1]), 1)  # zlib's (different) bytes
    assert hard[3] == 0
    for way in ("no_interior", "generic"):
        assert runs[way][0][n][1:4] == soft[1:4] and runs[way][0][n + 1][1:4] == hard[1:4], way
