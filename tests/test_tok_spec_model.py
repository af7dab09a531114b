"""The specialised symbol loop of the Huffman lane pass (inflate_tok.h tok_symbols) on the CPU model
(tools/cpu_model, one lane, MemorySanitizer): crafted dynamic-Huffman blocks whose code lengths sit
on and around what the specialised body relies on (tests/deflate_craft.py; every stream vouched
for by zlib).  Every block must inflate to zlib's bytes, and the model's per-block counters must
show the specialised body entered exactly for the DEFLATE blocks whose tables fit (both codes
complete, no length 1 or 2, no distance code above 11 bits) and the generic body for the rest; with
HBAM_TOK_GENERIC=1 only the generic body runs and every outcome is the same."""
import os
import re
import struct
import subprocess
import sys

import pytest

import deflate_craft as craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("HBAM_MODEL_CXX", "/opt/rocm/lib/llvm/bin/clang++")

# what each case must select, stated here and not derived from the code under test
EXPECT = {"ll_min1": [False], "ll_min2": [False], "ll_min3": [True], "ll_min4": [True], "ll_max14": [True],
          "ll_max15": [True], "d_max9": [True], "d_max10": [True], "d_max11": [True], "d_max12": [False],
          "d_max15": [False], "d_min1": [False], "d_min2": [False], "d_single": [False], "d_empty": [False],
          "fit_then_not": [True, False], "not_then_fit": [False, True], "dyn_then_fixed": [True, True],
          "dyn_then_stored": [True]}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ with MemorySanitizer")
    d = tmp_path_factory.mktemp("tok_spec_model")
    sys.path.insert(0, os.path.join(ROOT, "tools/cpu_model"))
    import build as model_build
    exe = model_build.build(str(d), "cur")
    cs = craft.cases()
    names = list(cs)
    recs = [(cs[k][0], cs[k][1]) for k in names]
    # two corrupted copies of a fitting block: zlib still inflates one (to other bytes), rejects the other
    soft, soft_u = craft.flipped(cs["ll_min3"][0], want_error=False)
    hard, _ = craft.flipped(cs["ll_min3"][0], want_error=True)
    recs += [(soft, soft_u), (hard, cs["ll_min3"][1])]
    path = str(d / "blocks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x4d544248, len(recs)))
        for raw, u in recs:
            f.write(struct.pack("<II", len(raw), len(u)) + raw + u)
    runs = {}
    for gen in ("0", "1"):
        r = subprocess.run([exe, path, "-v"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                           env=dict(os.environ, HBAM_TOK_GENERIC=gen))
        assert "MemorySanitizer" not in r.stderr, r.stderr[-4000:]
        rows = [tuple(int(x) for x in m.groups()) for m in re.finditer(
            r"^block (\d+) rc (-?\d+) produced (\d+) ok (\d) generic (\d+) specialised (\d+)$", r.stdout, re.M)]
        assert len(rows) == len(recs), r.stdout
        runs[gen] = rows
    return cs, names, runs


def test_cases_are_what_they_say():
    """The crafted code lengths have the stated shape (the test's own inputs, checked by hand rules)."""
    cs = craft.cases()
    assert set(cs) == set(EXPECT)
    for k, (raw, u, bodies) in cs.items():
        assert bodies == EXPECT[k], k
        assert 1000 <= len(u) <= 4096 and len(raw) >= 200, (k, len(u), len(raw))


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_model_inflates_and_enters_the_expected_body(model, name):
    cs, names, runs = model
    i = names.index(name)
    _, rc, produced, ok, gen, spec = runs["0"][i]
    assert (rc, produced, ok) == (0, len(cs[name][1]), 1)  # ok: bytes equal zlib's
    assert (gen, spec) == (EXPECT[name].count(False), EXPECT[name].count(True)), name
    _, rc, produced, ok, gen, spec = runs["1"][i]
    assert (rc, produced, ok) == (0, len(cs[name][1]), 1)
    assert (gen, spec) == (len(EXPECT[name]), 0), name


def test_corrupted_fitting_block_ends_as_in_the_generic_body(model):
    """One flipped bit in the symbol region of a block that takes the specialised body: the flip zlib
    still inflates gives zlib's (different) bytes, the flip zlib rejects fails, and both end with the
    same status and output count as under the generic body."""
    cs, names, runs = model
    n = len(names)
    soft, hard = runs["0"][n], runs["0"][n + 1]
    assert soft[1:4] == (0, len(cs["ll_min3"][1]), 1) and soft[5] == 1
    assert hard[3] == 0 and hard[5] == 1
    assert runs["1"][n][1:4] == soft[1:4] and runs["1"][n + 1][1:4] == hard[1:4]
    assert runs["1"][n][5] == 0 and runs["1"][n + 1][5] == 0
