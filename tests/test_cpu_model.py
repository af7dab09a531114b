"""The Huffman pass's per-lane decode (inflate_tok.h) compiled for the host under MemorySanitizer
(tools/cpu_model): round-3 verdict item 6.  The r02 profiling build (commit b49031e, predicated
fast path + cycle stamps) failed only in waves that reused a CU slot; a read of state the decode
never wrote (stale LDS symbol slots, code-length scratch, registers) is what launch position can
change.  Every block of the eight generated files of tools/check_inflate_crc.py (1 MB each here) is
decoded by the unmodified per-lane function with every such buffer left uninitialised, resolved
and compared with zlib: MSan reports any uninitialised value that reaches a branch, an address or
the output.  Result: none, in the current source and in the r02 source (the two
headers of that commit, kept under tests/golden/r02_b49031e/)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("HBAM_MODEL_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    d = tmp_path_factory.mktemp("cpu_model")
    out = str(d / "blocks.bin")
    subprocess.run(["python3", os.path.join(ROOT, "tools/cpu_model/make_blocks.py"), out, "1"], check=True,
                   stdout=subprocess.DEVNULL)
    return d, out


@pytest.mark.parametrize("variant", ["cur", "r02prof"])
def test_huffman_lane_has_no_uninitialised_reads(blocks, variant):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ with MemorySanitizer")
    d, path = blocks
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools/cpu_model"))
    import build as model_build
    exe = model_build.build(str(d), variant)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert "MemorySanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert " bad 0 " in r.stdout, r.stdout


def test_sanitizer_build_reports_a_stale_slot_read(blocks):
    """Negative control: the same build with one read of a never-written symbol slot into a
    branch (HBAM_MODEL_SELFTEST) is reported, so a clean run above means something."""
    if not os.path.exists(CXX):
        pytest.skip("no clang++ with MemorySanitizer")
    d, path = blocks
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools/cpu_model"))
    import build as model_build
    exe = model_build.build(str(d), "cur", extra=["-DHBAM_MODEL_SELFTEST"], tag="_selftest")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "use-of-uninitialized-value" in r.stderr, r.stderr[-2000:]
