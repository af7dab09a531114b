"""tools/ab_build.py refuses -D names that no file under csrc/ mentions (a variant built with one
is a copy of the product library)."""
import os
import subprocess
import sys

from conftest import ROOT


def test_unknown_defines():
    import ab_build
    assert ab_build.unknown_defines(["-DHBAM_PROF", "-DHBAM_SPLIT_TOK=1", "-O2"]) == []
    assert ab_build.unknown_defines(["-DHBAM_PROF", "-DHBAM_TOK_K=8", "-DHBAM_NO_SUCH"]) == ["HBAM_TOK_K", "HBAM_NO_SUCH"]


def test_stale_define_stops_the_build_before_it_compiles():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_build.py"), "libhbam_never.so", "-DHBAM_TOK_K=8"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "HBAM_TOK_K" in r.stderr
    assert not os.path.exists(os.path.join(ROOT, "hadoop-bam_amd", "libhbam_never.so"))
