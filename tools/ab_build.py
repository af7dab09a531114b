"""Build an A/B variant of libhbam.so with the product recipe (__graft_entry__.build: the Huffman
lane pass in its own max-ILP translation unit, everything else default-scheduled) plus extra
-D flags, into hadoop-bam_amd/NAME.  Never loaded by the tests, smoke() or bench.py unless
HBAM_LIB names it.  The lane pass's own A/B knobs have been constants since a2116c6: a variant of
it is built from a second source tree (a checkout of the other commit, with that tree's copy of
this script); -D flags still reach the switches that are left, such as the profiling build:
    python tools/ab_build.py libhbam_prof.so -DHBAM_PROF
A -D name that no file under csrc/ mentions is refused: it would build a copy of the product
library, and the A/B would compare identical code.  Knobs read from the environment when a context
is created (HBAM_CHAIN_SEG, HBAM_CHAIN_DENSE, ...) need no build of their own."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def unknown_defines(defs, csrc=None):
    """The -D names among `defs` that occur as a word in no file under csrc/."""
    csrc = csrc or g.CSRC
    text = "\n".join(open(os.path.join(csrc, f), errors="replace").read() for f in sorted(os.listdir(csrc)))
    names = [d[2:].split("=", 1)[0] for d in defs if d.startswith("-D")]
    return [n for n in names if not re.search(r"\b%s\b" % re.escape(n), text)]


def main():
    name, defs = sys.argv[1], sys.argv[2:]
    stale = unknown_defines(defs)
    if stale:
        sys.exit("ab_build: no file under csrc/ mentions %s: the variant would be the product library"
                 % ", ".join(stale))
    # HBAM_AB_CAPI_FLAGS: extra flags for the hbam_capi.hip unit only (e.g. its own scheduler)
    capi_extra = os.environ.get("HBAM_AB_CAPI_FLAGS", "").split()
    obj = os.path.join(ROOT, "build", "ab", name)
    os.makedirs(obj, exist_ok=True)
    cflags = [f for f in g.HIP_FLAGS if f != "-shared"] + ["-c"] + defs
    o_tok, o_capi = os.path.join(obj, "tok.o"), os.path.join(obj, "capi.o")
    procs = [subprocess.Popen([g.HIPCC] + cflags + ["-mllvm", "-amdgpu-sched-strategy=max-ilp", "-o", o_tok,
                               os.path.join(g.CSRC, "hbam_inflate_tokens.hip")]),
             subprocess.Popen([g.HIPCC] + cflags + capi_extra + ["-DHBAM_SPLIT_TOK", "-o", o_capi,
                               os.path.join(g.CSRC, "hbam_capi.hip")])]
    if any(p.wait() for p in procs):
        sys.exit("ab_build: compile failed")
    subprocess.check_call([g.HIPCC, "-shared", "-fPIC", "--offload-arch=" + g.ARCH, "-o",
                           os.path.join(g.PKG, name), o_capi, o_tok])
    print("built hadoop-bam_amd/%s %s" % (name, " ".join(defs)))


if __name__ == "__main__":
    main()
