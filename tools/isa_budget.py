"""Instruction budget of the Huffman lane pass's symbol loops from a gfx950 assembly listing built
with line tables:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-sched-strategy=max-ilp -Iinclude \
          --cuda-device-only -S -gline-tables-only -o tok.s hadoop-bam_amd/csrc/hbam_inflate_tokens.hip
    python tools/isa_budget.py tok.s hadoop-bam_amd/csrc/inflate_tok.h

Every loop of k_inflate_tokens that holds packed lookups (v_pk_sub_u16) is a symbol loop.  Its basic
blocks are listed with their instruction counts by unit (VALU / SALU / LDS / VMEM / other) and by
the source function the line table attributes each instruction to (the innermost inlined frame):
the lookups (huffp_lookup, ein_rev15), the refills (ein_refill*, ein_sel), the bases
(length_base*, dist_base*), the packet / mark (TSink, TPend), the epoch (ein_epoch*, ein_short),
the token logic of the iteration itself (tok_fast_spec, ein_drop, ein_peek), the careful symbol
(tok_careful) and the loop's exit bookkeeping (tok_symbols / inflate_tokens_block).  The fast path
is the straight run of blocks from the loop head to the back edge that holds no tok_careful line;
blocks with tok_careful lines are the careful symbol, and the short side blocks hold the chunk /
window stores.  Counts by category, nothing else.
"""
import re
import sys

CATS = [("lookup", r"huffp_lookup|ein_rev15|huffp_fold"), ("refill", r"ein_refill|ein_sel\b"),
        ("bases", r"length_base|dist_base"), ("packet/mark", r"put|mark|mark_if|switch_if|flush|win_store|chunk|literal|match|clear"),
        ("epoch", r"ein_epoch|ein_short|ein_load"), ("token logic", r"tok_fast_spec|ein_drop|ein_peek|ein_avail"),
        ("careful", r"tok_careful"), ("loop", r"tok_symbols|inflate_tokens_block|k_inflate_tokens")]


def functions(src):
    """[(first line, last line, name)] of the functions of a source file (brace matching from the signature)."""
    lines = open(src).read().splitlines()
    out, i = [], 0
    sig = re.compile(r"^\s*(?:template\s*<[^>]*>\s*)?(?:__device__|__global__|static|inline).*?\b(\w+)\s*\($|"
                     r"^\s*(?:__device__|__global__).*?\b(\w+)\s*\(")
    while i < len(lines):
        m = sig.match(lines[i])
        if m and not lines[i].rstrip().endswith(";"):
            name = m.group(1) or m.group(2)
            depth, j, seen = 0, i, False
            while j < len(lines):
                depth += lines[j].count("{") - lines[j].count("}")
                seen |= "{" in lines[j]
                if seen and depth <= 0:
                    break
                j += 1
            out.append((i + 1, j + 1, name))
            i = j + 1
        else:
            i += 1
    return out


def unit(op):
    if op.startswith(("v_",)):
        return "VALU"
    if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_load", "s_buffer_load")):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "scratch_", "flat_", "buffer_")):
        return "VMEM"
    return "other"


def main():
    listing, src = sys.argv[1], sys.argv[2]
    funcs = functions(src)
    srcname = src.split("/")[-1]
    text = open(listing).read()
    i = text.index("_ZN4hbam16k_inflate_tokens")
    i = text.index("\n", text.index(":", i))
    body = text[i:text.index(".Lfunc_end", i)].splitlines()
    files = {m.group(1): m.group(2) for m in re.finditer(r'\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', text)}
    # instructions with their block label and attributed function
    ins, label, cur = [], "entry", ("?", 0)
    labels = {}
    for l in body:
        t = l.strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label = m.group(1)
            labels[label] = len(ins)
            continue
        m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            cur = (files.get(m.group(1), "?"), int(m.group(2)))
            continue
        if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        fn = "?"
        if cur[0].endswith(srcname):
            for a, b, name in funcs:
                if a <= cur[1] <= b:
                    fn = name
        elif cur[0].endswith("hbam_inflate_tokens.hip"):
            fn = "k_inflate_tokens"
        cat = next((c for c, pat in CATS if re.fullmatch(pat, fn) or re.match("(?:%s)" % pat, fn)), "other")
        ins.append((label, op, cat, t))
    # loops: backward branches; keep the innermost ranges that hold packed lookups
    loops = []
    for k, (_, op, _, t) in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", t)
        if m and m.group(1) in labels and labels[m.group(1)] <= k:
            a = labels[m.group(1)]
            if any(x[1] == "v_pk_sub_u16" for x in ins[a:k + 1]):
                loops.append((a, k))
    loops = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    for a, k in loops:
        seg = ins[a:k + 1]
        npk = sum(1 for x in seg if x[1] == "v_pk_sub_u16")
        blocks = []
        for x in seg:
            if not blocks or blocks[-1][0] != x[0]:
                blocks.append((x[0], []))
            blocks[-1][1].append(x)
        print("symbol loop at %s: %d instructions, %d packed compares (v_pk_sub_u16)" % (ins[a][0], len(seg), npk))
        fast = []
        for lab, b in blocks:
            careful = any(x[2] == "careful" for x in b)
            stores = sum(1 for x in b if x[1].startswith(("global_store", "scratch_store")))
            kind = "careful symbol" if careful else "side block (stores)" if stores and len(b) < 40 else "fast path"
            print("  block %-10s %4d instructions  %s" % (lab, len(b), kind))
            if kind == "fast path":
                fast += b
        print("  fast path: %d instructions" % len(fast))
        print("    %-12s %5s %5s %5s %5s %5s" % ("", "VALU", "SALU", "LDS", "VMEM", "other"))
        tot = {}
        for c in [c for c, _ in CATS] + ["other"]:
            row = [sum(1 for x in fast if x[2] == c and unit(x[1]) == u) for u in ("VALU", "SALU", "LDS", "VMEM", "other")]
            if sum(row):
                print("    %-12s %5d %5d %5d %5d %5d" % ((c,) + tuple(row)))
            for u, v in zip(("VALU", "SALU", "LDS", "VMEM", "other"), row):
                tot[u] = tot.get(u, 0) + v
        print("    %-12s %5d %5d %5d %5d %5d" % ("total", tot["VALU"], tot["SALU"], tot["LDS"], tot["VMEM"], tot["other"]))
        print()


if __name__ == "__main__":
    main()
