"""Instruction budget of the Huffman lane pass's symbol loops from a gfx950 assembly listing built
with line tables:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-sched-strategy=max-ilp -Iinclude \
          --cuda-device-only -S -gline-tables-only -o tok.s hadoop-bam_amd/csrc/hbam_inflate_tokens.hip
    python tools/isa_budget.py tok.s hadoop-bam_amd/csrc/inflate_tok.h

Every loop of k_inflate_tokens that holds packed lookups (v_pk_sub_u16) is a symbol loop.  Its basic
blocks are listed with their instruction counts by unit (VALU / SALU / LDS / VMEM / other) and by
the source function the line table attributes each instruction to (the innermost inlined frame):
the lookups (huffp_lookup, ein_rev15), the refill (ein_window, ein_align, ein_take: the 64-bit
window at the bit cursor), the bases (length_base*, dist_base*), the packet / mark (TSink, TPend), the epoch (ein_epoch*, ein_short),
the token logic of the iteration itself (tok_fast_spec, ein_drop, ein_peek), the careful symbol
(tok_careful) and the loop's exit bookkeeping (tok_symbols / inflate_tokens_block).  The fast path
is the straight run of blocks from the loop head to the back edge that holds no tok_careful line;
blocks with tok_careful lines are the careful symbol, and the short side blocks hold the chunk /
window stores.  Below each table: the straight-line iteration (straight_line), the labelled blocks
a wave runs when no lane takes the careful symbol and no store side block is entered.  Counts by
category, nothing else.
"""
import re
import sys

CATS = [("lookup", r"huffp_lookup|ein_rev15|huffp_fold"), ("refill", r"ein_window|ein_align|ein_take"),
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
    falls = set()  # where an unlabelled block (; %bb.N:) begins: the fall-through of a branch
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
        if re.match(r"^; %bb\.\d+:", t):
            falls.add(len(ins))
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
        straight_line(ins, labels, falls, a, k)
        print()


def straight_line(ins, labels, falls, a, k):
    """The iteration a wave runs when no lane takes the careful symbol and no store side block is
    entered, in whole labelled blocks from the loop head to the back edge.  A block is followed by
    the next labelled block, with two exceptions.  A block that holds a store and that a conditional
    branch of the block before it skips exactly (the branch targets the label after it) is a side
    block: the walk takes the branch.  A block with a conditional branch over tok_careful lines is
    the careful-symbol gate: the walk takes that branch and counts nothing of the gate's block.  The
    "fast path" above also counts what sits behind the gate without a tok_careful line (the pending
    packet's flush, its refill, TSink::match, exec-restore stubs); this walk does not.  The epoch
    blocks, which run every TOK_K-th iteration, are on the walk, and so is store code that shares a
    label with the straight path: a guarded store tail, the unlabelled fall-through of an
    s_cbranch_execz that skips fewer than 40 instructions with a store among them.  A labelled
    block the table calls a side block can therefore be on the walk (straight code that ends in
    such a tail).  The tails on the walk are counted on their own line, so that two trees are
    compared without them."""
    starts = sorted(v for v in set(labels.values()) if a <= v <= k)
    if not starts or starts[0] != a:
        starts = [a] + starts
    bounds = {s0: (starts[i + 1] if i + 1 < len(starts) else k + 1) for i, s0 in enumerate(starts)}

    def branches(s0):
        for i in range(s0, bounds[s0]):
            m = re.match(r"s_cbranch\w*\s+(\.LBB\w+)", ins[i][3])
            if m and m.group(1) in labels:
                yield i, labels[m.group(1)]

    def skipped(src, n):  # n: a store side block that src branches around
        stores = any(y[1].startswith(("global_store", "scratch_store")) for y in ins[n:bounds[n]])
        return stores and any(t == bounds[n] for _, t in branches(src))

    def gate(n):  # the target of n's branch over the careful symbol
        for i, t in branches(n):
            if i < t <= k and any(y[2] == "careful" for y in ins[i + 1:t]):
                return t
        return None

    path, visited, cur, walked = [], [], a, set()
    while True:
        path += ins[cur:bounds[cur]]
        walked.update(range(cur, bounds[cur]))
        visited.append(ins[cur][0])
        if bounds[cur] > k:
            break
        nxt = bounds[cur]
        for _ in range(len(starts)):
            if skipped(cur, nxt):
                nxt = bounds[nxt]
            elif gate(nxt) is not None:
                nxt = gate(nxt)
            else:
                break
        if any(y[2] == "careful" for y in ins[nxt:bounds[nxt]]):
            print("  straight-line iteration: the walk ran into the careful symbol at %s" % ins[nxt][0])
            return
        cur = nxt
    u = {n: sum(1 for y in path if unit(y[1]) == n) for n in ("VALU", "SALU", "LDS", "VMEM", "other")}
    print("  straight-line iteration (no careful symbol, no store side block): %d instructions: %d VALU, %d SALU, "
          "%d LDS, %d VMEM, %d other" % (len(path), u["VALU"], u["SALU"], u["LDS"], u["VMEM"], u["other"]))
    print("    blocks: %s" % " ".join(visited))
    tails = set()
    for i in sorted(walked):
        m = re.match(r"s_cbranch_execz\s+(\.LBB\w+)", ins[i][3])
        t = labels.get(m.group(1), -1) if m else -1
        if i + 1 in falls and i + 1 < t <= k + 1 and t - (i + 1) < 40 and any(
                y[1].startswith(("global_store", "scratch_store")) for y in ins[i + 1:t]):
            tails.update(range(i + 1, t))
    tails &= walked
    print("    of which in guarded store tails (skipped when no lane stores): %d; without them: %d instructions"
          % (len(tails), len(path) - len(tails)))
    print("    %-12s %5s %5s %5s %5s %5s" % ("", "VALU", "SALU", "LDS", "VMEM", "other"))
    for c in [c for c, _ in CATS] + ["other"]:
        row = [sum(1 for y in path if y[2] == c and unit(y[1]) == n) for n in ("VALU", "SALU", "LDS", "VMEM", "other")]
        if sum(row):
            print("    %-12s %5d %5d %5d %5d %5d" % ((c,) + tuple(row)))


if __name__ == "__main__":
    main()
