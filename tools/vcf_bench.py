#!/usr/bin/env python
"""Text VCF on the device, measured: hbam_vcf_decode_split over >= 1 GB of VCF text resident on
the GPU (HIP events on the context's stream, after warm-up), beside a plain device-to-device copy
of the same buffer (the streaming yardstick), and vcf-sort's sort (hbam_sort_keys) and line
gather (hbam_vcf_gather_lines) over the same lines.  Prints one JSON object per measurement.

    python tools/vcf_bench.py [--bytes N] [--iters K] [--warmup W]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))

N_CONTIGS = 25
HEADER = ("##fileformat=VCFv4.1\n"
          + "".join("##contig=<ID=chr%d,length=%d>\n" % (i + 1, 250000000 - i) for i in range(N_CONTIGS))
          + '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')


def block(n_lines, n_samples, seed):
    """n_lines data lines (about 40 + 12 * n_samples bytes each), random contigs and positions."""
    rng = random.Random(seed)
    out = []
    for i in range(n_lines):
        gts = "\t".join("%d/%d:%d:%d,%d" % (rng.randint(0, 1), rng.randint(0, 1), rng.randint(0, 99),
                                          rng.randint(0, 60), rng.randint(0, 60)) for _ in range(n_samples))
        out.append("chr%d\t%d\trs%d\t%s\t%s\t%d\tPASS\tDP=%d;AF=0.5\tGT:GQ:HQ\t%s\n" % (
            rng.randint(1, N_CONTIGS), rng.randint(1, 200000000), i, rng.choice("ACGT"), rng.choice("ACGT"),
            rng.randint(1, 99), rng.randint(1, 500), gts))
    return "".join(out).encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=12)
    a = ap.parse_args()
    import torch
    from hadoop_bam import _lib
    from hadoop_bam.vcf import read_vcf_header

    samples = ["S%03d" % i for i in range(a.samples)]
    head = (HEADER + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n").encode()
    blk = block(20000, a.samples, 1)
    reps = max(1, -(-(a.bytes - len(head)) // len(blk)))
    n = len(head) + reps * len(blk)
    if n > 1 << 31:
        raise SystemExit("one window is at most 2 GiB")
    dev = torch.device("cuda", 0)
    buf = torch.empty(n + 64, dtype=torch.uint8, device=dev)  # 64 readable bytes follow the text
    buf[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
    buf[len(head):n] = torch.frombuffer(bytearray(blk), dtype=torch.uint8).to(dev).repeat(reps)
    text = buf[:n]
    _, contigs, data_start = read_vcf_header(head + blk[:1])
    ctx = _lib.Context(0)
    table = ctx.vcf_contig_table(contigs)
    n_lines = 20000 * reps

    # ---- the plain copy of the same bytes
    dst = torch.empty_like(buf)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_ms = []
    for it in range(a.warmup + a.iters):
        e0.record()
        dst[:n].copy_(text)
        e1.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            copy_ms.append(e0.elapsed_time(e1))
    del dst
    copy = statistics.median(copy_ms)
    print(json.dumps({"what": "device_to_device_copy", "bytes": n, "ms_median": round(copy, 3),
                      "ms_min": round(min(copy_ms), 3), "GBps": round(n / copy / 1e6, 1)}), flush=True)

    # ---- hbam_vcf_decode_split
    rows = []
    d = None
    for it in range(a.warmup + a.iters):
        rc, d = ctx.vcf_decode_split_device(text, 0, n, data_start, table, keep_text=True)
        if rc or d.status or d.n != n_lines:
            raise SystemExit("decode failed: rc %d status %d n %d (%s)" % (rc, d.status, d.n, ctx.last_error()))
        if it >= a.warmup:
            rows.append(ctx.timing())
    med = {k: statistics.median(r[k] for r in rows) for k in ("scan_ms", "walk_ms", "decode_ms", "total_ms")}
    print(json.dumps({"what": "hbam_vcf_decode_split", "bytes": n, "lines": n_lines,
                      "structural_scan_ms": round(med["scan_ms"], 3),
                      "line_scan_and_scatter_ms": round(med["walk_ms"], 3),
                      "field_pass_ms": round(med["decode_ms"], 3), "total_ms": round(med["total_ms"], 3),
                      "total_ms_min": round(min(r["total_ms"] for r in rows), 3),
                      "text_GBps": round(n / med["total_ms"] / 1e6, 1),
                      "copy_over_decode": round(copy / med["total_ms"], 3)}), flush=True)

    # ---- vcf-sort over the same lines: the key sort and the line gather
    vp = C.c_void_p

    def alloc(nbytes):
        p = vp()
        rc = ctx.L.hbam_device_alloc(ctx.h, int(nbytes), C.byref(p))
        if rc:
            raise SystemExit("hbam_device_alloc(%d) failed: %s" % (nbytes, ctx.last_error()))
        return p
    perm, off = alloc(4 * n_lines), alloc(8 * (n_lines + 1))
    tot = C.c_uint64(0)
    rc = ctx.L.hbam_vcf_gather_lines(ctx.h, C.byref(d), None, n_lines, None, 0, off, C.byref(tot))
    if rc:
        raise SystemExit("size query failed: %s" % ctx.last_error())
    out = alloc(tot.value)
    sort_ms, gather_ms, passes = [], [], 0
    for it in range(a.warmup + a.iters):
        rc = ctx.L.hbam_sort_keys(ctx.h, d.key, n_lines, None, perm)
        t = ctx.timing()
        rc = rc or ctx.L.hbam_vcf_gather_lines(ctx.h, C.byref(d), perm, n_lines, out, tot.value, off, C.byref(tot))
        if rc:
            raise SystemExit("sort / gather failed: %s" % ctx.last_error())
        if it >= a.warmup:
            sort_ms.append(t["total_ms"])
            passes = int(t["n_blocks"])
            gather_ms.append(ctx.timing()["pools_ms"])
    for p in (perm, off, out):
        ctx.L.hbam_device_free(ctx.h, p)
    g = statistics.median(gather_ms)
    print(json.dumps({"what": "vcf_sort", "lines": n_lines, "out_bytes": int(tot.value),
                      "sort_ms": round(statistics.median(sort_ms), 3), "radix_passes": passes,
                      "gather_ms": round(g, 3), "gather_GBps": round(tot.value / g / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
