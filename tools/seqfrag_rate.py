#!/usr/bin/env python3
"""Decode rate of the FASTQ device path next to the text-VCF path (the yardstick: existing code).

Generates about --gb GB of FASTQ in memory (a block of records with Illumina names, tiled), uploads
it, decodes it whole-file and device-resident with hbam_fastq_decode_split and prints text GB/s and
the stage times of ctx.timing(); then does the same for hbam_vcf_decode_split over a generated VCF
of the same size.  Not a test and not part of bench.py.

    python tools/seqfrag_rate.py [--gb 1.0] [--reps 3]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))


def fastq_block(records=4096, read_len=100, seed=1):
    r = random.Random(seed)
    out = bytearray()
    for k in range(records):
        seq = bytes(r.choice(b"ACGT") for _ in range(read_len))
        qual = bytes(r.randrange(35, 75) for _ in range(read_len))
        out += b"@M01:%d:FC0001:%d:%d:%d:%d 1:N:0:ACGTAC\n" % (r.randrange(1000), r.randrange(1, 9), r.randrange(1, 3000),
                                                          r.randrange(30000), r.randrange(30000))
        out += seq + b"\n+\n" + qual + b"\n"
    return bytes(out)


def vcf_parts(lines=4096, seed=2):
    r = random.Random(seed)
    header = b"##fileformat=VCFv4.1\n" + b"".join(b"##contig=<ID=chr%d,length=250000000>\n" % i for i in range(1, 23))
    header += b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\tS3\n"
    out = bytearray()
    for k in range(lines):
        out += b"chr%d\t%d\trs%d\t%s\t%s\t%d\tPASS\tDP=%d;AF=0.5\tGT:DP\t0/1:%d\t1/1:%d\t0/0:%d\n" % (
            r.randrange(1, 23), r.randrange(1, 240000000), k, r.choice((b"A", b"ACG", b"T")), r.choice((b"C", b"G,T")),
            r.randrange(100), r.randrange(100), r.randrange(60), r.randrange(60), r.randrange(60))
    return header, bytes(out)


def tiled(head, block, nbytes, torch):
    reps = max(1, (nbytes - len(head)) // len(block))
    host = np.concatenate([np.frombuffer(head, np.uint8), np.tile(np.frombuffer(block, np.uint8), reps)])
    dev = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")  # the 64 readable bytes behind the text
    dev[:host.size] = torch.from_numpy(host).cuda()
    return dev[:host.size], host.size


def report(name, nbytes, times):
    best = min(times, key=lambda t: t["total_ms"])
    print("%s: %.3f GB, %d records, %.2f GB/s (best of %d; total %.2f ms: scan %.2f, walk %.2f, decode %.2f, "
          "pools %.2f)" % (name, nbytes / 1e9, best["n_records"], nbytes / 1e6 / best["total_ms"], len(times),
                          best["total_ms"], best["scan_ms"], best["walk_ms"], best["decode_ms"], best["pools_ms"]),
          flush=True)
    return nbytes / 1e6 / best["total_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from hadoop_bam import _lib
    from hadoop_bam.vcf import read_vcf_header
    ctx = _lib.Context(0)
    nbytes = int(a.gb * 1e9)

    text, n = tiled(b"", fastq_block(), nbytes, torch)
    times = []
    for _ in range(a.reps + 1):  # the first run allocates the context's buffers
        rc, d = ctx.frag_decode_split_device("fastq", text, 0, n, file_len=n)
        assert rc == 0 and d.status == 0, (rc, d.status, ctx.last_error())
        times.append(ctx.timing())
    fq = report("fastq", n, times[1:])
    del text
    torch.cuda.empty_cache()

    head, block = vcf_parts()
    text, n = tiled(head, block, nbytes, torch)
    _, contigs, data_start = read_vcf_header(head + block)
    table = ctx.vcf_contig_table(contigs)
    times = []
    for _ in range(a.reps + 1):
        rc, d = ctx.vcf_decode_split_device(text, 0, n, data_start, table, file_len=n)
        assert rc == 0 and d.status == 0, (rc, d.status, ctx.last_error())
        times.append(ctx.timing())
    vcf = report("vcf", n, times[1:])
    print("fastq / vcf = %.2f" % (fq / vcf), flush=True)


if __name__ == "__main__":
    main()
