#!/usr/bin/env python
"""SAM text on the device, measured: hbam_sam_decode_split over about 1 GiB of SAM text resident on
the GPU (the library's own HIP events, after warm-up), beside a plain device-to-device copy of the
same buffer (the streaming yardstick), hbam_vcf_decode_split's recorded rate and hbam_decode_split
over the same records as BAM.  The text is one block of genbam records, rendered by the test
tree's renderer (tests/sam_ref.py) and repeated.  Prints one JSON object per measurement.

    python tools/sam_bench.py [--bytes N] [--iters K] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("hadoop-bam_amd", "tests", "oracle", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

VCF_DECODE_GBPS = 824.0  # hbam_vcf_decode_split at 1 GiB (profiles/vcf_text)
STAGES = ("scan_ms", "walk_ms", "inflate_ms", "huffman_ms", "resolve_ms", "decode_ms", "pools_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--block-records", type=int, default=20000)
    a = ap.parse_args()
    import numpy as np
    import torch
    import genbam
    import sam_cases
    import sam_ref
    from hadoop_bam import _lib, read_sam_text_header

    bam = np.asarray(genbam.generate(records=a.block_records, seed=1, odd_every=97))
    h, recs = sam_cases.bam_header_and_records(bam)
    head = sam_ref.sam_file(sam_ref.header_text(h.text, h.refs), [])
    blk = sam_ref.sam_file([], sam_ref.render(recs, [n for n, _ in h.refs]))
    reps = max(1, -(-(a.bytes - len(head)) // len(blk)))
    n = len(head) + reps * len(blk)
    if n > 1 << 31:
        raise SystemExit("one window is at most 2 GiB")
    n_lines = len(recs) * reps
    dev = torch.device("cuda", 0)
    buf = torch.empty(n + 64, dtype=torch.uint8, device=dev)  # 64 readable bytes follow the text
    buf[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
    buf[len(head):n] = torch.frombuffer(bytearray(blk), dtype=torch.uint8).to(dev).repeat(reps)
    buf[n:] = 0
    text = buf[:n]
    _, data_start, header = read_sam_text_header(head + blk[:1])
    ctx = _lib.Context(0)
    table = ctx.vcf_contig_table([nm for nm, _ in header.refs])

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

    # ---- hbam_sam_decode_split
    rows = []
    for it in range(a.warmup + a.iters):
        rc, d = ctx.sam_decode_split_device(text, 0, n, data_start, table, len(header.refs))
        if rc or d.status or d.n_records != n_lines:
            raise SystemExit("decode failed: rc %d status %d n %d (%s)" % (rc, d.status, d.n_records,
                                                                           ctx.last_error()))
        if it >= a.warmup:
            rows.append(ctx.timing())
    med = {k: statistics.median(r[k] for r in rows) for k in STAGES}
    bam_bytes = int(rows[0]["ubuf_bytes"])
    gbps = n / med["total_ms"] / 1e6
    enc = n / med["inflate_ms"] / 1e6
    print(json.dumps({"what": "hbam_sam_decode_split", "text_bytes": n, "lines": n_lines, "bam_bytes": bam_bytes,
                      "structural_scan_ms": round(med["scan_ms"], 3),
                      "line_scan_sizes_scan_ms": round(med["walk_ms"], 3),
                      "encode_ms": round(med["inflate_ms"], 3), "encode_lines_ms": round(med["huffman_ms"], 3),
                      "encode_seq_qual_ms": round(med["resolve_ms"], 3),
                      "fixed_fields_and_keys_ms": round(med["decode_ms"], 3),
                      "pools_ms": round(med["pools_ms"], 3), "total_ms": round(med["total_ms"], 3),
                      "total_ms_min": round(min(r["total_ms"] for r in rows), 3), "text_GBps": round(gbps, 1),
                      "copy_over_decode": round(copy / med["total_ms"], 3),
                      "encode_text_GBps": round(enc, 1), "copy_over_encode": round(copy / med["inflate_ms"], 3),
                      "over_vcf_decode_824GBps": round(gbps / VCF_DECODE_GBPS, 3)}), flush=True)

    # ---- hbam_decode_split over the same records as BAM, for scale
    hdr = h.to_bam_bytes()
    rec_blk = b"".join(recs)
    u = torch.empty(len(hdr) + reps * len(rec_blk), dtype=torch.uint8, device=dev)
    u[:len(hdr)] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    u[len(hdr):] = torch.frombuffer(bytearray(rec_blk), dtype=torch.uint8).to(dev).repeat(reps)
    comp = torch.empty(int(ctx.L.hbam_bgzf_bound(u.numel(), 0)) + 64, dtype=torch.uint8, device=dev)
    m = ctx.bgzf_compress(u, 0, out=comp)
    del u, buf, text
    hb = ctx.parse_header(comp[:min(m, 1 << 22)].cpu().numpy())
    rows = []
    for it in range(a.warmup + a.iters):
        rc, d = ctx.decode_split_device(comp[:m], hb["first_voffset"], (m << 16) | 0xffff, hb["n_ref"])
        if rc or d.status or d.n_records != n_lines:
            raise SystemExit("BAM decode failed: rc %d status %d n %d (%s)" % (rc, d.status, d.n_records,
                                                                               ctx.last_error()))
        if it >= a.warmup:
            rows.append(ctx.timing())
    t = statistics.median(r["total_ms"] for r in rows)
    print(json.dumps({"what": "hbam_decode_split_same_records_as_bam", "compressed_bytes": m,
                      "bam_bytes": int(rows[0]["ubuf_bytes"]), "records": n_lines, "total_ms": round(t, 3),
                      "total_ms_min": round(min(r["total_ms"] for r in rows), 3),
                      "bam_GBps": round(rows[0]["ubuf_bytes"] / t / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
