#!/usr/bin/env python
"""SAM text output on the device, measured: hbam_sam_render over the 2,520,000 records of
tools/sam_bench.py's workload (one block of genbam records repeated to about 1 GiB of SAM text),
resident on the GPU as the columns of a decode, by pass (the library's own HIP events, medians after
warm-up); in the same run a plain device-to-device copy of the bytes it writes (the streaming
yardstick) and hbam_sam_decode_split over the text it produced.  Prints one JSON object per
measurement.

    python tools/samtext_bench.py [--bytes N] [--iters K] [--warmup W]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("hadoop-bam_amd", "tests", "oracle", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))


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
    names = [n for n, _ in h.refs]
    head = sam_ref.sam_file(sam_ref.header_text(h.text, h.refs), [])
    blk = sam_ref.sam_file([], sam_ref.render(recs, names))
    reps = max(1, -(-(a.bytes - len(head)) // len(blk)))
    n_lines = len(recs) * reps
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    table = ctx.vcf_contig_table(names)
    _, data_start, header = read_sam_text_header(head + blk[:1])

    # the records, on the device: the decode of the workload's text (its columns stay the context's)
    n = len(head) + reps * len(blk)
    if n > 1 << 31:
        raise SystemExit("one window is at most 2 GiB")
    buf = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    buf[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
    buf[len(head):n] = torch.frombuffer(bytearray(blk), dtype=torch.uint8).to(dev).repeat(reps)
    buf[n:] = 0
    rc, d = ctx.sam_decode_split_device(buf[:n], 0, n, data_start, table, len(names))
    if rc or d.status or d.n_records != n_lines:
        raise SystemExit("decode failed: rc %d status %d n %d (%s)" % (rc, d.status, d.n_records, ctx.last_error()))
    del buf
    bam_bytes = int(d.ubuf_len)

    # ---- hbam_sam_render
    rows = []
    for it in range(a.warmup + a.iters):
        rc, t = ctx.sam_render_device(d.ubuf, d.rec_off, n_lines, names)
        if rc or t.status or t.n_records != n_lines:
            raise SystemExit("render failed: rc %d status %d n %d (%s)" % (rc, t.status, t.n_records,
                                                                           ctx.last_error()))
        if it >= a.warmup:
            rows.append(ctx.timing())
    text_len = int(t.text_len)
    if text_len != reps * len(blk) or t.n_deferred:
        raise SystemExit("render wrote %d bytes (%d deferred), the workload's text has %d" %
                         (text_len, t.n_deferred, reps * len(blk)))
    med = {k: statistics.median(r[k] for r in rows) for k in ("walk_ms", "huffman_ms", "resolve_ms", "total_ms")}

    # ---- the plain copy of the bytes it writes
    src = torch.empty(text_len, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_ms = []
    for it in range(a.warmup + a.iters):
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            copy_ms.append(e0.elapsed_time(e1))
    del src, dst
    copy = statistics.median(copy_ms)
    print(json.dumps({"what": "device_to_device_copy", "bytes": text_len, "ms_median": round(copy, 3),
                      "ms_min": round(min(copy_ms), 3), "GBps": round(text_len / copy / 1e6, 1)}), flush=True)
    print(json.dumps({"what": "hbam_sam_render", "records": n_lines, "bam_bytes": bam_bytes, "text_bytes": text_len,
                      "deferred": int(t.n_deferred), "sizes_and_scans_ms": round(med["walk_ms"], 3),
                      "head_and_tags_ms": round(med["huffman_ms"], 3), "seq_qual_ms": round(med["resolve_ms"], 3),
                      "total_ms": round(med["total_ms"], 3),
                      "total_ms_min": round(min(r["total_ms"] for r in rows), 3),
                      "text_GBps": round(text_len / med["total_ms"] / 1e6, 1),
                      "copy_over_render": round(copy / med["total_ms"], 3)}), flush=True)

    # ---- hbam_sam_decode_split over the text it produced (the window begins at data_start)
    nm = np.frombuffer(table[2], np.uint8) if table[2] else np.zeros(1, np.uint8)
    rows = []
    for it in range(a.warmup + a.iters):
        back = _lib.Columns()
        rc = ctx.L.hbam_sam_decode_split(ctx.h, C.c_void_p(t.text), 1, data_start, text_len, data_start + text_len, 0,
                                         data_start + text_len, data_start, C.cast(table[0], C.c_void_p), table[1],
                                         C.c_void_p(nm.ctypes.data), len(table[2]), len(names), C.byref(back))
        if rc or back.status or back.n_records != n_lines or back.ubuf_len != bam_bytes:
            raise SystemExit("decode of the rendered text failed: rc %d status %d n %d (%s)" %
                             (rc, back.status, back.n_records, ctx.last_error()))
        if it >= a.warmup:
            rows.append(ctx.timing())
    dt = statistics.median(r["total_ms"] for r in rows)
    print(json.dumps({"what": "hbam_sam_decode_split_of_the_rendered_text", "text_bytes": text_len, "lines": n_lines,
                      "total_ms": round(dt, 3), "total_ms_min": round(min(r["total_ms"] for r in rows), 3),
                      "text_GBps": round(text_len / dt / 1e6, 1),
                      "render_over_decode": round(med["total_ms"] / dt, 3)}), flush=True)


if __name__ == "__main__":
    main()
