"""Throughput of hbam_frag_render on a device-resident decode, recorded next to its yardsticks.

A generated FASTQ of about --mib MiB is uploaded and decoded once (hbam_fastq_decode_split); the
device columns are rendered as FASTQ (keys, Sanger) and as QSEQ (Illumina) --reps times after
--warmup calls, and the hbam_timing stages of each call are kept.  In the same process a
device-to-device copy of text_len bytes is timed with device events (the only yardstick a render can
be held to: it reads and writes the same bytes), and hbam_sam_render, the sibling kernel, renders a
generated BAM of comparable text size.  Prints one JSON document: per stage the median, minimum and
maximum in ms, and GB/s of text for the bulk pass and the copy.

    python tools/frag_render_bench.py --mib 256 --out profiles/frag_text/render.json
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("hadoop-bam_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))


def generated_fastq(mib, seed=31):
    """About mib MiB: a block of 4,096 records (Illumina ids, 100 to 150 bases, qualities in
    [33, 95] so that both encodings accept them) repeated."""
    r = random.Random(seed)
    block = bytearray()
    for _ in range(4096):
        n = r.randrange(100, 151)
        name = b"M%d:%d:FC%d:%d:%d:%d:%d %d:%s:%d:%s" % (
            r.randrange(100), r.randrange(1000), r.randrange(10), r.randrange(1, 9), r.randrange(1, 3000),
            r.randrange(1, 30000), r.randrange(1, 30000), r.randrange(1, 3), r.choice((b"Y", b"N")),
            r.randrange(0, 40), r.choice((b"ACGTAC", b"NNN")))
        block += b"@" + name + b"\n" + bytes(r.choice(b"ACGTN") for _ in range(n)) + b"\n+\n" + \
            bytes(r.randrange(33, 96) for _ in range(n)) + b"\n"
    return bytes(block) * max(1, (mib << 20) // len(block))


def summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def stages(timings, text_len):
    out = {k: summary([t[k] for t in timings]) for k in ("walk_ms", "huffman_ms", "resolve_ms", "total_ms")}
    out["names"] = {"walk_ms": "sizes pass + scans", "huffman_ms": "head pass", "resolve_ms": "bulk pass"}
    out["text_bytes"] = text_len
    out["bulk_gb_per_s"] = text_len / out["resolve_ms"]["median"] / 1e6
    out["total_gb_per_s"] = text_len / out["total_ms"]["median"] / 1e6
    return out


def copy_ms(nbytes, warmup, reps):
    import torch
    a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    times = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1))
    out = summary(times)
    out["bytes"] = nbytes
    out["gb_per_s_of_bytes_copied"] = nbytes / out["median"] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sam-bytes-per-record", type=int, default=330,
                    help="text bytes one generated BAM record renders to, roughly: sizes the sibling's input")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime opens the device before libhbam's)
    from hadoop_bam import _lib
    ctx = _lib.Context(0)
    res = {"warmup": a.warmup, "reps": a.reps}

    data = generated_fastq(a.mib)
    window = ctx.upload(data)
    rc, d = ctx.frag_decode_split_device("fastq", window, 0, len(data))
    assert rc == 0 and int(d.status) == 0, (rc, ctx.last_error())
    res["input"] = {"fastq_bytes": len(data), "records": int(d.n), "decode_ms": ctx.timing()["total_ms"]}
    for name, fmt, enc, flags in (("fastq", _lib.HBAM_FRAG_FASTQ, _lib.HBAM_QUAL_SANGER, _lib.HBAM_FRAG_USE_KEY),
                                  ("qseq", _lib.HBAM_FRAG_QSEQ, _lib.HBAM_QUAL_ILLUMINA, 0)):
        timings = []
        for k in range(a.warmup + a.reps):
            rc, t = ctx.frag_render_device(d, window, None, fmt, enc, flags)
            assert rc == 0 and int(t.status) == 0 and int(t.n_records) == int(d.n), (rc, ctx.last_error())
            if k >= a.warmup:
                timings.append(ctx.timing())
        text_len = int(t.text_len)
        if name == "fastq":
            assert text_len == len(data)
        res["render_" + name] = stages(timings, text_len)
        res["copy_" + name] = copy_ms(text_len, a.warmup, a.reps)
        res["render_" + name]["bulk_over_copy"] = (res["render_" + name]["resolve_ms"]["median"]
                                                   / res["copy_" + name]["median"])
        res["render_" + name]["total_over_copy"] = (res["render_" + name]["total_ms"]["median"]
                                                    / res["copy_" + name]["median"])
    window.free()

    # the sibling: hbam_sam_render over a decoded BAM whose text is of comparable size
    import numpy as np
    import genbam
    from hadoop_bam import read_sam_header
    bam = np.asarray(genbam.generate(records=max(1000, (a.mib << 20) // a.sam_bytes_per_record), seed=7))
    h = ctx.parse_header(bam)
    assert isinstance(h, dict), h
    names = [n for n, _ in read_sam_header(bam, ctx).refs]
    rc, dc = ctx.decode_split_device(bam, h["first_voffset"], (len(bam) << 16) | 0xffff, h["n_ref"])
    assert rc == 0, ctx.last_error()
    timings = []
    for k in range(a.warmup + a.reps):
        rc, t = ctx.sam_render_device(dc.ubuf, dc.rec_off, int(dc.n_records), names)
        assert rc == 0 and int(t.status) == 0, (rc, ctx.last_error())
        if k >= a.warmup:
            timings.append(ctx.timing())
    res["render_sam"] = stages(timings, int(t.text_len))
    res["render_sam"]["records"] = int(dc.n_records)
    res["copy_sam"] = copy_ms(int(t.text_len), a.warmup, a.reps)
    res["render_sam"]["bulk_over_copy"] = res["render_sam"]["resolve_ms"]["median"] / res["copy_sam"]["median"]
    res["render_sam"]["total_over_copy"] = res["render_sam"]["total_ms"]["median"] / res["copy_sam"]["median"]
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
