"""The summarize plugin end to end (cli/plugins/chipster/Summarize.java) and SummarySort
(chipster/SummarySort.java), host mirror of the reference classes over the device entry points:

* SummaryGroup, SummarizeReducer (Summarize.java:466-561, :812-828): the reference's stateful
  setup / reduce / cleanup API; the key-ordered batch it is fed is reduced on the device
  (hbam_summarize_reduce) at cleanup();
* SummarizeOutputFormat (:758-810): the lines of one named output as BGZF members (bgzf_compress),
  no terminator;
* summarize(): the plugin's run() — SummarizeInputFormat's splits decoded window by window, their
  ranges (hbam_summarize_ranges) appended to device buffers, one hbam_summarize_reduce over all of
  them (the shuffle's total order + ONE reducer), the summary files written under the reference's
  names; --sort is the reduce's sort_output;
* summary_sort(): SummarySort — the file inflated on the device, hbam_summary_keys,
  hbam_sort_keys, hbam_summary_gather_lines, bgzf_compress.

Not restated: more than one reduce partition, BlockCompressedLineRecordReader's
per-split cut-off, SAM text input, the CLI option parser.

No CPU fallback: the work runs in libhbam.so; without it _lib raises HbamUnavailable."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .consumers import IndexOutOfBoundsException, Range, RangeCount, SummarizeInputFormat, _raise
from .formats import (Configuration, NumberFormatException, WINDOW_BYTES_PROPERTY, compute_file_splits, context,
                      raise_for, read_header)
from .output import EMPTY_GZIP_BLOCK

SPLIT_SIZE_PROPERTY = "mapred.max.split.size"
SUMMARY_LEVELS_PROP = "summarize.summary.levels"


def getSummaryName(lvl, reverseStrand):
    """Summarize.java:447-450"""
    return "summary" + str(lvl) + ("r" if reverseStrand else "f")


def parse_levels(levels):
    """run()'s validation of LEVELS (:129-142, the plugin's messages), and what MultipleOutputs
    .addNamedOutput rejects when the outputs are declared (:307-314): a name that is not plain
    letters and digits, a name declared twice.  -> (level texts, ints)"""
    texts = levels.split(",") if isinstance(levels, str) else [str(x) for x in levels]
    vals = []
    for l in texts:
        try:
            v = _parse_int(l)
        except ValueError:
            raise ValueError("summarize :: summary level '%s' is not an integer!" % l)
        if v <= 0:
            raise ValueError("summarize :: summary level '%d' is not positive!" % v)
        vals.append(v)
    for l in texts:
        if not (l.isascii() and l.isdigit()):
            raise ValueError("Named output name cannot have characters other than [A-Za-z0-9]: summary%sf" % l)
    if len(set(texts)) != len(texts):
        dup = [l for l in texts if texts.count(l) > 1][0]
        raise ValueError("Named output 'summary%sf' already alreadyDefined" % dup)
    return texts, vals


def _parse_int(s):
    """Integer.parseInt: [+-]? ASCII digits, inside int32."""
    body = s[1:] if s[:1] in ("+", "-") else s
    if not body or not (body.isascii() and body.isdigit()):
        raise ValueError(s)
    v = int(s)
    if not -(1 << 31) <= v < (1 << 31):
        raise ValueError(s)
    return v


class SummaryGroup:
    """Summarize.java:812-828"""

    def __init__(self, lvl, name):
        self.level, self.outName = int(lvl), name
        self.reset()

    def reset(self):
        self.sumBeg = self.sumEnd = 0
        self.count = 0


class SummarizeReducer:
    """Summarize.java:466-561 with the reference's call sequence: setup(levels), reduce(key,
    ranges) for every key in the shuffle's order, cleanup().  reduce() only collects: the groups
    are an order-deterministic function of the whole key-ordered stream, so cleanup() hands it to
    hbam_summarize_reduce in one call and `outputs` then holds, per named output, the RangeCount
    lines MultipleOutputs would have received (text, one line per group, '\\n' ended)."""

    def __init__(self, conf=None):
        self.conf = conf
        self.summaryGroupsR, self.summaryGroupsF = [], []
        self.outputs = {}
        self._k, self._b, self._e, self._r = [], [], [], []

    def setup(self, levels):
        self.levels, vals = parse_levels(levels)
        for s, lvl in zip(self.levels, vals):
            self.summaryGroupsR.append(SummaryGroup(lvl, getSummaryName(s, True)))
            self.summaryGroupsF.append(SummaryGroup(lvl, getSummaryName(s, False)))

    def reduce(self, key, ranges):
        k = key.get() if hasattr(key, "get") else int(key)
        for r in ranges:
            self._k.append(k)
            self._b.append(r.beg)
            self._e.append(r.end)
            self._r.append(1 if r.reverseStrand else 0)

    def cleanup(self):
        ctx = context(self.conf)
        lv = [g.level for g in self.summaryGroupsF]
        res = ctx.summarize_reduce(np.asarray(self._k, np.int64), np.asarray(self._b, np.int32),
                                   np.asarray(self._e, np.int32), np.asarray(self._r, np.uint8), lv)
        self.result = res
        off = res["text_off"]
        for i in range(len(lv)):
            for s, groups in ((0, self.summaryGroupsF), (1, self.summaryGroupsR)):
                k = 2 * i + s
                self.outputs[groups[i].outName] = res["text"][int(off[k]):int(off[k + 1])]
        self._k, self._b, self._e, self._r = [], [], [], []

    def rangeCounts(self, name):
        """The RangeCount values of one named output."""
        out = []
        for line in self.outputs[name].splitlines():
            rid, b, e, c = (int(x) for x in line.split(b"\t"))
            out.append(RangeCount(Range(b, e), c, rid))
        return out


class SummarizeOutputFormat:
    """Summarize.java:758-810: TextOutputFormat's lines through a BlockCompressedOutputStream that
    is flushed, not closed: BGZF members without the terminator."""

    def __init__(self, conf=None):
        self.conf = conf

    def getRecordWriter(self, out):
        return _SummaryWriter(out, context(self.conf))


class _SummaryWriter:
    def __init__(self, out, ctx):
        self.f = open(out, "wb") if isinstance(out, (str, os.PathLike)) else out
        self.owned = self.f is not out
        self.ctx = ctx
        self.parts = []

    def write(self, key, value):  # NullWritable key; value: RangeCount, or text lines as bytes
        self.parts.append(value if isinstance(value, (bytes, bytearray)) else (str(value) + "\n").encode())

    def write_device(self, buf):
        """Lines already on the device (a DeviceBuffer / device tensor)."""
        self._flush()
        if buf.nbytes:
            self.f.write(self.ctx.bgzf_compress(buf).tobytes())

    def _flush(self):
        text = b"".join(self.parts)
        self.parts = []
        if text:
            self.f.write(self.ctx.bgzf_compress(text).tobytes())

    def close(self, terminator=False):
        self._flush()
        if terminator:
            self.f.write(EMPTY_GZIP_BLOCK)
        if self.owned:
            self.f.close()


class _DevAppend:
    """A growing device array (hbam_device_alloc): windows' context-owned outputs are copied in."""

    def __init__(self, ctx, itemsize):
        self.ctx, self.itemsize, self.n, self.cap, self.buf = ctx, itemsize, 0, 0, None

    def append(self, ptr, count):
        if not count:
            return
        if self.n + count > self.cap:
            cap = max(self.n + count, 2 * self.cap, 1 << 16)
            nb = self.ctx.device_alloc(cap * self.itemsize)
            if self.n:
                self.ctx.device_copy(nb.ptr, self.buf.ptr, self.n * self.itemsize)
            if self.buf is not None:
                self.buf.free()
            self.buf, self.cap = nb, cap
        self.ctx.device_copy(self.buf.ptr + self.n * self.itemsize, ptr, count * self.itemsize)
        self.n += count

    @property
    def ptr(self):
        return self.buf.ptr if self.buf is not None else 0

    def free(self):
        if self.buf is not None:
            self.buf.free()
        self.buf = None


def output_paths(work_dir, texts, in_path, out_dir=None):
    """The files summarize() writes, in (level-major, f then r) order: merged
    <out_dir>/<in name>-summary<L><s> (getFinalSummaryName, mergeOne), or the single reducer's
    unmerged part <work_dir>/<in name>-summary<L><s>-000000 (Utils.getMergeableWorkFile)."""
    name = os.path.basename(str(in_path))
    out = []
    for l in texts:
        for rev in (False, True):
            fn = name + "-" + getSummaryName(l, rev)
            out.append(os.path.join(out_dir, fn) if out_dir is not None else os.path.join(work_dir, fn + "-000000"))
    return out


def summarize(work_dir, levels, in_path, out_dir=None, sort=False, conf=None):
    """The summarize plugin's run() with one reduce task: every (level, strand) summary of the BAM
    at in_path.  levels: the plugin's comma-separated LEVELS.  With out_dir the merged files (BGZF
    members + the 28-byte terminator) go there; without it the reducer's parts stay in work_dir
    without a terminator, as the plugin leaves them.  sort: the --sort leg (SummarySort on every
    file).  A split whose reader raises fails the job: the exception propagates and nothing is
    written.  Returns dict(files, n_ranges, n_lines, timing)."""
    texts, vals = parse_levels(levels)
    conf = conf if conf is not None else Configuration()
    ctx = context(conf)
    paths = output_paths(work_dir, texts, in_path, out_dir)
    size = os.path.getsize(in_path)
    split_size = int(conf.get(SPLIT_SIZE_PROPERTY, 64 << 20))
    fmt = SummarizeInputFormat()
    splits = fmt.getSplits(compute_file_splits(in_path, size, split_size), conf)
    data = np.memmap(in_path, np.uint8, "r") if size else np.zeros(0, np.uint8)
    h = read_header(data, ctx)
    if isinstance(h, int):
        raise_for(h, "cannot read SAM header")
    window = int(conf.get(WINDOW_BYTES_PROPERTY, 1 << 30))
    cols = [_DevAppend(ctx, 8), _DevAppend(ctx, 4), _DevAppend(ctx, 4), _DevAppend(ctx, 1)]
    ranges_ms = 0.0
    try:
        for sp in splits:
            gen = ctx.split_stream(data, sp.getStartVirtualOffset(), sp.getEndVirtualOffset(), h["n_ref"], window,
                                   host=False)
            try:
                for d in gen:
                    r = _lib.RangesC()
                    rc = ctx.L.hbam_summarize_ranges(ctx.h, C.byref(d), C.byref(r))
                    if rc:
                        raise RuntimeError("hbam_summarize_ranges failed (%d): %s" % (rc, ctx.last_error()))
                    ranges_ms += ctx.timing()["total_ms"]
                    for col, p in zip(cols, (r.key, r.beg, r.end, r.rev)):
                        col.append(p, int(r.n))
                    if r.status not in (0, _lib.HBAM_EMORE):
                        _raise(int(r.status), "SummarizeRecordReader.nextKeyValue")
            finally:
                gen.close()
        n = cols[0].n
        s = ctx.summarize_reduce_device(cols[0].ptr, cols[1].ptr, cols[2].ptr, cols[3].ptr, n, vals, sort)
        timing = ctx.timing()
        text_off = ctx._d2h(s.text_off, int(s.n_streams) + 1, np.uint64)
        n_lines = int(s.n_lines)
        members = []
        for k in range(len(paths)):  # compress every stream before the first file is created
            a, b = int(text_off[k]), int(text_off[k + 1])
            members.append(ctx.bgzf_compress(_lib.DeviceBuffer(ctx, s.text + a, b - a, False)).tobytes()
                           if b > a else b"")
    finally:
        for col in cols:
            col.free()
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    os.makedirs(work_dir, exist_ok=True)
    for p, m in zip(paths, members):
        with open(p, "wb") as f:
            f.write(m)
            if out_dir is not None:
                f.write(EMPTY_GZIP_BLOCK)
    return dict(files=paths, n_ranges=n, n_lines=n_lines,
                timing=dict(ranges_ms=ranges_ms, reduce_ms=timing["total_ms"], shuffle_sort_ms=timing["scan_ms"],
                            line_sort_ms=timing["walk_ms"]))


def _inflate_file(ctx, data):
    """The inflated bytes of a BGZF file (device scan + inflate)."""
    if len(data) == 0:
        return np.zeros(0, np.uint8)
    rc, blocks = ctx.scan_blocks(data)
    if rc:
        raise_for(rc, ctx.last_error())
    rc, u, _, st = ctx.inflate(data, blocks, check_crc=True)
    if rc:
        raise_for(rc, ctx.last_error())
    bad = [int(x) for x in st if x]
    if bad:
        raise_for(bad[0], "BlockCompressedInputStream: a block of the summary file does not inflate")
    return u


def summary_sort(work_dir, in_path, out_path=None, conf=None):
    """The summarysort plugin (SummarySort.java) with one reduce task over the summary file at
    in_path read as one split: its lines in the stable order of getKey0(rid, pos).  With out_path
    the merged file (members + terminator); without it the part <work_dir>/<in name>-000000, no
    terminator.  A line SortRecordReader cannot key fails the job: the exception propagates and
    nothing is written.  Returns dict(file, n, timing)."""
    conf = conf if conf is not None else Configuration()
    ctx = context(conf)
    with open(in_path, "rb") as f:
        data = np.frombuffer(f.read(), np.uint8)
    text = _inflate_file(ctx, data)
    dtext = ctx.upload(text)
    perm = out = None
    try:
        s = ctx.summary_keys_device(dtext)
        keys_ms = ctx.timing()["total_ms"]
        if s.status:
            if s.status == _lib.HBAM_EINDEX:
                raise IndexOutOfBoundsException("SortRecordReader.nextKeyValue: line %d" % int(s.n))
            raise_for(int(s.status), "SortRecordReader.nextKeyValue: line %d" % int(s.n))
        n = int(s.n)
        sort_ms = 0.0
        if n:
            perm = ctx.device_alloc(4 * n)
            rc = ctx.L.hbam_sort_keys(ctx.h, C.c_void_p(s.key), n, None, C.c_void_p(perm.ptr))
            raise_for(rc, ctx.last_error())
            sort_ms = ctx.timing()["total_ms"]
        out = ctx.summary_gather_lines(s, C.c_void_p(perm.ptr) if perm is not None else None, n)
        gather_ms = ctx.timing()["pools_ms"]
        members = ctx.bgzf_compress(out).tobytes() if out.nbytes else b""
    finally:
        for b in (dtext, perm, out):
            if b is not None:
                b.free()
    if out_path is not None:
        path = out_path
    else:
        os.makedirs(work_dir, exist_ok=True)
        path = os.path.join(work_dir, os.path.basename(str(in_path)) + "-000000")
    with open(path, "wb") as f:
        f.write(members)
        if out_path is not None:
            f.write(EMPTY_GZIP_BLOCK)
    return dict(file=path, n=n, timing=dict(keys_ms=keys_ms, sort_ms=sort_ms, gather_ms=gather_ms))


__all__ = ["NumberFormatException", "Range", "RangeCount", "SummarizeInputFormat", "SummarizeOutputFormat",
           "SummarizeReducer", "SummaryGroup", "getSummaryName", "output_paths", "parse_levels", "summarize",
           "summary_sort"]
