"""Host-side mirror of Hadoop-BAM's text VCF classes over the MI355X C ABI.

VCFFormat (VCFFormat.java:38-61), VCFRecordReader (VCFRecordReader.java:72-142) and the vcf-sort
plugin (cli/plugins/VCFSort.java), same names, argument meaning and exceptions.  The lines, the
fields and the keys come from libhbam.so (hbam_vcf.hip); the header is parsed here.  htsjdk's
AsciiLineReader, AsciiLineReaderIterator and VCFCodec are not in the reference tree: the line,
header and decode rules are restated from memory (parity unpinned, DESIGN.md lists them).

Lines end at a newline; a carriage return directly before it is not part of the line.  A lone
carriage return (not followed by a newline) is out of scope: it is an ordinary byte here.
"""
import os

import numpy as np

from ._window import read_growing_window
from .bcf import BCFDecodeRuntimeException, TribbleException  # noqa: F401  (the reader's exceptions)
from .bcf import _raise
from .formats import FileSplit, IOException, SeekableFile, context, raise_for  # noqa: F401  (FileSplit: the reader's split)

TRUST_EXTS_PROPERTY = "hadoopbam.vcf.trust-exts"

VCF_WINDOW_TAIL = 1 << 20  # bytes read past the split's end at first (the last line's tail)


class VCFFormat:
    """VCFFormat.java:31-61."""
    VCF = "VCF"
    BCF = "BCF"

    @staticmethod
    def inferFromFilePath(path):
        name = os.path.basename(str(path))
        if name.endswith(".bcf"):
            return VCFFormat.BCF
        if name.endswith(".vcf"):
            return VCFFormat.VCF
        return None

    @staticmethod
    def inferFromData(data):
        """From the first byte of a stream, a path or a buffer: 0x1f (BGZF) or 'B' -> BCF, '#' -> VCF."""
        if hasattr(data, "read") and not isinstance(data, SeekableFile):
            b = data.read(1)
        else:
            ss = SeekableFile(data)
            b = ss.read_at(0, 1)
            ss.close()
        if b in (b"\x1f", b"B"):
            return VCFFormat.BCF
        if b == b"#":
            return VCFFormat.VCF
        return None


def _contig_id(line):
    """The ID value of a ##contig=<...> line: key=value pairs separated by commas, a quoted value
    may hold commas, ID need not be the first key."""
    lt, gt = line.find(b"<"), line.rfind(b">")
    body = line[lt + 1:gt if gt > lt else len(line)]
    i, n = 0, len(body)
    while i < n:
        eq = body.find(b"=", i)
        if eq < 0:
            return None
        key = body[i:eq].strip()
        j = eq + 1
        if j < n and body[j:j + 1] == b'"':
            k = j + 1
            while k < n and body[k:k + 1] != b'"':
                k += 2 if body[k:k + 1] == b"\\" else 1
            val, j = body[eq + 2:k], k + 1
        else:
            k = body.find(b",", j)
            k = n if k < 0 else k
            val, j = body[eq + 1:k], k
        if key == b"ID":
            return val
        i = j + 1  # past the comma
    return None


def parse_vcf_header(buf, complete, name=""):
    """The header in `buf` (the file's first bytes; complete: buf is the whole file) ->
    (header bytes, contig IDs in line order, data_start), or None when more bytes are needed.
    The header is the run of '#' lines up to and including the #CHROM line."""
    pos, contigs = 0, []
    while True:
        nl = buf.find(b"\n", pos)
        if nl < 0 and not complete:
            return None
        end = len(buf) if nl < 0 else nl
        line = buf[pos:end]
        if line.endswith(b"\r") and nl >= 0:
            line = line[:-1]
        nxt = len(buf) if nl < 0 else nl + 1
        if line.startswith(b"##"):
            if line.startswith(b"##contig=<"):
                cid = _contig_id(line)
                if cid is not None:
                    contigs.append(cid)
        elif line.startswith(b"#CHROM"):
            return buf[:nxt], contigs, nxt
        else:
            raise IOException("No VCF header found in %s" % name)
        if nxt >= len(buf):
            if complete:
                raise IOException("No VCF header found in %s" % name)
            return None
        pos = nxt


def read_vcf_header(ss, name=""):
    """VCFCodec.readHeader over a growing prefix of the stream -> (header bytes, contig IDs (bytes, in
    ##contig line order; contigDict maps each to its ordinal, a later duplicate overwriting),
    data_start = the offset of the line after #CHROM)."""
    ss = SeekableFile(ss)
    n = min(ss.length, 1 << 16)
    while True:
        h = parse_vcf_header(ss.read_at(0, n), n >= ss.length, name)
        if h is not None:
            return h
        n = min(ss.length, 4 * n)


class VCFRecord:
    """What the key and the reference's test read of a VariantContext (getChr, getStart, getEnd, ID,
    REF, ALT) and the raw line, which a Java caller hands to VCFCodec.  getEnd is POS + len(REF) - 1:
    an INFO END= override is not applied."""

    def __init__(self, reader, i):
        c = reader.cols
        o = int(c["line_off"][i]) - reader.base
        self._line = reader.window[o:o + int(c["line_len"][i])]
        self._tab = [int(x) for x in c["tab"][i]]
        self._pos, self._ref_len = int(c["pos"][i]), int(c["ref_len"][i])

    def _field(self, k):
        return self._line[(self._tab[k - 1] + 1 if k else 0):self._tab[k]]

    def getLine(self):
        return bytes(self._line)

    def getChr(self):
        return self._field(0).decode("latin-1")

    def getStart(self):
        return self._pos

    def getEnd(self):
        return self._pos + self._ref_len - 1

    def getID(self):
        return self._field(2).decode("latin-1")

    def getReference(self):
        return self._field(3).decode("latin-1")

    def getAlternateAlleles(self):
        return self._field(4).decode("latin-1").split(",")


def read_split_columns(ctx, ss, start, length, data_start, table):
    """hbam_vcf_decode_split over the window of FileSplit [start, start + length): file bytes
    [start - 1 (data_start for a split at 0), start + length + tail), the tail growing from
    VCF_WINDOW_TAIL while the decode answers HBAM_EMORE -> (host columns, window base, window)."""
    def call(window, base):
        cols = ctx.vcf_decode_split(window, start, length, data_start, table, text_base=base,
                                    file_len=ss.length)
        if cols["rc"]:
            raise_for(cols["rc"], cols.get("error", ""))
        return cols

    base = min(start - 1 if start else data_start, ss.length)
    cols, window = read_growing_window(ss, base, start, length, VCF_WINDOW_TAIL, call)
    return cols, base, window


class VCFRecordReader:
    """VCFRecordReader.java:72-142 over a FileSplit of an uncompressed VCF file;
    key = contigDict ordinal (or the CHROM's MurmurHash3) << 32 | (POS - 1).  Only
    [start - 1 (data_start for a split at 0), end + tail) is read; the tail grows while the last
    line runs past it (HBAM_EMORE)."""

    def __init__(self):
        self.cols = None

    def initialize(self, split, conf=None, data=None):
        path = split.getPath()
        ss = SeekableFile(data if data is not None else path)
        _, contigs, data_start = read_vcf_header(ss, path)
        start, length = split.getStart(), split.getLength()
        self.start, self.length = start, length
        if start == 0 and (data_start >= ss.length or ss.read_at(data_start, 1) == b"#"):
            raise IOException("Empty VCF file %s" % path)
        ctx = context(conf)
        cols, base, window = read_split_columns(ctx, ss, start, length, data_start,
                                                ctx.vcf_contig_table(contigs))
        self.window_bytes = len(window)
        self.base, self.window, self.file_len = base, window, ss.length
        self.cols, self.i, self.key = cols, -1, None

    def nextKeyValue(self):
        c = self.cols
        if self.i + 1 < c["n"]:
            self.i += 1
            self.key = int(c["key"][self.i])
            return True
        self.i = c["n"]
        _raise(c["status"], "VCFCodec.decode")
        return False

    def getCurrentKey(self):
        return self.key

    def getCurrentValue(self):
        return VCFRecord(self, self.i)

    def getProgress(self):  # :121-123: reader.getPosition() / length
        if self.length == 0:
            return 1.0
        c, i = self.cols, self.i
        if i + 1 < c["n"]:
            nxt = int(c["line_off"][i + 1])
        elif 0 <= i < c["n"] or (i == c["n"] and i > 0):
            j = min(i, c["n"] - 1)  # the next unread line starts after this one's newline
            e = int(c["line_off"][j]) + int(c["line_len"][j]) - self.base
            nl = self.window.find(b"\n", e)
            nxt = self.file_len if nl < 0 else self.base + nl + 1
        else:
            nxt = self.base
        return float(np.float32(nxt - (self.start - 1 if self.start else 0)) / np.float32(self.length))

    def close(self):
        self.cols = self.window = None


def vcf_sort(in_path, out_path, conf=None, data=None):
    """The vcf-sort plugin with -o (cli/plugins/VCFSort.java): the header's bytes as they are, then
    the data lines in the order of their keys, each ended by a newline.  The whole file is decoded
    on one GPU, the keys go through the stable hbam_sort_keys (equal keys keep input order) and
    hbam_vcf_gather_lines packs the lines.  A BCF input (BGZF or plain, by its first byte) is decoded
    on the device as one split, its keys sorted the same way, and its records rendered as VCF lines
    where they stand (VCFRecordWriter.write_device with the permutation).  Output is VCF text only: a
    .bcf output (BCFRecordWriter) is not restated."""
    import ctypes as C
    if VCFFormat.inferFromFilePath(out_path) == VCFFormat.BCF:
        raise NotImplementedError("vcf_sort writes VCF text only: %s" % out_path)
    ctx = context(conf)
    if VCFFormat.inferFromData(data if data is not None else in_path) == VCFFormat.BCF:
        return _vcf_sort_bcf(ctx, data if data is not None else in_path, out_path)
    ss = SeekableFile(data if data is not None else in_path)
    header, contigs, data_start = read_vcf_header(ss, in_path)
    if data_start >= ss.length or ss.read_at(data_start, 1) == b"#":
        raise IOException("Empty VCF file %s" % in_path)
    body = ss.read_at(data_start, ss.length - data_start)
    rc, d = ctx.vcf_decode_split_device(body, 0, ss.length, data_start, ctx.vcf_contig_table(contigs),
                                        text_base=data_start, file_len=ss.length, keep_text=True)
    raise_for(rc, ctx.last_error())
    n = int(d.n)
    perm = C.c_void_p()
    rc = ctx.L.hbam_device_alloc(ctx.h, 4 * max(n, 1), C.byref(perm))
    raise_for(rc, ctx.last_error())
    try:
        rc = ctx.L.hbam_sort_keys(ctx.h, d.key, n, None, perm)
        raise_for(rc, ctx.last_error())
        sort_ms = ctx.timing()["total_ms"]
        lines = ctx.vcf_gather_lines(d, perm, n)
        gather_ms = ctx.timing()["pools_ms"]
    finally:
        ctx.L.hbam_device_free(ctx.h, perm)
    with open(out_path, "wb") as f:
        f.write(header)
        f.write(lines)
    _raise(int(d.status), "VCFCodec.decode")  # a line that does not decode fails the job
    return {"n": n, "sort_ms": sort_ms, "gather_ms": gather_ms}


def _vcf_sort_bcf(ctx, src, out_path):
    """vcf_sort over a BCF input: one whole-file hbam_bcf_decode_split, the stable hbam_sort_keys on
    the keys, then hbam_vcf_render over the device columns in that order; only the text (and the
    records the device defers) leave the device."""
    import ctypes as C
    from .bcf import read_bcf_header
    from .vcf_text import VCFRecordWriter, read_vcf_header_from
    header = read_vcf_header_from(src, ctx)
    ss = SeekableFile(src)
    h = read_bcf_header(ss, ctx)
    body = ss.read_at(0, ss.length)
    ss.close()
    if h["bgzf"]:
        rc, d = ctx.bcf_decode_split_device(body, h, h["first_voffset"], (len(body) << 16) | 0xffff)
    else:
        rc, d = ctx.bcf_decode_split_device(body, h, 0, len(body))
    raise_for(rc, ctx.last_error())
    n = int(d.n_records)
    perm = C.c_void_p()
    rc = ctx.L.hbam_device_alloc(ctx.h, 4 * max(n, 1), C.byref(perm))
    raise_for(rc, ctx.last_error())
    try:
        rc = ctx.L.hbam_sort_keys(ctx.h, d.key, n, None, perm)
        raise_for(rc, ctx.last_error())
        sort_ms = ctx.timing()["total_ms"]
        w = VCFRecordWriter(out_path, header, True, ctx)
        try:
            res = w.write_device(d, perm, n)
        finally:
            w.close()
    finally:
        ctx.L.hbam_device_free(ctx.h, perm)
    _raise(int(d.status), "BCF2Codec.decode")  # a record that does not decode fails the job
    return {"n": n, "sort_ms": sort_ms, "render_ms": res["timing"]["total_ms"], "deferred": len(res["deferred"])}
