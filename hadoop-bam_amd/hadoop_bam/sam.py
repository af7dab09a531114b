"""Host-side mirror of Hadoop-BAM's SAM text input classes over the MI355X C ABI.

SAMFormat (SAMFormat.java:31-61), SAMRecordReader (SAMRecordReader.java:54-180, with the split
rule of its WorkaroundingStream) and SAMInputFormat (SAMInputFormat.java), same names, argument
meaning and exceptions.  The lines of a split become BAM records on the device
(hbam_sam_decode_split, hbam_sam.hip): what SAMRecordWritable.write sends through the shuffle
whatever the record was read from.  The header is parsed here.  htsjdk's SAMLineParser and
BAMRecordCodec are not in the reference tree: the per-line rules are restated from memory (parity
unpinned, DESIGN.md lists them).
"""
import os

import numpy as np

from . import _lib
from ._window import read_growing_window
from .formats import (BAMRecordBytes, FileSplit, IOException, LongWritable, SAMFormatException,  # noqa: F401
                      SAMRecordWritable, SeekableFile, compute_file_splits, context, raise_for)
from .output import SAMFileHeader

SAM_WINDOW_TAIL = 1 << 20  # bytes read past the split's end at first (the last line's tail)


class SAMUnsupportedException(NotImplementedError):
    """A line the device encoder does not restate (HBAM_EUNSUPPORTED): an H tag, a read name over 254
    bytes, more than 65535 CIGAR operations, float text outside the exactly rounded domain; or a split
    that begins inside the header."""


class SAMFormat:
    """SAMFormat.java:31-61."""
    SAM = "SAM"
    BAM = "BAM"

    @staticmethod
    def inferFromFilePath(path):
        name = os.path.basename(str(path))
        if name.endswith(".bam"):
            return SAMFormat.BAM
        if name.endswith(".sam"):
            return SAMFormat.SAM
        return None

    @staticmethod
    def inferFromData(data):
        """From the first byte of a stream, a path or a buffer: 0x1f -> BAM, '@' -> SAM."""
        if hasattr(data, "read") and not isinstance(data, SeekableFile):
            b = data.read(1)
        else:
            ss = SeekableFile(data)
            b = ss.read_at(0, 1)
            ss.close()
        if b == b"\x1f":
            return SAMFormat.BAM
        if b == b"@":
            return SAMFormat.SAM
        return None


def parse_sam_text_header(buf, complete):
    """The header in `buf` (the file's first bytes; complete: buf is the whole file) ->
    (header text, data_start, [(SN, LN)] in @SQ line order), or None when more bytes are needed.
    The header is the run of lines that begin with '@'; data_start is the offset of the first byte
    after the last of them."""
    pos, refs = 0, []
    while pos < len(buf) and buf[pos:pos + 1] == b"@":
        nl = buf.find(b"\n", pos)
        if nl < 0 and not complete:
            return None
        end = len(buf) if nl < 0 else nl
        line = buf[pos:end]
        if line.endswith(b"\r") and nl >= 0:
            line = line[:-1]
        f = line.split(b"\t")
        if f[0] == b"@SQ":
            sn = [x[3:] for x in f[1:] if x.startswith(b"SN:")]
            ln = [x[3:] for x in f[1:] if x.startswith(b"LN:")]
            if not sn or not ln:
                raise SAMFormatException("@SQ line without SN or LN: %r" % line)
            try:
                refs.append((sn[0], int(ln[0])))
            except ValueError:
                raise SAMFormatException("@SQ line whose LN is not a number: %r" % line)
        pos = len(buf) if nl < 0 else nl + 1
    if pos >= len(buf) and not complete:
        return None
    return bytes(buf[:pos]), pos, refs


def read_sam_text_header(source):
    """The header of a SAM text file, read over a growing prefix (a path, an open file, a buffer or
    a SeekableFile) -> (header text, data_start, SAMFileHeader).  The dictionary the device gets is
    the @SQ lines' SN in line order."""
    ss = SeekableFile(source)
    n = min(ss.length, 1 << 16)
    while True:
        h = parse_sam_text_header(ss.read_at(0, n), n >= ss.length)
        if h is not None:
            text, data_start, refs = h
            return text, data_start, SAMFileHeader(text, refs)
        n = min(ss.length, 4 * n)


def _raise(status, what):
    if status == _lib.HBAM_EUNSUPPORTED:
        raise SAMUnsupportedException(what)
    raise_for(status, what)


def read_split_columns(ctx, ss, start, length, data_start, table, n_ref):
    """hbam_sam_decode_split over the window of FileSplit [start, start + length): file bytes
    [start - 1 (data_start for a split at 0), start + length + tail), the tail growing from
    SAM_WINDOW_TAIL while the decode answers HBAM_EMORE -> (host columns, window base, window bytes)."""
    def call(window, base):
        cols = ctx.sam_decode_split(window, start, length, data_start, table, n_ref, text_base=base,
                                    file_len=ss.length)
        if cols["rc"]:
            _raise(cols["rc"], cols.get("error", ""))
        return cols

    base = min(start - 1 if start else data_start, ss.length)
    cols, window = read_growing_window(ss, base, start, length, SAM_WINDOW_TAIL, call)
    return cols, base, len(window)


class SAMRecordReader:
    """SAMRecordReader.java:54-180 over a FileSplit of a SAM text file: the split returns the lines
    whose first byte lies in [max(start, data_start), start + length).  The key is
    BAMRecordReader.getKey of the record, the value a SAMRecordWritable over the record's BAM bytes,
    as the BAM reader gives.  Only [start - 1 (data_start for a split at 0), end + tail) is read; the
    tail grows while the last line runs past it (HBAM_EMORE)."""

    def __init__(self):
        self.key = LongWritable()
        self.record = SAMRecordWritable()
        self.cols = None

    def initialize(self, split, conf=None, data=None):
        path = split.getPath()
        ss = SeekableFile(data if data is not None else path)
        _, data_start, header = read_sam_text_header(ss)
        self.header = header
        start, length = split.getStart(), split.getLength()
        ctx = context(conf)
        table = ctx.vcf_contig_table([n for n, _ in header.refs])
        cols, base, wlen = read_split_columns(ctx, ss, start, length, data_start, table, len(header.refs))
        self.window_bytes = wlen
        # the reference moves start to the first byte it reads: the header's end, or start - 1 (:130-139)
        self.start, self.end, self.file_len = (data_start if start == 0 else start - 1), start + length, ss.length
        self.cols, self.i = cols, -1
        ss.close()

    def nextKeyValue(self):
        c = self.cols
        if self.i + 1 < c["n"]:
            self.i += 1
            i = self.i
            self.key.set(int(c["key"][i]))
            o, bs = int(c["rec_off"][i]), int(c["block_size"][i])
            self.record.set(BAMRecordBytes(c["ubuf"][o:o + 4 + bs].tobytes()))
            return True
        self.i = c["n"]
        if c["status"] not in (_lib.HBAM_OK, _lib.HBAM_EMORE):
            _raise(c["status"], "SAM line %d of the split" % c["n"])
        return False

    def getCurrentKey(self):
        return self.key

    def getCurrentValue(self):
        return self.record

    def getProgress(self):  # :161-167, the stream position taken as the next unread line's offset
        c, i = self.cols, self.i
        pos = int(c["voffset"][i + 1]) if i + 1 < c["n"] else self.end
        if pos >= self.end or self.end <= self.start:
            return 1.0
        return float(np.float32(pos - self.start) / np.float32(self.end - self.start))

    def close(self):
        self.cols = None


class SAMInputFormat:
    """SAMInputFormat.java: plain byte splits of a splittable text file, read by SAMRecordReader."""

    def createRecordReader(self, split, conf=None):
        rr = SAMRecordReader()
        rr.initialize(split, conf)
        return rr

    def isSplitable(self, job=None, path=None):
        return True

    def getSplits(self, paths, split_size):
        """FileInputFormat.getSplits over `paths` (one path or a list) with this split size."""
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        out = []
        for p in paths:
            out += compute_file_splits(p, os.path.getsize(p), split_size)
        return out
