"""Host-side mirror of Hadoop-BAM's text write formats for reads over the MI355X C ABI.

FastqOutputFormat / FastqRecordWriter (FastqOutputFormat.java) and QseqOutputFormat /
QseqRecordWriter (QseqOutputFormat.java): same names, argument meaning, configuration properties
and exceptions.  The text itself - the id line or the leading QSEQ fields, the sequence, the quality
conversion and its range checks - is rendered by libhbam.so (hbam_fragtext.hip, hbam_frag_render);
this module buffers the fragments into columns, hands them over and raises what the status says.

write(key, fragment) buffers SequencedFragments as host columns and a string pool (the render's
window) and renders when _FLUSH_BYTES are buffered, at close() and, for FASTQ, whenever `key is
None` changes (the id line's source is one flag per device call).  When a render reports a failing
record, the records before it are written, then the bytes of that record the reference's stream
already holds, and the reference's exception is raised: FormatException, RuntimeException, or
SeqUnsupportedException where the device path does not restate the reference (include/hbam.h).

write_split() and convert() are the device-resident path: a split's window is uploaded once,
decoded (hbam_fastq_decode_split / hbam_qseq_decode_split) and rendered from the device columns and
the same device window; only the text, or its compressed form, comes back.

Compression.  getRecordWriter(path, conf, compress=True) appends ".gz" as GzipCodec's extension and
writes the rendered text from device memory through the device BGZF compressor (Context.
bgzf_compress), followed by the 28-byte BGZF terminator at close().  BGZF members are gzip members,
so any gzip reader (GzipCodec, zlib, fastq.py's own reader) inflates the file to the same text; the
file's bytes are not GzipCodec's (one deflate stream from java.util.zip), which are out of scope,
as are the other codecs.

Out of scope: SequencedFragment's Writable wire form.
"""
import os

import numpy as np

from . import _lib
from .fastq import (BaseQualityEncoding, FastqRecordReader, QseqRecordReader, RuntimeException,
                    SeqUnsupportedException, SEQ_WINDOW_TAIL, _codec, _gunzip)
from .formats import FormatException, SeekableFile, context, raise_for
from .output import EMPTY_GZIP_BLOCK

_FLUSH_BYTES = 64 << 20  # pool and string bytes buffered before a device render
_INT_FIELDS = (("run", "runNumber"), ("lane", "lane"), ("tile", "tile"), ("xpos", "xpos"), ("ypos", "ypos"),
               ("read", "read"), ("filter_passed", "filterPassed"), ("control", "controlNumber"))
_STR_FIELDS = (("instrument", "instrument"), ("flowcell", "flowcellId"), ("index", "indexSequence"))
_FORMATS = {"fastq": _lib.HBAM_FRAG_FASTQ, "qseq": _lib.HBAM_FRAG_QSEQ}


def _bytes(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


class _SeqRecordWriter:
    """What the two writers share: setConf, the column buffer, the device render and close."""
    _FMT = None
    CONF_BASE_QUALITY_ENCODING = None
    CONF_BASE_QUALITY_ENCODING_DEFAULT = None

    def __init__(self, conf=None, out=None, ctx=None, compress=False):
        self.conf = conf if conf is not None else {}
        self._own = isinstance(out, (str, os.PathLike))
        self.out = open(out, "wb") if self._own else out
        self.compress = bool(compress)
        self._ctx = ctx
        self.setConf(self.conf)
        self._reset()

    def setConf(self, conf):
        setting = conf.get(self.CONF_BASE_QUALITY_ENCODING, self.CONF_BASE_QUALITY_ENCODING_DEFAULT)
        if setting == "illumina":
            self.baseQualityFormat = BaseQualityEncoding.Illumina
        elif setting == "sanger":
            self.baseQualityFormat = BaseQualityEncoding.Sanger
        else:
            raise RuntimeException("Invalid property value '%s' for %s.  Valid values are 'illumina' or 'sanger'"
                                   % (setting, self.CONF_BASE_QUALITY_ENCODING))

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = context(self.conf)
        return self._ctx

    def _encoding(self):
        return (_lib.HBAM_QUAL_ILLUMINA if self.baseQualityFormat == BaseQualityEncoding.Illumina
                else _lib.HBAM_QUAL_SANGER)

    # ---- the column buffer ------------------------------------------------------------------------
    def _reset(self):
        self._present = []
        self._ints = {k: [] for k, _ in _INT_FIELDS}
        self._strs = {k: [] for k, _ in _STR_FIELDS}
        self._pools = {k: bytearray() for k in ("key", "seq", "qual")}
        self._offs = {k: [0] for k in ("key", "seq", "qual")}
        self._window = bytearray()
        self._keyed = None
        self._bytes = 0

    def write(self, key, fragment):
        keyed = key is not None and self._FMT == "fastq"
        if self._present and self._FMT == "fastq" and keyed != self._keyed:
            self._flush()
        self._keyed = keyed
        p = 0
        for col, attr in _INT_FIELDS:
            v = getattr(fragment, attr)
            if v is not None:
                p |= _lib.FRAG_PRESENT[col]
            self._ints[col].append(0 if v is None else int(v))
        for col, attr in _STR_FIELDS:
            v = getattr(fragment, attr)
            if v is None:
                self._strs[col].append((0, 0))
            else:
                p |= _lib.FRAG_PRESENT[col]
                b = _bytes(v)
                self._strs[col].append((len(self._window), len(b)))
                self._window += b
        self._present.append(p)
        for name, b in (("key", _bytes(key) if keyed else b""), ("seq", _bytes(fragment.sequence)),
                        ("qual", _bytes(fragment.quality))):
            self._pools[name] += b
            self._offs[name].append(len(self._pools[name]))
            self._bytes += len(b)
        self._bytes += 64
        if self._bytes + len(self._window) >= _FLUSH_BYTES:
            self._flush()

    def _flush(self):
        n = len(self._present)
        if not n:
            return
        cols = {"n": n, "present": np.array(self._present, np.uint32)}
        for k, _ in _INT_FIELDS:
            cols[k] = np.array(self._ints[k], np.int64).astype(np.int32)
        for k, _ in _STR_FIELDS:
            cols[k] = np.array(self._strs[k], np.uint32).reshape(n, 2)
        for k in ("key", "seq", "qual"):
            cols[k] = np.frombuffer(bytes(self._pools[k]), np.uint8)
            cols[k + "_off"] = np.array(self._offs[k], np.uint64)
        window, keyed = bytes(self._window), self._keyed
        self._reset()
        self._render(cols, window, _lib.HBAM_FRAG_USE_KEY if keyed else 0)

    # ---- the device render -------------------------------------------------------------------------
    def _render(self, cols, window, flags, n=None, perm=None):
        ctx = self.ctx
        rc, t = ctx.frag_render_device(cols, window, n, _FORMATS[self._FMT], self._encoding(), flags, perm)
        if rc:
            raise_for(rc, ctx.last_error())
        held = int(t.text_len) + int(t.partial_len)  # what the reference's stream holds
        if held:
            text = _lib.DeviceBuffer(ctx, t.text, held, False)
            if self.compress:
                self.out.write(ctx.bgzf_compress(text).tobytes())
            else:
                self.out.write(ctx.download(text.ptr, held)[:held].tobytes())
        status = int(t.status)
        if status != _lib.HBAM_OK:
            msg = "%s record %d of the batch" % (self._FMT, int(t.err_record))
            if status == _lib.HBAM_ESEQFORMAT:
                raise FormatException("base quality score out of range for Sanger format: " + msg)
            if status == _lib.HBAM_ERUNTIME:
                raise RuntimeException("output quality score over allowed range.  Maybe you meant to write in "
                                       "Sanger format? " + msg)
            if status == _lib.HBAM_EUNSUPPORTED:
                raise SeqUnsupportedException("a byte >= 0x80 in the sequence or the quality: " + msg)
            raise_for(status, msg)

    def write_split(self, cols, window=None, src_format=None, n=None, perm=None):
        """The records of one decoded split, rendered where they stand: cols = the device
        FragColumnsC of Context.frag_decode_split_device (or host columns, or a FastqRecordReader /
        QseqRecordReader, whose columns, window and format are taken), window = the bytes its string
        pairs point into (a _lib.DeviceBuffer, a device tensor or host bytes), src_format = "fastq" /
        "qseq".  A QSEQ source's index column is the raw field (HBAM_FRAG_INDEX_DOTS); FASTQ to FASTQ
        keeps the keys."""
        self._flush()
        if hasattr(cols, "cols") and hasattr(cols, "_FMT"):  # a reader
            cols, window, src_format = cols.cols, cols.window, cols._FMT
        flags = _lib.HBAM_FRAG_INDEX_DOTS if src_format == "qseq" else 0
        if src_format == "fastq" and self._FMT == "fastq":
            flags |= _lib.HBAM_FRAG_USE_KEY
        self._render(cols, b"" if window is None else window, flags, n, perm)

    def close(self, task=None):
        if self.out is None:
            return
        self._flush()
        if self.compress:
            self.out.write(EMPTY_GZIP_BLOCK)
        if hasattr(self.out, "flush"):
            self.out.flush()
        if self._own:
            self.out.close()
        self.out = None


class FastqRecordWriter(_SeqRecordWriter):
    """FastqOutputFormat.FastqRecordWriter (FastqOutputFormat.java:70-153): key None = the Illumina
    id of makeId, else the key is the id line."""
    _FMT = "fastq"
    CONF_BASE_QUALITY_ENCODING = "hbam.fastq-output.base-quality-encoding"
    CONF_BASE_QUALITY_ENCODING_DEFAULT = "sanger"


class QseqRecordWriter(_SeqRecordWriter):
    """QseqOutputFormat.QseqRecordWriter (QseqOutputFormat.java:66-165): the key is ignored."""
    _FMT = "qseq"
    CONF_BASE_QUALITY_ENCODING = "hbam.qseq-output.base-quality-encoding"
    CONF_BASE_QUALITY_ENCODING_DEFAULT = "illumina"


class _SeqOutputFormat:
    _WRITER = None

    def getRecordWriter(self, path, conf=None, compress=False, ctx=None):
        """The writer over `path` (a file name; with compress ".gz" is appended, see the module's
        notes on compression) or an open binary stream."""
        if compress and isinstance(path, (str, os.PathLike)):
            path = str(path) + ".gz"
        return self._WRITER(conf, path, ctx=ctx, compress=compress)


class FastqOutputFormat(_SeqOutputFormat):
    """FastqOutputFormat.java:54-186."""
    CONF_BASE_QUALITY_ENCODING = FastqRecordWriter.CONF_BASE_QUALITY_ENCODING
    CONF_BASE_QUALITY_ENCODING_DEFAULT = FastqRecordWriter.CONF_BASE_QUALITY_ENCODING_DEFAULT
    FastqRecordWriter = FastqRecordWriter
    _WRITER = FastqRecordWriter


class QseqOutputFormat(_SeqOutputFormat):
    """QseqOutputFormat.java:61-198."""
    CONF_BASE_QUALITY_ENCODING = QseqRecordWriter.CONF_BASE_QUALITY_ENCODING
    CONF_BASE_QUALITY_ENCODING_DEFAULT = QseqRecordWriter.CONF_BASE_QUALITY_ENCODING_DEFAULT
    QseqRecordWriter = QseqRecordWriter
    _WRITER = QseqRecordWriter


# ---- the device-resident conversion -------------------------------------------------------------
_READERS = {"fastq": FastqRecordReader, "qseq": QseqRecordReader}
_OUTPUTS = {"fastq": FastqOutputFormat, "qseq": QseqOutputFormat}


def _decode_split_device(ctx, fmt, ss, start, length, enc, filter_qc):
    """One split's window uploaded once and decoded on the device -> (device columns, the window's
    DeviceBuffer); the window grows x4 from SEQ_WINDOW_TAIL while the decode answers HBAM_EMORE."""
    base = min(start if fmt == "fastq" else max(start - 1, 0), ss.length)
    tail = SEQ_WINDOW_TAIL
    while True:
        stop = ss.length if length is None else max(base, min(ss.length, start + length + tail))
        window = ctx.upload(ss.read_at(base, stop - base))
        rc, d = ctx.frag_decode_split_device(fmt, window, start, length, enc, filter_qc, text_base=base,
                                             file_len=ss.length)
        if rc:
            window.free()
            raise_for(rc, ctx.last_error())
        if int(d.status) != _lib.HBAM_EMORE or stop == ss.length:
            return d, window
        window.free()
        tail *= 4


def convert(src, dst, src_format, dst_format, conf=None, split_size=None, compress=False):
    """Read `src` (a path or bytes; "fastq" or "qseq", ".gz" paths inflated on the host as the
    readers do) split by split and write it as `dst_format` to `dst` (a path or a binary stream)
    without the records leaving the device: per split one upload, one decode, one render, then the
    text (or its BGZF members) comes down.  conf carries the readers' and the writers' properties.
    A decode status is raised after the records before it are written.  -> the records written."""
    conf = conf if conf is not None else {}
    probe = object.__new__(_READERS[src_format])
    probe.setConf(conf)
    enc = (_lib.HBAM_QUAL_ILLUMINA if probe.qualityEncoding == BaseQualityEncoding.Illumina
           else _lib.HBAM_QUAL_SANGER)
    ctx = context(conf)
    data = src
    if isinstance(src, (str, os.PathLike)) and _codec(src) == "gz":
        raw = SeekableFile(src)
        data = _gunzip(raw.read_at(0, raw.length))
        raw.close()
        split_size = None
    ss = SeekableFile(data)
    splits = [(0, None)] if not split_size else [(s, min(split_size, ss.length - s))
                                                 for s in range(0, ss.length, split_size)]
    w = _OUTPUTS[dst_format]().getRecordWriter(dst, conf, compress=compress, ctx=ctx)
    total = 0
    try:
        for start, length in splits:
            d, window = _decode_split_device(ctx, src_format, ss, start, length, enc, probe.filterFailedQC)
            try:
                w.write_split(d, window, src_format)
                total += int(d.n)
            finally:
                window.free()
            status = int(d.status)
            if status == _lib.HBAM_EMORE:
                raise RuntimeError("the window reached the end of the file and the decode still asks for more")
            if status != _lib.HBAM_OK:
                msg = "%s at %s:%d" % (_READERS[src_format]._WHAT, src if isinstance(src, (str, os.PathLike)) else
                                       "<bytes>", int(d.err_pos))
                if status == _lib.HBAM_ERUNTIME:
                    raise RuntimeException(msg)
                if status == _lib.HBAM_EUNSUPPORTED:
                    raise SeqUnsupportedException(msg)
                raise_for(status, msg)
    finally:
        ss.close()
        w.close()
    return total
