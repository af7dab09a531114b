"""Host-side mirror of Hadoop-BAM's text read formats over the MI355X C ABI.

FormatConstants (FormatConstants.java), FormatException, SequencedFragment (SequencedFragment.java),
FastqInputFormat / FastqRecordReader (FastqInputFormat.java) and QseqInputFormat / QseqRecordReader
(QseqInputFormat.java): same names, argument meaning, configuration properties and exceptions.  The
lines, the record frames, the identifiers, the QC filter, the quality conversion and the three
pools come from libhbam.so (hbam_fastq.hip, hbam_fastq_decode_split / hbam_qseq_decode_split); this
module reads the window, maps the columns onto the classes and raises what the status says.

A .gz file is not splittable and is inflated here with zlib (one DEFLATE stream has no block
parallelism, the BGZF kernels do not apply); its text goes through the same device call with
start = 0 and an unbounded end.  Other codec extensions raise NotImplementedError.

The output formats (FastqOutputFormat, QseqOutputFormat) are in fastq_text.py, FASTA input in
fasta.py.  Out of scope: SequencedFragment's Writable wire form (readFields / write) and a Java shim
class.  Inputs the device path does not restate raise SeqUnsupportedException (include/hbam.h lists
them under HBAM_EUNSUPPORTED).
"""
import zlib

import numpy as np

from . import _lib
from ._window import read_growing_window
from .formats import (FileSplit, FormatException, IllegalArgumentException,  # noqa: F401
                      NumberFormatException, SeekableFile, context, raise_for)

SEQ_WINDOW_TAIL = 1 << 20  # bytes read past the split's end at first (the last record's tail)


class RuntimeException(RuntimeError):
    """java.lang.RuntimeException as the two readers raise it."""


class SeqUnsupportedException(NotImplementedError):
    """Input the device path does not restate (HBAM_EUNSUPPORTED)."""


class BaseQualityEncoding:
    Illumina = "Illumina"
    Sanger = "Sanger"


class FormatConstants:
    """FormatConstants.java:25-59."""
    SANGER_OFFSET = 33
    SANGER_MAX = 93
    ILLUMINA_OFFSET = 64
    ILLUMINA_MAX = 62
    BaseQualityEncoding = BaseQualityEncoding
    CONF_INPUT_BASE_QUALITY_ENCODING = "hbam.input.base-quality-encoding"
    CONF_INPUT_FILTER_FAILED_QC = "hbam.input.filter-failed-qc"


def parse_boolean(value, default):
    """util/ConfHelper.java:41-64."""
    if value is None:
        return default
    v = str(value).strip().lower()
    if v in ("yes", "true", "t", "y", "1"):
        return True
    if v in ("no", "false", "f", "n", "0"):
        return False
    raise IllegalArgumentException("Unrecognized boolean value '%s'" % value)


def _signed(b):
    return b - 256 if b >= 128 else b


class SequencedFragment:
    """SequencedFragment.java:33-291 without the Writable wire form.  Sequence and quality are bytes
    (the contents of the reference's Text objects); a null field is None."""
    _FIELDS = ("instrument", "runNumber", "flowcellId", "lane", "tile", "xpos", "ypos", "read",
               "filterPassed", "controlNumber", "indexSequence")

    def __init__(self):
        self.clear()

    def clear(self):
        self.sequence, self.quality = b"", b""
        for f in self._FIELDS:
            setattr(self, f, None)

    def getSequence(self):
        return self.sequence

    def getQuality(self):
        return self.quality

    def setSequence(self, seq):
        if seq is None:
            raise IllegalArgumentException("can't have a null sequence")
        self.sequence = bytes(seq)

    def setQuality(self, qual):
        if qual is None:
            raise IllegalArgumentException("can't have a null quality")
        self.quality = bytes(qual)

    def equals(self, other):
        return (isinstance(other, SequencedFragment)
                and all(getattr(self, f) == getattr(other, f) for f in self._FIELDS)
                and self.sequence == other.sequence and self.quality == other.quality)

    __eq__ = equals
    __hash__ = None

    def toString(self):
        def s(v):
            return "null" if v is None else str(v)
        return "\t".join([s(self.instrument), s(self.runNumber), s(self.flowcellId), s(self.lane), s(self.tile),
                          s(self.xpos), s(self.ypos), s(self.indexSequence), s(self.read),
                          self.sequence.decode("utf-8", "replace"), self.quality.decode("utf-8", "replace"),
                          "1" if self.filterPassed is None or self.filterPassed else "0"])

    __str__ = toString

    @staticmethod
    def _range(encoding):
        if encoding == BaseQualityEncoding.Illumina:
            return FormatConstants.ILLUMINA_OFFSET, FormatConstants.ILLUMINA_OFFSET + FormatConstants.ILLUMINA_MAX
        if encoding == BaseQualityEncoding.Sanger:
            return FormatConstants.SANGER_OFFSET, FormatConstants.SANGER_OFFSET + FormatConstants.SANGER_MAX
        raise IllegalArgumentException("Unsupported base encoding quality %s" % encoding)

    @staticmethod
    def verifyQuality(quality, encoding):
        """:263-291 -> the index of the first out-of-range byte, or -1 (bytes are signed, as in Java)."""
        lo, hi = SequencedFragment._range(encoding)
        for i, b in enumerate(bytes(quality)):
            if not lo <= _signed(b) <= hi:
                return i
        return -1

    @staticmethod
    def convertQuality(quality, current, target):
        """:211-250, in place on a bytearray (bytes before an out-of-range one are already rewritten)."""
        if current == target:
            raise IllegalArgumentException("current and target quality encodinds are the same (%s)" % current)
        pair = (current, target)
        if pair not in ((BaseQualityEncoding.Illumina, BaseQualityEncoding.Sanger),
                        (BaseQualityEncoding.Sanger, BaseQualityEncoding.Illumina)):
            raise IllegalArgumentException("unsupported BaseQualityEncoding transformation from %s to %s" % pair)
        lo, hi = SequencedFragment._range(current)
        d = FormatConstants.ILLUMINA_OFFSET - FormatConstants.SANGER_OFFSET
        d = -d if current == BaseQualityEncoding.Illumina else d
        for i in range(len(quality)):
            if not lo <= _signed(quality[i]) <= hi:
                raise FormatException("base quality score out of range for %s format (found %d)"
                                      % (current, _signed(quality[i]) - lo))
            quality[i] = (quality[i] + d) & 0xff


def _accessors(name):
    cap = name[0].upper() + name[1:]
    setattr(SequencedFragment, "get" + cap, lambda self: getattr(self, name))
    setattr(SequencedFragment, "set" + cap, lambda self, v: setattr(self, name, v))


for _n in SequencedFragment._FIELDS:  # getInstrument / setInstrument ... getIndexSequence / setIndexSequence
    _accessors(_n)


_COMPRESSED_EXTS = (".bz2", ".deflate", ".snappy", ".lz4", ".zst", ".lzo", ".lzo_deflate")


def _codec(path):
    """CompressionCodecFactory.getCodec by extension: "gz", None, or NotImplementedError."""
    name = str(path)
    if name.endswith(".gz"):
        return "gz"
    for e in _COMPRESSED_EXTS:
        if name.endswith(e):
            raise NotImplementedError("compression codec %s is not supported: %s" % (e, name))
    return None


def _gunzip(raw):
    out, raw = [], bytes(raw)
    while raw:  # concatenated members, as GzipCodec's stream reads them
        d = zlib.decompressobj(47)
        out.append(d.decompress(raw))
        out.append(d.flush())
        raw = d.unused_data
    return b"".join(out)


def read_split_columns(ctx, fmt, ss, start, length, encoding, filter_failed_qc):
    """The device call over the window of FileSplit [start, start + length): file bytes from the
    reader's first byte (start for FASTQ, start - 1 for QSEQ) to start + length + tail, the tail
    growing x4 from SEQ_WINDOW_TAIL while the call answers HBAM_EMORE (length None: the whole file)
    -> (host columns, window base, window)."""
    def call(window, base):
        cols = ctx.frag_decode_split(fmt, window, start, length, encoding, filter_failed_qc, text_base=base,
                                     file_len=ss.length)
        if cols["rc"]:
            raise_for(cols["rc"], cols.get("error", ""))
        return cols

    base = min(start if fmt == "fastq" else max(start - 1, 0), ss.length)
    cols, window = read_growing_window(ss, base, start, length, SEQ_WINDOW_TAIL, call)
    return cols, base, window


class _SeqRecordReader:
    """What the two readers share: the constructor (:105-133), setConf, the iteration, getPos,
    getProgress (float32 arithmetic) and makePositionMessage."""
    _FMT = None
    _WHAT = None

    def __init__(self, conf=None, split=None, data=None):
        self.conf = conf if conf is not None else {}
        self.setConf(self.conf)
        self.file = split.getPath()
        start, length = split.getStart(), split.getLength()
        src = data if data is not None else self.file
        if _codec(self.file) == "gz":
            if start != 0:
                raise RuntimeException("Start position for compressed file is not 0! (found %d)" % start)
            raw = SeekableFile(src)
            src, length = _gunzip(raw.read_at(0, raw.length)), None  # end = Long.MAX_VALUE
            raw.close()
        ss = SeekableFile(src)
        enc = _lib.HBAM_QUAL_ILLUMINA if self.qualityEncoding == BaseQualityEncoding.Illumina else _lib.HBAM_QUAL_SANGER
        cols, base, window = read_split_columns(context(self.conf), self._FMT, ss, start, length, enc,
                                                self.filterFailedQC)
        ss.close()
        if cols["status"] == _lib.HBAM_EMORE:
            raise RuntimeError("the window reached the end of the file and the decode still asks for more")
        self.cols, self.base, self.window, self.i = cols, base, window, -1
        # positionAtFirstRecord moves start; getProgress uses the moved one
        self.start = self.pos = cols["first_pos"]
        self.end = (1 << 63) - 1 if length is None else start + length
        self.currentKey, self.currentValue = None, SequencedFragment()

    def setConf(self, conf):
        encoding = conf.get(self.CONF_BASE_QUALITY_ENCODING,
                            conf.get(FormatConstants.CONF_INPUT_BASE_QUALITY_ENCODING,
                                     self.CONF_BASE_QUALITY_ENCODING_DEFAULT))
        if encoding == "illumina":
            self.qualityEncoding = BaseQualityEncoding.Illumina
        elif encoding == "sanger":
            self.qualityEncoding = BaseQualityEncoding.Sanger
        else:
            raise RuntimeException("Unknown input base quality encoding value %s" % encoding)
        self.filterFailedQC = parse_boolean(
            conf.get(self.CONF_FILTER_FAILED_QC, conf.get(FormatConstants.CONF_INPUT_FILTER_FAILED_QC)), False)

    def initialize(self, split=None, context=None):
        pass

    def _fail(self):
        c = self.cols
        code, msg = c["status"], "%s at %s:%d" % (self._WHAT, self.file, c["err_pos"])
        if code == _lib.HBAM_ERUNTIME:
            raise RuntimeException(msg)
        if code == _lib.HBAM_EUNSUPPORTED:
            raise SeqUnsupportedException(msg)
        raise_for(code, msg)

    def _str(self, pair):
        o, n = int(pair[0]), int(pair[1])
        return bytes(self.window[o:o + n]).decode("utf-8", "replace")

    def _value(self, i):
        c, v = self.cols, SequencedFragment()
        p = int(c["present"][i])
        P = _lib.FRAG_PRESENT
        v.sequence = c["seq"][int(c["seq_off"][i]):int(c["seq_off"][i + 1])].tobytes()
        v.quality = c["qual"][int(c["qual_off"][i]):int(c["qual_off"][i + 1])].tobytes()
        for col, attr in (("run", "runNumber"), ("lane", "lane"), ("tile", "tile"), ("xpos", "xpos"),
                          ("ypos", "ypos"), ("read", "read"), ("control", "controlNumber")):
            if p & P[col]:
                setattr(v, attr, int(c[col][i]))
        if p & P["filter_passed"]:
            v.filterPassed = bool(c["filter_passed"][i])
        if p & P["instrument"]:
            v.instrument = self._str(c["instrument"][i])
        if p & P["flowcell"]:
            v.flowcellId = self._str(c["flowcell"][i])
        if p & P["index"]:
            v.indexSequence = self._str(c["index"][i])
            if self._FMT == "qseq":
                v.indexSequence = v.indexSequence.replace(".", "N")
        return v

    def next(self, key=None, value=None):
        """next(key, value): True and the record in getCurrentKey / getCurrentValue, False at the
        split's end, or the reference's exception."""
        c = self.cols
        if self.i + 1 < c["n"]:
            self.i += 1
            i = self.i
            self.currentKey = c["key"][int(c["key_off"][i]):int(c["key_off"][i + 1])].tobytes().decode("utf-8", "replace")
            self.currentValue = self._value(i)
            self.pos = int(c["pos_after"][i])
            return True
        self.i = c["n"]
        self.pos = c["end_pos"]
        if c["status"] != _lib.HBAM_OK:
            self._fail()
        return False

    nextKeyValue = next

    def getCurrentKey(self):
        return self.currentKey

    def getCurrentValue(self):
        return self.currentValue

    def createKey(self):
        return ""

    def createValue(self):
        return SequencedFragment()

    def getPos(self):
        return self.pos

    def getProgress(self):
        if self.start == self.end:
            return 1.0
        return float(min(np.float32(1.0), np.float32(self.pos - self.start) / np.float32(self.end - self.start)))

    def makePositionMessage(self, pos=None):
        return "%s:%d" % (self.file, self.pos if pos is None else pos)

    def close(self):
        self.cols = self.window = None


class FastqRecordReader(_SeqRecordReader):
    """FastqInputFormat.FastqRecordReader (FastqInputFormat.java:56-393); key = the read's id (str),
    value = SequencedFragment."""
    _FMT, _WHAT = "fastq", "fastq record"
    CONF_BASE_QUALITY_ENCODING = "hbam.fastq-input.base-quality-encoding"
    CONF_FILTER_FAILED_QC = "hbam.fastq-input.filter-failed-qc"
    CONF_BASE_QUALITY_ENCODING_DEFAULT = "sanger"
    MAX_LINE_LENGTH = 10000


class QseqRecordReader(_SeqRecordReader):
    """QseqInputFormat.QseqRecordReader (QseqInputFormat.java:58-429)."""
    _FMT, _WHAT = "qseq", "qseq line"
    CONF_BASE_QUALITY_ENCODING = "hbam.qseq-input.base-quality-encoding"
    CONF_FILTER_FAILED_QC = "hbam.qseq-input.filter-failed-qc"
    CONF_BASE_QUALITY_ENCODING_DEFAULT = "illumina"
    MAX_LINE_LENGTH = 20000


class _SeqInputFormat:
    _READER = None

    def isSplitable(self, context=None, path=None):
        return _codec(path) is None

    def createRecordReader(self, split, conf=None, data=None):
        return self._READER(conf, split, data=data)


class FastqInputFormat(_SeqInputFormat):
    """FastqInputFormat.java:48-409."""
    CONF_BASE_QUALITY_ENCODING = FastqRecordReader.CONF_BASE_QUALITY_ENCODING
    CONF_FILTER_FAILED_QC = FastqRecordReader.CONF_FILTER_FAILED_QC
    CONF_BASE_QUALITY_ENCODING_DEFAULT = FastqRecordReader.CONF_BASE_QUALITY_ENCODING_DEFAULT
    FastqRecordReader = FastqRecordReader
    _READER = FastqRecordReader


class QseqInputFormat(_SeqInputFormat):
    """QseqInputFormat.java:50-445."""
    CONF_BASE_QUALITY_ENCODING = QseqRecordReader.CONF_BASE_QUALITY_ENCODING
    CONF_FILTER_FAILED_QC = QseqRecordReader.CONF_FILTER_FAILED_QC
    CONF_BASE_QUALITY_ENCODING_DEFAULT = QseqRecordReader.CONF_BASE_QUALITY_ENCODING_DEFAULT
    QseqRecordReader = QseqRecordReader
    _READER = QseqRecordReader
