"""Host-side mirror of Hadoop-BAM's FASTA read format over the MI355X C ABI.

ReferenceFragment (ReferenceFragment.java) and FastaInputFormat / FastaRecordReader
(FastaInputFormat.java): same names, argument meaning and exceptions.  The '>' offsets behind
getSplits, the lines, the positions, the keys and the sequence pool come from libhbam.so
(hbam_fasta.hip, hbam_fasta_sections / hbam_fasta_decode_split); this module reads the windows, maps
the columns onto the classes and raises what the status says.

The sequence of a record is what the reference hands out: Hadoop 1.2.1's Text keeps its backing
array, and scanFastaLine appends the whole array, so a line shorter than an earlier one (or than the
header line) carries that line's tail.  `line_len` in the columns is the line's own length.

A .gz file is not splittable.  Its reader never reads a header line, so indexSequence stays null and
the first next() over a non-empty stream raises NullPointerException: that is answered here, on the
host, without a device call.  Other codec extensions raise NotImplementedError.

Out of scope: ReferenceFragment's Writable wire form (readFields / write) and a Java shim class.  A
header line with a byte >= 0x80 raises SeqUnsupportedException (include/hbam.h).
"""
import numpy as np

from . import _lib
from ._window import read_growing_window
from .fastq import (SEQ_WINDOW_TAIL, RuntimeException, SeqUnsupportedException,  # noqa: F401
                    _codec, _gunzip)
from .formats import (FileSplit, IllegalArgumentException, IOException, SeekableFile, context, raise_for)

SECTION_WINDOW = 64 << 20  # bytes per hbam_fasta_sections call


class ReferenceFragment:
    """ReferenceFragment.java:33-136 without the Writable wire form.  The sequence is bytes (the
    contents of the reference's Text); a null field is None."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.sequence, self.indexSequence, self.position = b"", None, None

    def getSequence(self):
        return self.sequence

    def getPosition(self):
        return self.position

    def getIndexSequence(self):
        return self.indexSequence

    def setPosition(self, pos):
        if pos is None:
            raise IllegalArgumentException("can't have null reference position")
        self.position = int(pos)

    def setIndexSequence(self, v):
        if v is None:
            raise IllegalArgumentException("can't have null index sequence")
        self.indexSequence = v

    def setSequence(self, seq):
        if seq is None:
            raise IllegalArgumentException("can't have a null sequence")
        self.sequence = bytes(seq)

    def toString(self):
        def s(v):
            return "null" if v is None else str(v)
        return "\t".join([s(self.indexSequence), s(self.position), self.sequence.decode("utf-8", "replace")])

    __str__ = toString

    def equals(self, other):
        return (isinstance(other, ReferenceFragment) and self.position == other.position
                and self.indexSequence == other.indexSequence and self.sequence == other.sequence)

    __eq__ = equals
    __hash__ = None


def read_split_columns(ctx, ss, start, length):
    """The device call over the window of FileSplit [start, start + length) of SeekableFile `ss`:
    file bytes from `start` to start + length + tail, the tail growing x4 from SEQ_WINDOW_TAIL while
    the call answers HBAM_EMORE -> (host columns, window base, window)."""
    def call(window, base):
        cols = ctx.fasta_decode_split(window, start, length, text_base=base, file_len=ss.length)
        if cols["rc"]:
            raise_for(cols["rc"], cols.get("error", ""))
        return cols

    base = min(start, ss.length)
    cols, window = read_growing_window(ss, base, start, length, SEQ_WINDOW_TAIL, call)
    return cols, base, window


def read_split_columns_device(ctx, ss, start, length):
    """The same call for a caller that keeps the pools on the device -> (device FastaColumnsC, window
    base, window).  The columns are the context's until its next FASTA decode."""
    def call(window, base):
        rc, d = ctx.fasta_decode_split_device(window, start, length, text_base=base, file_len=ss.length)
        if rc:
            raise_for(rc, ctx.last_error())
        return d

    base = min(start, ss.length)
    d, window = read_growing_window(ss, base, start, length, SEQ_WINDOW_TAIL, call)
    return d, base, window


def _first_line_consumed(text):
    """LineReader.readLine's bytesConsumed for the line at the start of `text`."""
    a = np.frombuffer(text, np.uint8)
    ends = np.flatnonzero((a == 0x0a) | (a == 0x0d))
    if len(ends) == 0:
        return len(text)
    i = int(ends[0])
    return i + 2 if text[i:i + 2] == b"\r\n" else i + 1


class FastaRecordReader:
    """FastaInputFormat.FastaRecordReader (FastaInputFormat.java:146-361); key = the section's
    description and the line's position (str), value = ReferenceFragment."""
    MAX_LINE_LENGTH = 20000

    def __init__(self, conf=None, split=None, data=None):
        self.conf = conf if conf is not None else {}
        self.file = split.getPath()
        start, length = split.getStart(), split.getLength()
        src = data if data is not None else self.file
        self.currentKey, self.currentValue = None, ReferenceFragment()
        self.cols = self.window = self.indexSequence = None
        self.i = -1
        if _codec(self.file) == "gz":
            if start != 0:
                raise RuntimeException("Start position for compressed file is not 0! (found %d)" % start)
            raw = SeekableFile(src)
            self.text = _gunzip(raw.read_at(0, raw.length))
            raw.close()
            # positionAtFirstRecord is not called: no indexSequence, pos = 0, end = Long.MAX_VALUE
            self.start = self.pos = 0
            self.end = (1 << 63) - 1
            return
        ss = SeekableFile(src)
        cols, base, window = read_split_columns(context(self.conf), ss, start, length)
        ss.close()
        self.text = None
        if cols["status"] == _lib.HBAM_EMORE:
            raise RuntimeError("the window reached the end of the file and the decode still asks for more")
        if cols["status"] == _lib.HBAM_EINDEX:  # substring(1, 0) of an empty header line
            raise IndexError("String index out of range: -1 (empty header line at %s:%d)" % (self.file, start))
        if cols["status"] == _lib.HBAM_EUNSUPPORTED:
            raise SeqUnsupportedException("header line with a byte >= 0x80 at %s:%d" % (self.file, start))
        self.cols, self.base, self.window = cols, base, window
        o, n = cols["index_off"], cols["index_len"]
        self.indexSequence = bytes(window[o:o + n]).decode("ascii")
        # positionAtFirstRecord moves start; getProgress uses the moved one
        self.start = self.pos = cols["first_pos"]
        self.end = start + length

    def initialize(self, split=None, context=None):
        pass

    def _next_compressed(self):
        at = self.pos
        if at >= len(self.text):
            return False  # readLine returns 0: the end of the stream
        consumed = _first_line_consumed(self.text[at:])
        self.pos += consumed
        if consumed >= self.MAX_LINE_LENGTH:
            raise RuntimeException("found abnormally large line (length %d) at %s"
                                   % (consumed, self.makePositionMessage(at)))
        raise_for(_lib.HBAM_ENULL, "no index sequence was read for a compressed file: %s" % self.makePositionMessage(at))

    def next(self, key=None, value=None):
        """next(key, value): True and the record in getCurrentKey / getCurrentValue, False at the
        split's end, or the reference's exception."""
        if self.text is not None:
            return self._next_compressed()
        c = self.cols
        if self.i + 1 < c["n"]:
            self.i += 1
            i = self.i
            self.currentKey = c["key"][int(c["key_off"][i]):int(c["key_off"][i + 1])].tobytes().decode("ascii")
            v = ReferenceFragment()
            v.position = int(c["position"][i])
            v.indexSequence = self.indexSequence
            v.sequence = c["seq"][int(c["seq_off"][i]):int(c["seq_off"][i + 1])].tobytes()
            self.currentValue = v
            self.pos = int(c["pos_after"][i])
            return True
        self.i = c["n"]
        self.pos = c["end_pos"]
        if c["status"] == _lib.HBAM_ERUNTIME:
            raise RuntimeException("found abnormally large line at %s" % self.makePositionMessage(c["err_pos"]))
        if c["status"] != _lib.HBAM_OK:
            raise_for(c["status"], self.makePositionMessage(c["err_pos"]))
        return False

    nextKeyValue = next

    def getCurrentKey(self):
        return self.currentKey

    def getCurrentValue(self):
        return self.currentValue

    def createKey(self):
        return ""

    def createValue(self):
        return ReferenceFragment()

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


class FastaInputFormat:
    """FastaInputFormat.java:56-377."""
    FastaRecordReader = FastaRecordReader

    def getSplits(self, inputs, conf=None, data=None):
        """:59-144.  inputs = a path, FileSplits, or a list of either (paths stand for the FileSplits
        FileInputFormat makes of them); data = the file's bytes when the path is only a name.  One
        split per section, a section starting at every '>' below the end of the last input split."""
        if isinstance(inputs, (str, bytes, FileSplit)) or hasattr(inputs, "__fspath__"):
            inputs = [inputs]
        src = lambda p: data if data is not None else p  # noqa: E731
        splits = []
        for x in inputs:
            if isinstance(x, FileSplit):
                splits.append(x)
            else:
                ss = SeekableFile(src(x))
                splits.append(FileSplit(x, 0, ss.length))
                ss.close()
        if not splits:
            raise IndexError("no input")
        splits.sort(key=lambda s: str(s.getPath()))
        if any(str(s.getPath()) != str(splits[0].getPath()) for s in splits):
            raise IOException("FastaInputFormat assumes single FASTA input file!")
        path, hosts = splits[0].getPath(), splits[-1].getLocations()
        ss = SeekableFile(src(path))
        scanned = 0
        for s in splits:
            scanned = max(scanned, min(ss.length, s.getStart() + s.getLength()))
        ctx = context(conf)
        found = []
        for base in range(0, scanned, SECTION_WINDOW):
            res = ctx.fasta_sections(ss.read_at(base, min(SECTION_WINDOW, scanned - base)), text_base=base)
            if res["rc"]:
                raise_for(res["rc"], res.get("error", ""))
            found.append(res["offsets"])
        ss.close()
        p = [int(x) for x in np.concatenate(found)] if found else []
        out = [FileSplit(path, a, b - 1 - a, hosts) for a, b in zip(p, p[1:])]
        last = p[-1] if p else 0
        out.append(FileSplit(path, last, scanned - last, hosts))
        return out

    def isSplitable(self, context=None, path=None):
        return _codec(path) is None

    def createRecordReader(self, split, conf=None, data=None):
        return FastaRecordReader(conf, split, data=data)
