"""The tests' restatement of the reference's FASTQ and QSEQ readers (host Python, no device).

LineReader is a literal port of LineReader.readLine / skip (LineReader.java:111-230) with its 64 KiB
buffer and its maxBytesToConsume hint, over a stream model in which every read fills the buffer unless
the file ends.  FastqReader and QseqReader are FastqRecordReader (FastqInputFormat.java:105-392) and
QseqRecordReader (QseqInputFormat.java:105-428) run as the sequential state machines they are; their
positioning walks call the two-argument readLine, whose int is maxLineLength (the hint stays
Integer.MAX_VALUE, so no line of a walk is cut).  run_fastq / run_qseq drive one to the end of its
split and return what the device columns hold.

Inputs the device path documents as not restated raise Unsupported at the point the device answers
HBAM_EUNSUPPORTED: an empty line where a FASTQ record should start with data behind it, and a byte
>= 0x80 in a key the Illumina pattern would be run on or in QSEQ fields 0-7.
"""
import random
import re

OK, EUNSUPPORTED, ERUNTIME, ESEQFORMAT, ENUMBER = 0, -9, -15, -18, -19
BUFFER_SIZE = 64 * 1024
INT_MAX = 2 ** 31 - 1
LONG_MAX = 2 ** 63 - 1

# SequencedFragment's *_Present bits
P_INSTRUMENT, P_RUN, P_FLOWCELL, P_LANE, P_TILE, P_XPOS, P_YPOS, P_READ, P_FILTER, P_CONTROL, P_INDEX = (
    1 << i for i in range(11))


class RuntimeException(Exception):
    code = ERUNTIME


class FormatException(RuntimeException):
    code = ESEQFORMAT


class NumberFormatException(Exception):
    code = ENUMBER


class Unsupported(Exception):
    code = EUNSUPPORTED


class EOFException(Exception):
    pass


class Stream:
    """FSDataInputStream over bytes: read(buffer) fills the buffer unless the file ends."""

    def __init__(self, data):
        self.data, self.at = bytes(data), 0

    def seek(self, pos):
        self.at = pos

    def read(self, size):
        chunk = self.data[self.at:self.at + size]
        self.at += len(chunk)
        return chunk if chunk else None  # None: read() returned -1


class Text:
    def __init__(self):
        self.b = bytearray()

    def clear(self):
        self.b = bytearray()


def java_int(v):
    """(int) of a long."""
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


class LineReader:
    def __init__(self, stream, buffer_size=BUFFER_SIZE):
        self.inp, self.bufferSize = stream, buffer_size
        self.buffer, self.bufferLength, self.bufferPosn = b"", 0, 0

    def readLine(self, text, maxLineLength=INT_MAX, maxBytesToConsume=INT_MAX):
        text.clear()
        txtLength = newlineLength = 0
        prevCharCR = False
        bytesConsumed = 0
        while True:
            startPosn = self.bufferPosn
            if self.bufferPosn >= self.bufferLength:
                startPosn = self.bufferPosn = 0
                if prevCharCR:
                    bytesConsumed += 1
                chunk = self.inp.read(self.bufferSize)
                self.buffer = chunk or b""
                self.bufferLength = len(chunk) if chunk is not None else -1
                if self.bufferLength <= 0:
                    break
            buf = self.buffer
            while self.bufferPosn < self.bufferLength:
                if buf[self.bufferPosn] == 0x0a:
                    newlineLength = 2 if prevCharCR else 1
                    self.bufferPosn += 1
                    break
                if prevCharCR:
                    newlineLength = 1
                    break
                prevCharCR = buf[self.bufferPosn] == 0x0d
                self.bufferPosn += 1
            readLength = self.bufferPosn - startPosn
            if prevCharCR and newlineLength == 0:
                readLength -= 1
            bytesConsumed += readLength
            appendLength = readLength - newlineLength
            if appendLength > maxLineLength - txtLength:
                appendLength = maxLineLength - txtLength
            if appendLength > 0:
                text.b += buf[startPosn:startPosn + appendLength]
                txtLength += appendLength
            if not (newlineLength == 0 and bytesConsumed < maxBytesToConsume):
                break
        return bytesConsumed

    def skip(self, n):
        end, toskip = False, n
        while toskip > 0 and not end:
            if self.bufferPosn < self.bufferLength:
                skipped = min(self.bufferLength - self.bufferPosn, toskip)
                self.bufferPosn += skipped
                toskip -= skipped
            if self.bufferPosn >= self.bufferLength:
                chunk = self.inp.read(self.bufferSize)
                self.buffer = chunk or b""
                self.bufferLength = len(self.buffer)
                self.bufferPosn = 0
                end = self.bufferLength == 0
        return n - toskip


def parse_int(b):
    """Integer.parseInt (Java 7 and later: a leading '+' is accepted)."""
    if not re.fullmatch(rb"[+-]?[0-9]+", bytes(b)):
        raise NumberFormatException(bytes(b))
    v = int(bytes(b))
    if not -2 ** 31 <= v <= INT_MAX:
        raise NumberFormatException(bytes(b))
    return v


def new_fragment():
    return {"seq": b"", "qual": b"", "instrument": None, "run": None, "flowcell": None, "lane": None, "tile": None,
            "xpos": None, "ypos": None, "read": None, "filter_passed": None, "control": None, "index": None}


def quality_check(qual, illumina):
    """verifyQuality (sanger) / convertQuality (illumina) on Java's signed bytes -> the Phred+33 bytes."""
    lo, hi = (64, 126) if illumina else (33, 126)
    for b in qual:
        s = b - 256 if b >= 128 else b
        if s < lo or s > hi:
            raise FormatException("base quality score out of range")
    return bytes(b - 31 for b in qual) if illumina else bytes(qual)


def parse_conf(conf, fmt):
    """setConf's lookup order -> (illumina, filter_failed_qc)."""
    default = "sanger" if fmt == "fastq" else "illumina"
    enc = conf.get("hbam.%s-input.base-quality-encoding" % fmt, conf.get("hbam.input.base-quality-encoding", default))
    if enc not in ("illumina", "sanger"):
        raise RuntimeException("Unknown input base quality encoding value %s" % enc)
    f = conf.get("hbam.%s-input.filter-failed-qc" % fmt, conf.get("hbam.input.filter-failed-qc"))
    flt = False
    if f is not None:
        f = f.strip().lower()
        if f in ("yes", "true", "t", "y", "1"):
            flt = True
        elif f not in ("no", "false", "f", "n", "0"):
            raise ValueError(f)
    return enc == "illumina", flt


ILLUMINA_PATTERN = re.compile(rb"([^:]+):([0-9]+):([^:]*):([0-9]+):([0-9]+):(-?[0-9]+):(-?[0-9]+)"
                              rb"[ \t\n\x0b\f\r]+([123]):([YN]):([0-9]+):(.*)")
MAX_FASTQ_LINE = 10000
MAX_QSEQ_LINE = 20000


class FastqReader:
    def __init__(self, data, start, length, illumina=False, filter_qc=False, compressed=False):
        self.data = bytes(data)
        self.start, self.end = start, start + length
        self.illumina, self.filterFailedQC = illumina, filter_qc
        self.buffer = Text()
        self.lookForIlluminaIdentifier = True
        stream = Stream(self.data)
        if not compressed:
            self.positionAtFirstRecord(stream)
        else:
            if start != 0:
                raise RuntimeException("Start position for compressed file is not 0!")
            self.end = LONG_MAX
            self.pos = 0
        self.lineReader = LineReader(stream)
        self.key, self.value = Text(), new_fragment()

    def positionAtFirstRecord(self, stream):
        if self.start > 0:
            stream.seek(self.start)
            reader = LineReader(stream)
            buffer = self.buffer
            while True:
                # readLine(Text, int): the int is maxLineLength
                bytesRead = reader.readLine(buffer, java_int(min(MAX_FASTQ_LINE, self.end - self.start)))
                if bytesRead > 0 and (len(buffer.b) <= 0 or buffer.b[0] != 0x40):
                    self.start += bytesRead
                else:
                    backtrackPosition = self.start + bytesRead
                    bytesRead = reader.readLine(buffer, java_int(min(MAX_FASTQ_LINE, self.end - self.start)))
                    bytesRead = reader.readLine(buffer, java_int(min(MAX_FASTQ_LINE, self.end - self.start)))
                    if bytesRead > 0 and len(buffer.b) > 0 and buffer.b[0] == 0x2b:
                        break
                    self.start = backtrackPosition
                    stream.seek(self.start)
                    reader = LineReader(stream)
                if not bytesRead > 0:
                    break
            stream.seek(self.start)
        self.pos = self.start

    def readLineInto(self, dest):
        bytesRead = self.lineReader.readLine(dest, MAX_FASTQ_LINE)
        if bytesRead <= 0:
            raise EOFException()
        self.pos += bytesRead
        return bytesRead

    def lowLevelFastqRead(self):
        # (not restated by the device: an empty line where a record starts, with data behind it)
        d, p = self.data, self.pos
        if p < len(d) and d[p] in (0x0a, 0x0d):
            term = 2 if d[p:p + 2] == b"\r\n" else 1
            if p + term < len(d):
                raise Unsupported("empty line at a record start")
        skipped = self.lineReader.skip(1)
        self.pos += skipped
        if skipped == 0:
            return False
        self.rec_off = self.pos - 1
        self.readLineInto(self.key)
        self.value = value = new_fragment()
        t = Text()
        self.readLineInto(t)
        value["seq"] = bytes(t.b)
        self.readLineInto(self.buffer)
        if len(self.buffer.b) == 0 or self.buffer.b[0] != 0x2b:
            raise RuntimeException("unexpected fastq line separating sequence and quality")
        t = Text()
        self.readLineInto(t)
        value["qual"] = bytes(t.b)
        self.lookForIlluminaIdentifier = self.lookForIlluminaIdentifier and self.scanIlluminaId(self.key, value)
        if not self.lookForIlluminaIdentifier:
            self.scanNameForReadNumber(self.key, value)
        return True

    def next(self):
        if self.pos >= self.end:
            return False
        try:
            while True:
                gotData = self.lowLevelFastqRead()
                v = self.value
                goodRecord = gotData and (not self.filterFailedQC or v["filter_passed"] is None or v["filter_passed"])
                if not (gotData and not goodRecord):
                    break
            if goodRecord:
                v["qual"] = quality_check(v["qual"], self.illumina)
            return goodRecord
        except EOFException:
            raise RuntimeException("unexpected end of file in fastq record")

    @staticmethod
    def scanNameForReadNumber(name, fragment):
        b = name.b
        if len(b) >= 2:
            last = len(b) - 1
            if b[last - 1] == 0x2f and 0x30 <= b[last] <= 0x39:
                fragment["read"] = b[last] - 0x30

    @staticmethod
    def scanIlluminaId(name, fragment):
        if any(c >= 0x80 for c in name.b):
            raise Unsupported("the pattern runs on the decoded key")
        m = ILLUMINA_PATTERN.fullmatch(bytes(name.b))
        if m:
            fragment["instrument"] = m.group(1)
            fragment["run"] = parse_int(m.group(2))
            fragment["flowcell"] = m.group(3)
            fragment["lane"] = parse_int(m.group(4))
            fragment["tile"] = parse_int(m.group(5))
            fragment["xpos"] = parse_int(m.group(6))
            fragment["ypos"] = parse_int(m.group(7))
            fragment["read"] = parse_int(m.group(8))
            fragment["filter_passed"] = m.group(9) == b"N"
            fragment["control"] = parse_int(m.group(10))
            fragment["index"] = m.group(11)
        return m is not None


class QseqReader:
    def __init__(self, data, start, length, illumina=True, filter_qc=False, compressed=False):
        self.data = bytes(data)
        self.start, self.end = start, start + length
        self.illumina, self.filterFailedQC = illumina, filter_qc
        self.buffer = Text()
        stream = Stream(self.data)
        if not compressed:
            self.positionAtFirstRecord(stream)
        else:
            if start != 0:
                raise RuntimeException("Start position for compressed file is not 0!")
            self.end = LONG_MAX
            self.pos = 0
        self.lineReader = LineReader(stream)
        self.key, self.value = Text(), new_fragment()

    def positionAtFirstRecord(self, stream):
        if self.start > 0:
            self.start -= 1
            stream.seek(self.start)
            reader = LineReader(stream)
            bytesRead = reader.readLine(self.buffer, java_int(min(MAX_QSEQ_LINE, self.end - self.start)))
            self.start += bytesRead
            stream.seek(self.start)
        self.pos = self.start

    def lowLevelQseqRead(self):
        bytesRead = self.lineReader.readLine(self.buffer, MAX_QSEQ_LINE)
        self.rec_off = self.pos
        self.pos += bytesRead
        if bytesRead >= MAX_QSEQ_LINE:
            self.err_pos = self.pos - bytesRead
            raise RuntimeException("found abnormally large line")
        elif bytesRead > 0:
            self.scanQseqLine(self.buffer)
        return bytesRead

    def next(self):
        if self.pos >= self.end:
            return False
        while True:
            bytesRead = self.lowLevelQseqRead()
            v = self.value
            goodRecord = bytesRead > 0 and (not self.filterFailedQC or v["filter_passed"] is None or v["filter_passed"])
            if not (bytesRead > 0 and not goodRecord):
                break
        if goodRecord:
            self.err_pos = self.pos - bytesRead
            v["seq"] = v["seq"].replace(b".", b"N")
            v["qual"] = quality_check(v["qual"], self.illumina)
        return goodRecord

    def scanQseqLine(self, line):
        b = bytes(line.b)
        pos = fieldno = 0
        fp, fl = [0] * 11, [0] * 11
        while pos < len(b) and fieldno < 11:
            endpos = b.find(b"\t", pos)
            if endpos < 0:
                endpos = len(b)
            fp[fieldno], fl[fieldno] = pos, endpos - pos
            pos = endpos + 1
            fieldno += 1
        if fieldno != 11:
            self.err_pos = self.pos - len(b)
            raise FormatException("found %d fields instead of 11" % fieldno)
        if any(c >= 0x80 for c in b[:fp[7] + fl[7]]):
            raise Unsupported("Text.decode of fields 0-7")
        key = bytearray(b[:fp[5] + fl[5]].replace(b"\t", b":"))
        key += b":" + b[fp[7]:fp[7] + fl[7]]
        self.key.b = key
        self.value = f = new_fragment()

        def field(i):
            return b[fp[i]:fp[i] + fl[i]]
        f["instrument"] = field(0)
        f["run"] = parse_int(field(1))
        f["lane"] = parse_int(field(2))
        f["tile"] = parse_int(field(3))
        f["xpos"] = parse_int(field(4))
        f["ypos"] = parse_int(field(5))
        f["read"] = parse_int(field(7))
        f["filter_passed"] = b[fp[10]] != 0x30
        if fl[6] > 0 and b[fp[6]] == 0x30:
            f["index"] = None
        else:
            f["index"] = field(6).replace(b".", b"N")
        f["seq"], f["qual"] = field(8), field(9)


def present_mask(v):
    names = ("instrument", "run", "flowcell", "lane", "tile", "xpos", "ypos", "read", "filter_passed", "control",
             "index")
    return sum(1 << i for i, k in enumerate(names) if v[k] is not None)


def _run(reader):
    """Drive a reader to the end of its split -> first_pos, records (each with key, rec_off,
    pos_after and present), status, err_pos (the position the exception's message carries, None when
    it carries none) and end_pos (getPos() after the last call)."""
    out = {"first_pos": reader.pos, "records": [], "status": OK, "err_pos": None}
    try:
        while reader.next():
            v = dict(reader.value)
            v.update(key=bytes(reader.key.b), rec_off=reader.rec_off, pos_after=reader.pos, present=present_mask(v))
            out["records"].append(v)
    except (RuntimeException, NumberFormatException, Unsupported) as e:
        out["status"] = e.code
        if isinstance(reader, FastqReader):
            if not isinstance(e, (Unsupported, NumberFormatException)):
                out["err_pos"] = reader.pos
        elif isinstance(e, RuntimeException):
            out["err_pos"] = reader.err_pos
    out["end_pos"] = reader.pos
    out["n"] = len(out["records"])
    return out


def run_fastq(data, start, length, illumina=False, filter_qc=False, compressed=False):
    return _run(FastqReader(data, start, length, illumina, filter_qc, compressed))


def run_qseq(data, start, length, illumina=True, filter_qc=False, compressed=False):
    return _run(QseqReader(data, start, length, illumina, filter_qc, compressed))


def file_splits(file_len, split_size):
    """(start, length) of fixed-size splits covering the file, the last one shorter."""
    return [(s, min(split_size, file_len - s)) for s in range(0, file_len, split_size)]


_TERMS = (b"\n", b"\r\n", b"\r")


def generate_fastq(seed=20, records=60, long_at=38, first_plain=44):
    """About 24 KiB of FASTQ: LF, CRLF and lone-CR terminators mixed per line, Illumina names up to
    record `first_plain` and a mix after it, filterPassed Y and N, some qualities that begin with '@'
    or '+', and at `long_at` a record whose sequence is 10001 bytes and whose quality is 300."""
    r = random.Random(seed)
    out = bytearray()
    for k in range(records):
        n = r.randrange(30, 150)
        seq = bytes(r.choice(b"ACGTN") for _ in range(n))
        qual = bytearray(r.randrange(33, 127) for _ in range(n))
        if r.random() < 0.2:
            qual[0] = r.choice(b"@+")
        if k == long_at:
            seq = bytes(r.choice(b"ACGT") for _ in range(10001))
            qual = bytearray(r.randrange(35, 100) for _ in range(300))
        if k < first_plain or r.random() < 0.5:
            name = b"M%d:%d:FC%d:%d:%d:%d:%d %d:%s:%d:%s" % (
                r.randrange(100), r.randrange(1000), r.randrange(10), r.randrange(1, 9), r.randrange(1, 3000),
                r.randrange(-50, 30000), r.randrange(-50, 30000), r.randrange(1, 4), r.choice((b"Y", b"N")),
                r.randrange(0, 40), r.choice((b"ACGTAC", b"", b"NNN")))
        else:
            name = b"read.%d plain" % k + r.choice((b"/1", b"/2", b"", b"/x"))
        plus = b"+" + (name if r.random() < 0.3 else b"")
        for line in (b"@" + name, seq, plus, bytes(qual)):
            out += line + r.choice(_TERMS)
    return bytes(out)


def generate_qseq(seed=21, records=110):
    """About 24 KiB of QSEQ with the same terminator mix, filter 0 / 1, "0", dotted and plain index
    sequences, dots in the bases, and Phred+64 qualities."""
    r = random.Random(seed)
    out = bytearray()
    for k in range(records):
        n = r.randrange(40, 150)
        seq = bytes(r.choice(b"ACGT.") for _ in range(n))
        qual = bytes(r.randrange(64, 127) for _ in range(n))
        fields = [b"M%d" % r.randrange(100), b"%d" % r.randrange(1000), b"%d" % r.randrange(1, 9),
                  b"%d" % r.randrange(1, 3000), r.choice((b"", b"+", b"-")) + b"%d" % r.randrange(1, 30000),
                  b"%d" % r.randrange(1, 30000), r.choice((b"0", b"ATC..G", b"ACGT", b"")),
                  b"%d" % r.randrange(1, 4), seq, qual, r.choice((b"0", b"1"))]
        out += b"\t".join(fields) + r.choice(_TERMS)
    return bytes(out)


# ---- the recorded assertions of the reference's own tests (tests/golden/seqfrag/expected.json) ----
def progress(first_pos, end, pos):
    """getProgress() in float arithmetic; start is where positionAtFirstRecord left it."""
    import numpy as np
    if first_pos == end:
        return 1.0
    return float(min(np.float32(1.0), np.float32(pos - first_pos) / np.float32(end - first_pos)))


def assert_case(case, res, end):
    """One expected.json entry against a run result (run_fastq / run_qseq's form, the strings as
    bytes); end = the reader's end (start + length, Long.MAX_VALUE for a compressed file)."""
    names = {OK: None, ERUNTIME: "RuntimeException", ESEQFORMAT: "FormatException", ENUMBER: "NumberFormatException",
             EUNSUPPORTED: "Unsupported"}
    assert names[res["status"]] == case.get("raises"), (case["test"], res["status"])
    recs = case["records"]
    assert len(res["records"]) >= len(recs), case["test"]
    if "n" in case:
        assert res["n"] == case["n"], case["test"]
    if "first_pos" in case:
        assert res["first_pos"] == case["first_pos"], case["test"]
    for want, got in zip(recs, res["records"]):
        for k, v in want.items():
            g = got[k]
            if isinstance(g, bytes):
                g = g.decode("ascii")
            assert g == v, (case["test"], k, g, v)
    if "progress" in case:
        pos = [res["first_pos"]] + [r["pos_after"] for r in res["records"]]
        for want, p in zip(case["progress"], pos):
            assert abs(progress(res["first_pos"], end, p) - want) <= 0.01, (case["test"], p)
