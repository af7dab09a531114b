"""The tests' restatement of the reference's FASTA reader (host Python, no device).

get_splits is FastaInputFormat.getSplits' byte loop (FastaInputFormat.java:96-143); FastaReader is
FastaRecordReader's constructor, positionAtFirstRecord, next and scanFastaLine (:173-232, :322-360)
run as the sequential state machine it is, over seqfrag_ref's LineReader and Stream.  BackedText is
Hadoop 1.2.1's Text as far as the reader uses it: clear() only zeroes the length, append() grows the
backing array to exactly the needed size when it is too small and keeps the current length, and
getBytes() is that array, whose length scanFastaLine appends.  (Restated from upstream knowledge of
Text.java; unpinned, as DESIGN.md says.)

tail_rule is the closed form of what that gives, the rule the device implements; the tests show the
two agree.  run_fasta drives a reader to the end of its split and returns what the device columns
hold.
"""
from seqfrag_ref import (BUFFER_SIZE, ERUNTIME, EUNSUPPORTED, LONG_MAX, OK, LineReader,  # noqa: F401
                         RuntimeException, Stream, Unsupported, java_int)

EMORE, EINDEX, ENULL = -12, -13, -16
MAX_LINE_LENGTH = 20000


class StringIndexOutOfBoundsException(Exception):
    code = EINDEX


class NullPointerException(Exception):
    code = ENULL


class _Appender:
    """`text.b += chunk`, the way seqfrag_ref.LineReader appends, as Text.append."""

    def __init__(self, text):
        self.text = text

    def __iadd__(self, chunk):
        self.text.append(chunk, 0, len(chunk))
        return self


class BackedText:
    """org.apache.hadoop.io.Text (1.2.1): bytes, length, clear, append, setCapacity."""

    def __init__(self):
        self.bytes, self.length = bytearray(), 0

    def clear(self):
        self.length = 0

    def setCapacity(self, length, keepData):
        if len(self.bytes) < length:
            newBytes = bytearray(length)
            if keepData:
                newBytes[:self.length] = self.bytes[:self.length]
            self.bytes = newBytes

    def append(self, utf8, start, length):
        self.setCapacity(self.length + length, True)
        self.bytes[self.length:self.length + length] = utf8[start:start + length]
        self.length += length

    def getBytes(self):
        return self.bytes

    def getLength(self):
        return self.length

    b = property(lambda self: _Appender(self), lambda self, v: None)


def get_splits(data, orig=None):
    """getSplits' loop over the FileInputFormat splits `orig` of one file ((start, length) pairs,
    default one split over the whole file) -> (start, length) pairs."""
    data = bytes(data)
    orig = [(0, len(data))] if orig is None else list(orig)
    new, byte_counter, prev, first_chromosome = [], 0, 0, True
    for j, (s, n) in enumerate(orig):
        while byte_counter < s + n:
            buf = data[byte_counter:byte_counter + min(1024, s + n - byte_counter)]
            if not buf:
                break  # (a split past the end of the file: the reference would read forever)
            for i, b in enumerate(buf):
                if b == 0x3e:
                    if not first_chromosome:
                        new.append((prev, byte_counter + i - 1 - prev))
                    first_chromosome = False
                    prev = byte_counter + i
            byte_counter += len(buf)
        if j == len(orig) - 1:
            new.append((prev, byte_counter - prev))
            break
    return new


class FastaReader:
    def __init__(self, data, start, length, compressed=False, buffer_size=BUFFER_SIZE):
        self.data = bytes(data)
        self.start, self.end = start, start + length
        self.buffer_size = buffer_size
        self.current_split_pos = 1
        self.current_split_indexseq = None
        self.buffer = BackedText()
        self.pos = 0
        stream = Stream(self.data)
        if not compressed:
            self.positionAtFirstRecord(stream)
        else:
            if start != 0:
                raise RuntimeException("Start position for compressed file is not 0!")
            self.end = LONG_MAX
        self.lineReader = LineReader(stream, buffer_size)
        self.key, self.value = None, None

    def positionAtFirstRecord(self, stream):
        if self.start > 0:
            stream.seek(self.start)
        reader = LineReader(stream, self.buffer_size)
        # readLine(Text, int): the int is maxLineLength
        bytesRead = reader.readLine(self.buffer, java_int(min(MAX_LINE_LENGTH, self.end - self.start)))
        stored = bytes(self.buffer.getBytes()[:self.buffer.getLength()])
        if any(c >= 0x80 for c in stored):
            raise Unsupported("Text.toString / String.getBytes of the header line")
        if len(stored) < 1:
            raise StringIndexOutOfBoundsException("substring(1, 0)")
        self.current_split_indexseq = stored[1:]
        self.current_split_pos = 1
        self.start = self.start + bytesRead
        stream.seek(self.start)
        self.pos = self.start

    def next(self):
        if self.pos >= self.end:
            return False
        self.rec_off = self.pos
        bytesRead = self.lineReader.readLine(self.buffer, MAX_LINE_LENGTH)
        self.pos += bytesRead
        if bytesRead >= MAX_LINE_LENGTH:
            self.err_pos = self.pos - bytesRead
            raise RuntimeException("found abnormally large line")
        elif bytesRead <= 0:
            return False
        else:
            self.scanFastaLine(self.buffer)
            self.current_split_pos = java_int(self.current_split_pos + bytesRead)
            return True

    def scanFastaLine(self, line):
        if self.current_split_indexseq is None:
            raise NullPointerException("current_split_indexseq")
        key = bytearray(self.current_split_indexseq)
        key += str(self.current_split_pos).encode()
        for i in range(len(key)):
            if key[i] == 0x09:
                key[i] = 0x3a
        self.key = bytes(key)
        # fragment.getSequence().append(line.getBytes(), 0, line.getBytes().length)
        self.value = {"position": self.current_split_pos, "index": self.current_split_indexseq,
                      "seq": bytes(line.getBytes()), "line_len": line.getLength()}


def run_fasta(data, start, length, compressed=False, buffer_size=BUFFER_SIZE):
    """Drive a reader to the end of its split -> n, status, first_pos, index (the indexSequence
    bytes), records (key, seq, position, line_len, rec_off, pos_after), err_pos and end_pos.  An
    exception out of the constructor gives n = 0 and first_pos = start."""
    out = {"first_pos": start, "records": [], "status": OK, "err_pos": None, "index": None, "end_pos": start, "n": 0}
    try:
        reader = FastaReader(data, start, length, compressed, buffer_size)
    except (StringIndexOutOfBoundsException, Unsupported) as e:
        out["status"] = e.code
        return out
    out["first_pos"], out["index"] = reader.pos, reader.current_split_indexseq
    try:
        while reader.next():
            v = dict(reader.value)
            v.update(key=reader.key, rec_off=reader.rec_off, pos_after=reader.pos)
            out["records"].append(v)
    except RuntimeException as e:
        out["status"], out["err_pos"] = e.code, reader.err_pos
    except NullPointerException as e:
        out["status"] = e.code
    out["end_pos"] = reader.pos
    out["n"] = len(out["records"])
    return out


def tail_rule(lines):
    """The closed form of the stale tail.  lines[0] = the stored header line ('>' included, line -1),
    lines[1:] = the stored data lines -> the sequence of every data line: cap_k = max(L_-1 .. L_k)
    bytes, byte c the line's own for c < L_k, else byte c of the latest earlier line longer than c."""
    # `longer` = the earlier lines that are longer than every line after them, oldest (and longest)
    # first: the latest earlier line longer than c is the last of them that is longer than c
    out, longer = [], [0]
    for k in range(1, len(lines)):
        seq = bytearray(lines[k])
        for j in reversed(longer):
            if len(lines[j]) > len(seq):
                seq += lines[j][len(seq):]
        assert len(seq) == max(len(x) for x in (lines[longer[0]], lines[k]))  # cap_k
        out.append(bytes(seq))
        while longer and len(lines[longer[-1]]) <= len(lines[k]):
            longer.pop()
        longer.append(k)
    return out
