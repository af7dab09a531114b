"""A line-by-line Python reading of the summarize plugin's reduce side and of SummarySort's reader
(cli/plugins/chipster/Summarize.java, SummarySort.java), stateful as the Java is: the reducer keeps
running sums and counters per group and is fed one key at a time; nothing here is formulated as
prefix differences or scans.  Java's int / long arithmetic is made explicit (_i32, _i64, _ldiv).

The statuses are the library's: -13 IndexOutOfBoundsException, -19 NumberFormatException."""

EINDEX, ENUMBER = -13, -19


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def _i64(x):
    x &= 0xffffffffffffffff
    return x - (1 << 64) if x >> 63 else x


def _ldiv(a, b):
    """Java long division: truncates toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def get_key0(ref_idx, start0):
    """BAMRecordReader.getKey0: (long)refIdx << 32 | alignmentStart0 (the int is sign-extended)."""
    return _i64((ref_idx << 32) | (start0 & 0xffffffffffffffff))


def centre_of_mass(beg, end):
    """Range.getCentreOfMass (:575-577): (int)(((long)beg + end) / 2)"""
    return _i32(_ldiv(beg + end, 2))


def range_key(ref_idx, beg, end):
    """What SummarizeRecordReader.nextKeyValue sets for a record's first range (:714-715)."""
    return get_key0(ref_idx, centre_of_mass(beg, end))


def get_summary_name(lvl, reverse):
    return "summary" + lvl + ("r" if reverse else "f")


class SummaryGroup:
    """Summarize.java:812-828"""

    def __init__(self, lvl, name):
        self.level, self.outName = lvl, name
        self.reset()

    def reset(self):
        self.sumBeg = self.sumEnd = 0
        self.count = 0
        self.span = None  # (not in the Java) positions in the reducer's input stream, for the coverage tests


class RangeCount:
    def __init__(self):
        self.rid = self.beg = self.end = self.count = 0

    def __str__(self):  # :601-606
        return "%d\t%d\t%d\t%d" % (self.rid, self.beg, self.end, self.count)


class SummarizeReducer:
    """Summarize.java:466-561.  outputs[name] = the lines MultipleOutputs receives for that named
    output, in write order; spans[name] = for each line the first and last position (in the
    reducer's input stream) of the ranges it summarizes; sums[name] = its (sumBeg, sumEnd)."""

    def __init__(self):
        self.summaryGroupsR, self.summaryGroupsF = [], []
        self.summary = RangeCount()
        self.currentReferenceID = 0  # :483
        self.outputs, self.spans, self.sums = {}, {}, {}
        self._at = 0

    def setup(self, levels):  # :485-497
        for s in levels:
            lvl = int(s)
            self.summaryGroupsR.append(SummaryGroup(lvl, get_summary_name(s, True)))
            self.summaryGroupsF.append(SummaryGroup(lvl, get_summary_name(s, False)))
        for g in self.summaryGroupsF + self.summaryGroupsR:
            self.outputs[g.outName], self.spans[g.outName], self.sums[g.outName] = [], [], []

    def reduce(self, key, ranges):  # :499-527
        referenceID = _i32((key & 0xffffffffffffffff) >> 32)
        if referenceID != self.currentReferenceID:
            self.currentReferenceID = referenceID
            self.doAllSummaries()
        for beg, end, rev in ranges:
            groups = self.summaryGroupsR if rev else self.summaryGroupsF
            for group in groups:
                group.sumBeg = _i64(group.sumBeg + beg)
                group.sumEnd = _i64(group.sumEnd + end)
                group.span = (group.span[0] if group.span else self._at, self._at)
                group.count += 1
                if group.count == group.level:
                    self.doSummary(group)
            self._at += 1

    def cleanup(self):  # :529-537
        self.doAllSummaries()

    def doAllSummaries(self):  # :539-546
        for group in self.summaryGroupsR:
            if group.count > 0:
                self.doSummary(group)
        for group in self.summaryGroupsF:
            if group.count > 0:
                self.doSummary(group)

    def doSummary(self, group):  # :548-560
        s = self.summary
        s.rid = self.currentReferenceID
        s.beg = _i32(_ldiv(group.sumBeg, group.count))
        s.end = _i32(_ldiv(group.sumEnd, group.count))
        s.count = group.count
        self.outputs[group.outName].append(str(s))
        self.spans[group.outName].append(group.span)
        self.sums[group.outName].append((group.sumBeg, group.sumEnd))
        group.reset()


def shuffle(key, beg, end, rev):
    """The map output through the total-order shuffle into ONE reducer: (key, values) in the order
    of the signed keys, the values of equal keys in input order (the project's tie-break)."""
    order = sorted(range(len(key)), key=lambda i: key[i])  # sorted() is stable
    out = []
    for i in order:
        if out and out[-1][0] == key[i]:
            out[-1][1].append((beg[i], end[i], rev[i]))
        else:
            out.append((key[i], [(beg[i], end[i], rev[i])]))
    return out


def run_reducer(key, beg, end, rev, levels):
    """-> the reducer after setup, every reduce call and cleanup.  levels: the level texts."""
    r = SummarizeReducer()
    r.setup(levels)
    for k, vals in shuffle(key, beg, end, rev):
        r.reduce(k, vals)
    r.cleanup()
    return r


def stream_names(levels):
    """The output streams in (level-major, f then r) order."""
    return [get_summary_name(l, rev) for l in levels for rev in (False, True)]


def stream_text(lines):
    """TextOutputFormat: every value's toString and a newline."""
    return b"".join(l.encode() + b"\n" for l in lines)


# ---- SummarySort ------------------------------------------------------------------------------
def line_reader(data):
    """Hadoop LineReader.readLine over the whole stream: LF, a lone CR and CRLF end a line; a last
    line without a terminator is delivered; readLine returning 0 consumed bytes ends the file (so
    there is no empty last line, but an empty line between terminators is a line)."""
    out, i, n = [], 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] not in (10, 13):
            j += 1
        out.append(bytes(data[i:j]))
        if j < n:
            j += 2 if (data[j] == 13 and j + 1 < n and data[j + 1] == 10) else 1
        i = j
    return out


class _Raise(Exception):
    def __init__(self, status):
        self.status = status


def _text_decode(line, start, length):
    if length < 0 or start + length > len(line):
        raise _Raise(EINDEX)  # Text.decode -> ByteBuffer.wrap: IndexOutOfBoundsException
    return line[start:start + length]


def _parse_int(b):
    """Integer.parseInt: [+-]? digit+ inside int; a byte >= 0x80 is declared NumberFormatException."""
    if any(c >= 0x80 for c in b):
        raise _Raise(ENUMBER)
    body = b[1:] if b[:1] in (b"+", b"-") else b
    if not body or any(not 48 <= c <= 57 for c in body):
        raise _Raise(ENUMBER)
    v = int(b)
    if not -(1 << 31) <= v < (1 << 31):
        raise _Raise(ENUMBER)
    return v


def sort_record_key(line):
    """SortRecordReader.nextKeyValue (SummarySort.java:240-260) after the line is read."""
    tabOne = line.find(b"\t")
    rid = _parse_int(_text_decode(line, 0, tabOne))
    tabTwo = line.find(b"\t", tabOne + 1)
    posBeg = tabOne + 1
    posEnd = tabTwo - 1
    pos = _parse_int(_text_decode(line, posBeg, posEnd - posBeg + 1))
    return get_key0(rid, pos)


def summary_keys(data):
    """-> (lines delivered, their keys, status of the exception after them or 0)"""
    lines, keys = [], []
    for line in line_reader(data):
        try:
            k = sort_record_key(line)
        except _Raise as e:
            return lines, keys, e.status
        lines.append(line)
        keys.append(k)
    return lines, keys, 0


def gathered(lines, keys=None):
    """SortOutputFormat's text: each line and a newline, in file order or (keys) in the shuffle's
    stable key order (SortReducer is the identity)."""
    order = range(len(lines)) if keys is None else sorted(range(len(lines)), key=lambda i: keys[i])
    return b"".join(lines[i] + b"\n" for i in order)


def summary_sort(data):
    lines, keys, status = summary_keys(data)
    assert status == 0, status
    return gathered(lines, keys)
