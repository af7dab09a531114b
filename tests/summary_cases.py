"""Crafted inputs with declared outcomes for the summarize reduce (hbam_summarize_reduce) and for
SummarySort's reader and writer (hbam_summary_keys, hbam_summary_gather_lines).

A reducer case is the map output of a job — ranges (ref, beg, end, reverse) in input order, keyed as
SummarizeRecordReader keys a record's first range — plus the level texts; `want` holds hand-written
lines per output stream for the unsorted run, `want_sorted` for the --sort run, where the case is
small enough to do by hand.  The expected bytes of every case come from tests/summary_ref.py.

Worth knowing when reading the hand-written lines: SummarizeReducer.reduce sets
currentReferenceID to the new reference BEFORE it flushes (Summarize.java:508-511), so a trailing
partial group flushed at a segment change is written with the rid of the segment that follows."""
import numpy as np

import summary_ref as R

INT_MAX, INT_MIN = 2147483647, -2147483648


class ReducerCase:
    def __init__(self, name, ranges, levels, want=None, want_sorted=None, keys=None):
        self.name, self.levels, self.want, self.want_sorted = name, levels, want, want_sorted
        self.ref = [r[0] for r in ranges]
        self.beg = [r[1] for r in ranges]
        self.end = [r[2] for r in ranges]
        self.rev = [1 if r[3] else 0 for r in ranges]
        self.key = keys if keys is not None else [R.range_key(r[0], r[1], r[2]) for r in ranges]

    def arrays(self):
        return (np.asarray(self.key, np.int64), np.asarray(self.beg, np.int32), np.asarray(self.end, np.int32),
                np.asarray(self.rev, np.uint8))

    def level_values(self):
        return [int(l) for l in self.levels]

    def __repr__(self):
        return self.name


F, Rv = False, True

_READ = {}


def reading(case):
    """The reducer's reading of a case (tests/summary_ref.py), computed once per session and shared
    by every test that needs it."""
    if case.name not in _READ:
        _READ[case.name] = R.run_reducer(case.key, case.beg, case.end, case.rev, case.levels)
    return _READ[case.name]


def _random_case(n, seed):
    """n ranges over references 0..3 in shuffled order; about 1 in 40 has a negative centre (the
    rid = -1 segment), centres repeat (equal keys), and both strands are interleaved."""
    rng = np.random.RandomState(seed)
    ref = rng.randint(0, 4, n)
    beg = rng.randint(1, 3000, n)
    length = rng.randint(1, 200, n)
    neg = rng.randint(0, 40, n) == 0
    beg = np.where(neg, -beg - 400, beg)
    rev = rng.randint(0, 2, n)
    ranges = [(int(ref[i]), int(beg[i]), int(beg[i] + length[i]), bool(rev[i])) for i in range(n)]
    return ReducerCase("random_n%d" % n, ranges, ["1", "2", "3", "64", "100000"])


REDUCER_CASES = [
    # one segment (refID 0 first: the reducer's initial currentReferenceID), forward strand only, input
    # not in key order.  L = 1; L = 2 divides the segment exactly (no partial line); L = 100 and
    # L = 2^31-1 are larger than the segment
    ReducerCase("level_sizes", [(0, 50, 60, F), (0, 10, 20, F), (0, 70, 80, F), (0, 30, 40, F)],
                ["1", "2", "100", "2147483647"],
                want={"summary1f": ["0\t10\t20\t1", "0\t30\t40\t1", "0\t50\t60\t1", "0\t70\t80\t1"],
                      "summary1r": [],
                      "summary2f": ["0\t20\t30\t2", "0\t60\t70\t2"], "summary2r": [],
                      "summary100f": ["0\t40\t50\t4"], "summary100r": [],
                      "summary2147483647f": ["0\t40\t50\t4"], "summary2147483647r": []}),
    # strands interleaved in key order: the partition decides which ranges share a group
    ReducerCase("strands_interleaved", [(1, 1, 2, F), (1, 3, 4, Rv), (1, 5, 6, F), (1, 7, 8, Rv), (1, 9, 10, F)],
                ["2"],
                want={"summary2f": ["1\t3\t4\t2", "1\t9\t10\t1"], "summary2r": ["1\t5\t6\t2"]}),
    # three segments: the rid = -1 segment of a negative centre (whatever the record's refID), then
    # references 0 and 1.  Segments -1 and 1 have one strand only.  Partial groups flushed at a segment
    # change carry the next segment's rid
    ReducerCase("three_segments", [(0, 100, 110, F), (1, 5, 15, F), (2, -10, -4, F), (0, 300, 310, Rv),
                                   (0, 200, 210, F)],
                ["2"],
                want={"summary2f": ["0\t-10\t-4\t1", "0\t150\t160\t2", "1\t5\t15\t1"],
                      "summary2r": ["1\t300\t310\t1"]},
                want_sorted={"summary2f": ["0\t-10\t-4\t1", "0\t150\t160\t2", "1\t5\t15\t1"],
                             "summary2r": ["1\t300\t310\t1"]}),
    # equal keys (all centres 15) straddling a group boundary: input order decides; one of them on the
    # other strand
    ReducerCase("equal_keys", [(0, 10, 20, F), (0, 12, 18, F), (0, 11, 19, Rv), (0, 14, 16, F)], ["2"],
                want={"summary2f": ["0\t11\t19\t2", "0\t14\t16\t1"], "summary2r": ["0\t11\t19\t1"]}),
    # sums needing more than 32 bits
    ReducerCase("big_sums", [(0, INT_MAX, INT_MAX, F)] * 3, ["3", "2"],
                want={"summary3f": ["0\t2147483647\t2147483647\t3"], "summary3r": [],
                      "summary2f": ["0\t2147483647\t2147483647\t2", "0\t2147483647\t2147483647\t1"],
                      "summary2r": []}),
    # negative sums truncate toward zero: sumBeg = -9 -> -4, sumEnd = -7 -> -3 (floor would give -5, -4)
    ReducerCase("negative_truncation", [(0, -5, -3, Rv), (0, -4, -4, Rv)], ["2"],
                want={"summary2f": [], "summary2r": ["-1\t-4\t-3\t2"]}),
    # every rendered width: -2147483648, -1, 0, 9, 10, 2147483647
    ReducerCase("rendered_values", [(0, INT_MIN, -1, F), (0, 0, 9, F), (0, 10, INT_MAX, F)], ["1"],
                want={"summary1f": ["-1\t-2147483648\t-1\t1", "0\t0\t9\t1", "0\t10\t2147483647\t1"],
                      "summary1r": []}),
    # --sort: beg order differs from the emission (centre of mass) order, and a negative beg sorts
    # first through getKey0's sign extension
    ReducerCase("sort_differs", [(0, 100, 300, F), (0, 150, 160, F), (0, -20, 500, F), (1, 7, 9, F), (1, 2, 30, F)],
                ["1"],
                want={"summary1f": ["0\t150\t160\t1", "0\t100\t300\t1", "0\t-20\t500\t1", "1\t7\t9\t1",
                                    "1\t2\t30\t1"],
                      "summary1r": []},
                want_sorted={"summary1f": ["0\t-20\t500\t1", "0\t100\t300\t1", "0\t150\t160\t1", "1\t2\t30\t1",
                                           "1\t7\t9\t1"],
                             "summary1r": []}),
    # the first reference is not the reducer's initial currentReferenceID: the flush it triggers is empty
    ReducerCase("first_ref_nonzero", [(3, 10, 20, F), (3, 30, 40, Rv), (5, 1, 1, Rv)], ["1", "5"],
                want={"summary1f": ["3\t10\t20\t1"], "summary1r": ["3\t30\t40\t1", "5\t1\t1\t1"],
                      "summary5f": ["5\t10\t20\t1"], "summary5r": ["5\t30\t40\t1", "5\t1\t1\t1"]}),
] + [_random_case(n, 100 + n) for n in (0, 1, 63, 64, 65, 255, 256, 257, 70001)]


# ---- summary lines ----------------------------------------------------------------------------
class LineCase:
    def __init__(self, name, data, n, status, keys=None):
        self.name, self.data, self.n, self.status, self.keys = name, data, n, status, keys

    def __repr__(self):
        return self.name


def _k(rid, pos):
    return R.get_key0(rid, pos)


def _line(rid, pos, pad=0):
    """A summary line without its terminator; `pad` extra bytes in the last field (never parsed)."""
    return b"%d\t%d\t%d\t1%s" % (rid, pos, pos + 1, b"0" * pad)


def _edges():
    """Terminators at the edges of the structural pass: an LF as the last byte of a 16-byte quad, a
    CRLF straddling a quad (CR at 31, LF at 32), a lone CR as a quad's last byte, then a CRLF
    straddling the 1 KiB wave step, the 4 KiB tile and a lone CR / LF at the next tile's edge."""
    out = b""

    def upto(target, term):  # a line whose terminator's first byte lands at offset `target`
        nonlocal out
        base = _line(7, len(out))
        out += base + b"0" * (target - len(out) - len(base)) + term
    upto(15, b"\n")
    upto(31, b"\r\n")
    upto(47, b"\r")
    upto(1023, b"\r\n")
    for _ in range(60):
        out += _line(7, len(out)) + b"\n"
    upto(4095, b"\r\n")
    upto(8191, b"\r")
    upto(12287, b"\n")
    out += _line(7, len(out))  # no final terminator
    return out


def _late_error():
    """A clean prefix of 1100 lines (several workgroups of the per-line pass), then the first error
    (a line with one tab: IndexOutOfBounds), clean lines, and a second, different error."""
    lines = [_line(i % 3, 5000 - i) for i in range(1100)] + [b"1\t5"] + [_line(1, i) for i in range(300)]
    lines += [b"x\t1\t2\t1"] + [_line(2, 3)]
    return b"\n".join(lines) + b"\n"


LINE_CASES = [
    LineCase("empty_file", b"", 0, 0, []),
    LineCase("lf", b"0\t5\t9\t1\n1\t7\t8\t2\n", 2, 0, [_k(0, 5), _k(1, 7)]),
    LineCase("mixed_terminators", b"0\t9\t2\t1\r\n0\t3\t4\t1\r0\t5\t6\t1\n0\t1\t1\t1\r\n", 4, 0,
             [_k(0, 9), _k(0, 3), _k(0, 5), _k(0, 1)]),
    LineCase("no_final_terminator", b"2\t9\t9\t1\n2\t10\t11\t1", 2, 0, [_k(2, 9), _k(2, 10)]),
    LineCase("final_cr", b"2\t9\t9\t1\r", 1, 0, [_k(2, 9)]),
    LineCase("plus_and_minus_zero", b"+5\t-0\t1\t1\n-1\t+7\t1\t1\n", 2, 0, [_k(5, 0), _k(-1, 7)]),
    LineCase("ten_and_eleven_chars", b"2147483647\t-2147483648\t0\t1\n-2147483648\t2147483647\t0\t1\n", 2, 0,
             [_k(INT_MAX, INT_MIN), _k(INT_MIN, INT_MAX)]),
    LineCase("negative_pos_sorts_first", b"1\t5\t6\t1\n1\t-3\t6\t1\n0\t9\t9\t1\n", 3, 0,
             [_k(1, 5), _k(1, -3), _k(0, 9)]),
    LineCase("ten_digits_overflow", b"0\t1\t1\t1\n2147483648\t1\t1\t1\n", 1, R.ENUMBER),
    LineCase("eleven_digits", b"0\t12345678901\t1\t1\n", 0, R.ENUMBER),
    LineCase("twenty_digits", b"0\t18446744073709551617\t1\t1\n", 0, R.ENUMBER),
    LineCase("edges", _edges(), None, 0),
    LineCase("empty_rid", b"\t5\t1\t1\n", 0, R.ENUMBER),
    LineCase("empty_pos", b"0\t1\t1\t1\n3\t\t1\n", 1, R.ENUMBER),
    LineCase("one_tab", b"3\t5\n", 0, R.EINDEX),
    LineCase("one_tab_bad_rid", b"x\t5\n", 0, R.ENUMBER),  # rid is parsed before the second tab is looked for
    LineCase("no_tab", b"0\t1\t1\t1\n35\n", 1, R.EINDEX),
    LineCase("empty_line", b"0\t1\t1\t1\n\n0\t2\t2\t1\n", 1, R.EINDEX),
    LineCase("only_newline", b"\n", 0, R.EINDEX),
    LineCase("non_digit", b"0\t1x\t2\t1\n", 0, R.ENUMBER),
    LineCase("sign_only", b"0\t-\t2\t1\n", 0, R.ENUMBER),
    LineCase("high_byte", b"0\t1\t1\t1\n0\t\xc3\xa9\t2\t1\n", 1, R.ENUMBER),
    LineCase("high_byte_rid", b"\xff\t1\t2\t1\n", 0, R.ENUMBER),
    LineCase("late_error", _late_error(), 1100, R.EINDEX),
]
