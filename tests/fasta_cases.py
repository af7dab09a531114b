"""Crafted FASTA inputs shared by tests/test_fasta.py (the restatement alone) and
tests/test_fasta_gpu.py (the device against the restatement).  Every file is a few hundred bytes to a
few hundred KiB.  A case is (id, file bytes, start, length); length None = to the end of the file."""

# the hand-derived fixture: 34 bytes, '>' at 0 and 23
FIXTURE = b">chr1 desc\tx\nACGTAC\nGG\n>c2\nTTTT\r\nA"
FIXTURE_SPLITS = [(0, 22), (23, 11)]
FIXTURE_EXPECTED = {
    (0, 22): {"first_pos": 13, "end_pos": 23, "index": b"chr1 desc\tx",
              "records": [(b"chr1 desc:x1", 1, b"ACGTACdesc\tx"), (b"chr1 desc:x8", 8, b"GGGTACdesc\tx")]},
    (23, 11): {"first_pos": 27, "end_pos": 34, "index": b"c2",
               "records": [(b"c21", 1, b"TTTT"), (b"c27", 7, b"ATTT")]},
    (0, 34): {"first_pos": 13, "end_pos": 34, "index": b"chr1 desc\tx",
              "records": [(b"chr1 desc:x1", 1, b"ACGTACdesc\tx"), (b"chr1 desc:x8", 8, b"GGGTACdesc\tx"),
                          (b"chr1 desc:x11", 11, b">c2TACdesc\tx"), (b"chr1 desc:x15", 15, b"TTTTACdesc\tx"),
                          (b"chr1 desc:x21", 21, b"ATTTACdesc\tx")],
              "line_len": [6, 2, 3, 4, 1]},
}


def line_bytes(k, n):
    """n bytes that tell line k and the column apart (no '\\n', '\\r', '>' or byte >= 0x80)."""
    return bytes(63 + (k * 7 + c * 3) % 60 for c in range(n))


def profile(header_len, lens, term=b"\n"):
    """A one-section file: a header line of header_len bytes ('>' included), then lines of `lens`."""
    out = bytearray(b">" + line_bytes(-1, header_len - 1) + term)
    for k, n in enumerate(lens):
        out += line_bytes(k, n) + term
    return bytes(out)


def _boundary(at):
    """4300 two-byte lines; the lines at the indices `at` are longer, each shorter than the one before."""
    lens = [2] * 4300
    for rank, i in enumerate(sorted(at)):
        lens[i] = 30 - 5 * rank
    return profile(3, lens)


def _sawtooth():
    return profile(4, [(k * 7) % 23 for k in range(200)])


CASES = [
    # ---- terminators
    ("lf", b">h\nACGT\nAC\n", 0, None),
    ("cr", b">h\rACGT\rAC\r", 0, None),
    ("crlf", b">h\r\nACGT\r\nAC\r\n", 0, None),
    ("mixed", b">h d\r\nACGT\rAC\n\nGGGTTT\r\n\r\nA\r", 0, None),
    ("cr-cr-at-the-end", b">h\nACGT\r\r", 0, None),
    ("empty-lines", b">h\n\n\nAC\n\n", 0, None),
    ("no-final-terminator", b">h\nACGT\nAC", 0, None),
    ("header-only", b">h", 0, None),
    ("header-only-lf", b">h\n", 0, None),
    # ---- header
    ("header-stored-0-empty-line", b">h\n\nAC\n", 3, 4),
    ("header-stored-0-length-0", b">h\nAC\n", 0, 0),
    ("header-stored-0-end-of-file", b">h\nAC\n", 6, 5),
    ("header-stored-1", b">\nACGT\nAC\n", 0, None),
    ("header-stored-2", b">x\nACGT\nA\n", 0, None),
    ("header-not-gt", b"ACGT\nAC\nG\n", 1, None),
    ("header-tabs", b">a\tb\t\tc\nACGT\n\tA\n", 0, None),
    ("header-cut-by-the-split", b">chr1 long description\nACGT\nAC\n", 0, 5),
    ("split-ends-behind-the-header", b">chr1 long description\rACGT\nAC\n", 0, 24),
    ("header-20500", b">" + b"h" * 20500 + b"\nACGT\nAC\n", 0, None),
    ("header-byte-0x80", b">caf\xc3\xa9\nAC\n", 0, None),
    ("header-byte-0x80-behind-the-cut", b">abc\xff\nAC\n", 0, 4),
    ("gt-inside-the-header", b">a >b c\nACGT\n>z\nTT\n", 3, 9),
    # ---- line-length profiles for the tail rule
    ("all-equal", profile(5, [10] * 70), 0, None),
    ("decreasing", profile(3, list(range(40, 0, -1))), 0, None),
    ("increasing", profile(3, list(range(1, 41))), 0, None),
    ("sawtooth", _sawtooth(), 0, None),
    ("sawtooth-crlf", profile(4, [(k * 5) % 19 for k in range(150)], b"\r\n"), 0, None),
    ("header-longest", profile(50, [(k * 11) % 31 for k in range(150)]), 0, None),
    ("long-line-then-4200-short", profile(3, [300] + [1 + k % 3 for k in range(4200)]), 0, None),
    ("short-then-long-at-4100", profile(3, [1 + k % 3 for k in range(4100)] + [200, 1, 2, 3]), 0, None),
    ("cover-at-63-64-4095-4096", _boundary((63, 64, 4095, 4096)), 0, None),
    ("cover-at-63", _boundary((63,)), 0, None),
    ("cover-at-64", _boundary((64,)), 0, None),
    ("cover-at-4095", _boundary((4095,)), 0, None),
    ("cover-at-4096", _boundary((4096,)), 0, None),
    # ---- length limit
    ("line-consumes-19999", b">h\nAC\n" + b"A" * 19998 + b"\nGG\n", 0, None),
    ("line-consumes-20000", b">h\nAC\nGGG\n" + b"A" * 19999 + b"\nGG\n", 0, None),
    ("line-consumes-20001-crlf", b">h\nAC\n" + b"A" * 19999 + b"\r\nGG\n", 0, None),
    ("line-consumes-20000-unterminated", b">h\nAC\n" + b"A" * 20000, 0, None),
]

# ~150 bytes, three sections, every terminator
SWEEP = (b">one first\tsection\nACGTACGTAC\nGGGTTTAAAC\r\nAC\n\n>two\rTTTTGGGGCCCCAAAA\rACG\r\n>three 3\n"
         b"ACGTACGTACGTACGTACGT\nAACC\nG\r\rTTTTTTTTTTTT\nA")


def sweep_splits(data):
    """Every start of `data` with the lengths 1, to the byte before the next '>' and to the end."""
    out = []
    for s in range(len(data)):
        nxt = data.find(b">", s + 1)
        to_next = (nxt if nxt >= 0 else len(data)) - 1 - s
        for n in sorted({1, max(to_next, 0), len(data) - s}):
            out.append((s, n))
    return out


def case_range(case):
    _, data, start, length = case
    return data, start, (len(data) - start if length is None else length)
