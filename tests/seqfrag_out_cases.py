"""Shared inputs of the FASTQ / QSEQ output tests: fragments (seqfrag_ref's dicts) as the host
columns hbam_frag_render takes, the field grid, the quality-edge records, the recorded assertions of
the reference's own writer tests (tests/golden/seqfrag_out/expected.json) and the file format of
tools/frag_text_host.cpp."""
import json
import os
import random
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "golden", "seqfrag_out", "expected.json")

FASTQ, QSEQ = 0, 1
SANGER, ILLUMINA = 0, 1
USE_KEY, INDEX_DOTS = 1, 2
INT_COLS = ("run", "lane", "tile", "xpos", "ypos", "read", "filter_passed", "control")
STR_COLS = ("instrument", "flowcell", "index")
PRESENT = {"instrument": 0x001, "run": 0x002, "flowcell": 0x004, "lane": 0x008, "tile": 0x010, "xpos": 0x020,
           "ypos": 0x040, "read": 0x080, "filter_passed": 0x100, "control": 0x200, "index": 0x400}

INTS = [0, 1, -1, 9, 10, 99, 100, 999999999, 1000000000, 2 ** 31 - 1, -2 ** 31]
STR_LENS = [0, 1, 15, 16, 17]
BULK_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
LONG = 10000


def _b(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def columns(records):
    """Fragments -> host columns (numpy) and the window their strings stand in.  An absent integer
    column holds a value that must not show, an absent string a pair that points far outside the
    window."""
    n = len(records)
    c = {"n": n, "present": np.zeros(n, np.uint32)}
    for k in INT_COLS:
        c[k] = np.full(n, 123456789, np.int32)
    for k in STR_COLS:
        c[k] = np.tile(np.array([0xfffffff0, 77], np.uint32), (n, 1))
    window = bytearray(b"\xa5\xa5\xa5")  # no string starts at offset 0
    pools = {"key": bytearray(), "seq": bytearray(), "qual": bytearray()}
    offs = {k: [0] for k in pools}
    for i, f in enumerate(records):
        p = 0
        for k in INT_COLS:
            if f[k] is not None:
                p |= PRESENT[k]
                c[k][i] = int(f[k])
        for k in STR_COLS:
            if f[k] is not None:
                p |= PRESENT[k]
                s = _b(f[k])
                c[k][i] = (len(window), len(s))
                window += s
        c["present"][i] = p
        for k in pools:
            pools[k] += _b(f.get(k) or b"")
            offs[k].append(len(pools[k]))
    for k in pools:
        c[k] = np.frombuffer(bytes(pools[k]), np.uint8).copy()
        c[k + "_off"] = np.array(offs[k], np.uint64)
    c["window"] = bytes(window)
    return c


def host_input(c, fmt, encoding, flags):
    """The input file of tools/frag_text_host.cpp."""
    out = [struct.pack("<8Q", c["n"], len(c["key"]), len(c["seq"]), len(c["qual"]), len(c["window"]), fmt, encoding,
                       flags), c["present"].tobytes()]
    out += [c[k].tobytes() for k in INT_COLS]
    out += [np.ascontiguousarray(c[k]).tobytes() for k in STR_COLS]
    out += [c[k + "_off"].tobytes() for k in ("key", "seq", "qual")]
    out += [c[k].tobytes() for k in ("key", "seq", "qual")]
    out.append(c["window"])
    return b"".join(out)


def host_output(blob, n):
    """tools/frag_text_host.cpp's output -> [(flags, bytes)] per record."""
    out, p = [], 0
    for _ in range(n):
        flags, ln = struct.unpack_from("<II", blob, p)
        out.append((flags, blob[p + 8:p + 8 + ln]))
        p += 8 + ln
    assert p == len(blob)
    return out


def fragment(**kw):
    f = {"key": b"", "seq": b"", "qual": b"", "instrument": None, "run": None, "flowcell": None, "lane": None,
         "tile": None, "xpos": None, "ypos": None, "read": None, "filter_passed": None, "control": None, "index": None}
    f.update(kw)
    return f


def _text(r, n, alphabet):
    return bytes(r.choice(alphabet) for _ in range(n))


def grid_records(seed=5):
    """2,048 records, record k with present mask k: every integer of INTS in every integer column,
    string and key lengths over STR_LENS, sequence and quality lengths over BULK_LENS (different in
    one record), 'N' and '.' in sequences and index strings, qualities in [33, 95] (legal for every
    format and encoding), and 10,000-byte sequences / qualities at records 100, 101 and 1000."""
    r = random.Random(seed)
    out = []
    names = list(PRESENT)
    for k in range(2048):
        f = fragment()
        for j, name in enumerate(names):
            if not k & PRESENT[name]:
                continue
            if name == "filter_passed":
                f[name] = (k >> 3) & 1
            elif name in INT_COLS:
                f[name] = INTS[(k // 7 + 3 * j) % len(INTS)]
            else:
                f[name] = _text(r, STR_LENS[(k // 3 + j) % len(STR_LENS)], b"ACGTN.xyz-_" if name == "index" else b"Mabc019_")
        ls, lq = BULK_LENS[k % len(BULK_LENS)], BULK_LENS[(7 * k + 3) % len(BULK_LENS)]
        if k == 100:
            ls, lq = LONG, LONG
        elif k == 101:
            ls = LONG
        elif k == 1000:
            lq = LONG
        f["seq"] = _text(r, ls, b"ACGTN")
        f["qual"] = bytes(r.randrange(33, 96) for _ in range(lq))
        f["key"] = _text(r, STR_LENS[(k // 5) % len(STR_LENS)], b"read:/ 0123N.")
        out.append(f)
    return out


def short_record(r, ls=None, lq=None):
    ls = r.randrange(20, 80) if ls is None else ls
    lq = ls if lq is None else lq
    return fragment(key=b"r%d" % r.randrange(1000), instrument=b"M1", run=r.randrange(100), lane=1, tile=2, xpos=3, ypos=4,
                    read=1, filter_passed=1, index=b"ACG", seq=_text(r, ls, b"ACGTN"),
                    qual=bytes(r.randrange(33, 96) for _ in range(lq)))


def with_qual_byte(records, at, where, byte):
    """A copy of `records` with quality byte `where` (0 or -1) of record `at` set to `byte`."""
    out = [dict(f) for f in records]
    q = bytearray(out[at]["qual"])
    q[where] = byte
    out[at]["qual"] = bytes(q)
    return out


# ---- the recorded assertions of the reference's own tests ------------------------------------------
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def case_fragment(section, case):
    f = fragment()
    vals = dict(section["base"])
    vals.update(case.get("fragment", {}))
    for k, v in vals.items():
        f[k] = v.encode("ascii") if isinstance(v, str) else v
    return f


def java_split(s, sep):
    """String.split(sep): trailing empty strings are dropped."""
    parts = s.split(sep)
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def check_case(case, out):
    """One expected.json entry against the bytes a writer produced for it."""
    s = bytes(out).decode("ascii")
    lines, fields = java_split(s, "\n"), java_split(s, "\t")
    if "lines" in case:
        assert len(lines) == case["lines"], (case["test"], lines)
    if "id_prefix" in case:
        assert lines[0].startswith(case["id_prefix"]), case["test"]
    if "id_pieces" in case:
        id_line = lines[0][1:]
        pieces = id_line.split(" ")[0].split(":") + id_line.split(" ")[1].split(":")
        assert pieces == case["id_pieces"], (case["test"], pieces)
    for k, v in case.get("line", {}).items():
        assert lines[int(k)] == v, (case["test"], k, lines[int(k)], v)
    if "fields" in case:
        assert len(fields) == case["fields"], (case["test"], fields)
    for k, v in case.get("field", {}).items():
        assert fields[int(k)] == v, (case["test"], k, fields[int(k)], v)
