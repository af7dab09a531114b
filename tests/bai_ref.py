"""Plain-Python checker of the BAI index and of indexed region queries (tests/test_bai.py).

A restatement of the indexing rules over the CPU oracle's decode (oracle.read_split of the whole
file plus a CIGAR walk), written as the streaming loop [htsjdk] BAMIndexer runs (one record at a
time, chunks appended or extended per bin) — not the sort / scan / compact form the device uses —
plus a .bai parser, a brute-force overlap query and a small BAM writer for crafted records.  The
product never imports this module.  htsjdk is not in the reference tree: the rules are restated
from memory (DESIGN.md lists them), so parity is between two restatements."""
import struct

import numpy as np

import helpers
import oracle

EDATA, EINDEX = -7, -13
META_BIN = 37450
MAX_WIN = 32768
_REF_OPS = (0, 2, 3, 7, 8)  # M D N = X


def window(p):
    return (0 if p <= 0 else p - 1) >> 14


def same_or_adjacent(a, b):
    return (a >> 16) == (b >> 16) or (a >> 16) + 1 == (b >> 16)


def reg2bin(beg, end):
    """SAM spec 5.3 over the 0-based half-open [beg, end)."""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def end_voffset(data, first_voffset):
    """The file pointer after the last record a reader gets: the start of the first empty BGZF
    block after the first record's block, else the end of the file."""
    b = oracle.scan_blocks(data)
    for c, s in zip(b["coff"], b["isize"]):
        if int(s) == 0 and int(c) > (int(first_voffset) >> 16):
            return int(c) << 16
    return len(data) << 16


def decode(data):
    """The oracle's whole-file decode plus start1 / reflen / end1 of every record."""
    data = np.asarray(data, np.uint8)
    h = oracle.read_header(data)
    r = oracle.read_split(data, h["first_voffset"], (len(data) << 16) | 0xffff)
    n = r["n"]
    p = oracle.pools(r)
    ok = p["layout_ok"].astype(bool)
    cnt = np.where(ok, r["n_cigar"].astype(np.int64), 0)
    ops = p["cigars"].astype(np.int64)
    assert len(ops) == int(cnt.sum())
    rec = np.repeat(np.arange(n, dtype=np.int64), cnt)
    reflen = np.zeros(n, np.int64)
    np.add.at(reflen, rec, np.where(np.isin(ops & 15, _REF_OPS), ops >> 4, 0))
    start1 = r["pos"].astype(np.int64) + 1
    end1 = np.where(r["flag"] & 4, 0, start1 + reflen - 1)
    r.update(header=h, n_ref=h["n_ref"], layout_ok=p["layout_ok"], reflen=reflen, start1=start1, end1=end1,
             end_voffset=end_voffset(data, h["first_voffset"]))
    return r


def build(rec, n_ref=None, end_voff=None):
    """-> (status, err_record, .bai bytes or None, facts about what the input exercised)."""
    n_ref = rec["n_ref"] if n_ref is None else n_ref
    end_voff = rec["end_voffset"] if end_voff is None else end_voff
    if rec["status"] != 0:
        return rec["status"], rec["err_record"], None, {}
    n = rec["n"]
    refs = [dict(bins={}, lin={}, first=None, last=0, al=0, un=0, maxw=-1) for _ in range(n_ref)]
    facts = dict(multi_chunk_bin=False, extended_across_block=False, multi_window_record=False,
                 filled_slot=False, empty_reference=False, placed_unmapped=False, n_no_coor=0)
    cur = None
    voff = [int(x) for x in rec["voffset"]]
    for i in range(n):
        if int(rec["pos"][i]) < 0:
            facts["n_no_coor"] += 1
            continue
        r = int(rec["ref_id"][i])
        if r < 0 or r >= n_ref or (cur is not None and r < cur):
            return EDATA, i, None, facts
        cur = r
        s, e = int(rec["start1"][i]), int(rec["end1"][i])
        w0, w1 = (window(s - 1),) * 2 if e == 0 else (window(s), window(e))
        if w0 >= MAX_WIN or w1 >= MAX_WIN:
            return EINDEX, i, None, facts
        beg, end = voff[i], voff[i + 1] if i + 1 < n else end_voff
        R = refs[r]
        chunks = R["bins"].setdefault(int(rec["bin"][i]), [])
        if chunks and same_or_adjacent(chunks[-1][1], beg):
            facts["extended_across_block"] |= (chunks[-1][0] >> 16) != (end >> 16)
            chunks[-1][1] = end
        else:
            chunks.append([beg, end])
            facts["multi_chunk_bin"] |= len(chunks) > 1
        for w in range(w0, w1 + 1):
            if w not in R["lin"] or beg < R["lin"][w]:
                R["lin"][w] = beg
        facts["multi_window_record"] |= w1 > w0
        R["maxw"] = max(R["maxw"], w1)
        R["first"] = beg if R["first"] is None else min(R["first"], beg)
        R["last"] = max(R["last"], end)
        if int(rec["flag"][i]) & 4:
            R["un"] += 1
            facts["placed_unmapped"] = True
        else:
            R["al"] += 1
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    for R in refs:
        nb = len(R["bins"])
        facts["empty_reference"] |= nb == 0
        out.append(struct.pack("<i", nb + 1 if nb else 0))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<Ii", b, len(R["bins"][b])))
            out.extend(struct.pack("<QQ", x, y) for x, y in R["bins"][b])
        if nb:
            out.append(struct.pack("<IiQQQQ", META_BIN, 2, R["first"], R["last"], R["al"], R["un"]))
        out.append(struct.pack("<i", R["maxw"] + 1))
        last = 0
        for w in range(R["maxw"] + 1):
            if w in R["lin"]:
                last = R["lin"][w]
            elif last:
                facts["filled_slot"] = True
            out.append(struct.pack("<Q", last))
    out.append(struct.pack("<Q", facts["n_no_coor"]))
    return 0, None, b"".join(out), facts


def parse(bai):
    """.bai bytes -> (refs: [dict(bins={bin: [(beg, end)]}, lin=[...])], n_no_coor or None); the
    metadata pseudo-bin is kept under its number."""
    assert bai[:4] == b"BAI\x01"
    (n_ref,) = struct.unpack_from("<i", bai, 4)
    p = 8
    refs = []
    for _ in range(n_ref):
        (nb,) = struct.unpack_from("<i", bai, p)
        p += 4
        bins = {}
        for _ in range(nb):
            b, nc = struct.unpack_from("<Ii", bai, p)
            p += 8
            bins[b] = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(nc)]
            p += 16 * nc
        (ni,) = struct.unpack_from("<i", bai, p)
        p += 4
        lin = list(struct.unpack_from("<%dQ" % ni, bai, p))
        p += 8 * ni
        refs.append(dict(bins=bins, lin=lin))
    nnc = struct.unpack_from("<Q", bai, p)[0] if p + 8 <= len(bai) else None
    return refs, nnc


def overlapping(rec, r, beg, end, contained=False):
    """Brute force: indices of the records of reference r overlapping (contained in) the 1-based
    inclusive [beg, end]; beg <= 0 means 1, end <= 0 the end of the reference."""
    qb = 1 if beg <= 0 else beg
    qe = (1 << 62) if end <= 0 else end
    s = rec["start1"]
    e = np.where(rec["end1"] == 0, s, rec["end1"])
    on = rec["ref_id"] == r
    keep = on & (s >= qb) & (e <= qe) if contained else on & (s <= qe) & (e >= qb)
    return np.nonzero(keep)[0]


def record_bytes(rec, idx):
    """block_size + record bytes of records idx of a decode() result."""
    fixed = oracle.record_fixed_bytes(rec, idx)
    vo = rec["var_off"]
    return [fixed[k].tobytes() + rec["var"][int(vo[i]):int(vo[i + 1])].tobytes() for k, i in enumerate(idx)]


def craft_bam(refs, records, block=65280):
    """A BAM from scratch: refs = [(name bytes, length)], records = dicts with ref, pos and optionally
    flag, cigar (u32 ops), n_cigar / stored_l_seq (the stored values, when they should differ from
    what the variable block holds), bin, l_seq, name."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(
        b"@SQ\tSN:" + nm + b"\tLN:" + str(ln).encode() + b"\n" for nm, ln in refs)
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for nm, ln in refs:
        out += [struct.pack("<i", len(nm) + 1), nm, b"\0", struct.pack("<i", ln)]
    for k, r in enumerate(records):
        cig = list(r.get("cigar", ()))
        flag = r.get("flag", 0)
        l_seq = r.get("l_seq", 4)
        name = r.get("name", b"r%05d" % k) + b"\0"
        span = sum(c >> 4 for c in cig if (c & 15) in _REF_OPS)
        b = r.get("bin", reg2bin(r["pos"], r["pos"] + max(1, span)) if 0 <= r["pos"] < (1 << 29) else 4680)
        var = name + b"".join(struct.pack("<I", c) for c in cig) + bytes((max(l_seq, 0) + 1) // 2) + \
            b"\x20" * max(l_seq, 0)
        body = struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], len(name), r.get("mapq", 30), b,
                           r.get("n_cigar", len(cig)), flag, r.get("stored_l_seq", l_seq), -1, -1, 0) + var
        out.append(struct.pack("<i", len(body)) + body)
    return np.frombuffer(helpers.bgzf_pack(b"".join(out), block=block), np.uint8).copy()
