"""Crafted BGZF files for the sparse chain build (build_chain_sparse in csrc/hbam_capi.hip; k_seg_scan,
k_seg_walk, k_seg_stitch, k_seg_table in csrc/hbam_kernels.hip), a Python model of its segment,
stitch and cap bookkeeping, and the cases shared by test_sparse_chain_model.py (CPU: each case has
the structure it claims) and test_sparse_chain_gpu.py (device: sparse path = dense path = oracle).

A file is a BAM stream of "host" records (chain_craft.BamStream) with opaque payloads: random bytes
deflate to members of about their own size, so a few hundred KiB of file need no more stream than
that, and a stored member carries its payload verbatim, so header-shaped bytes can be put at a
chosen file position.  The segment size is chosen after the file is laid out (HBAM_CHAIN_SEG), which
puts a segment boundary wherever a case wants it."""
import functools
import struct
import zlib

import numpy as np

import chain_craft as cc

MAGIC = b"\x1f\x8b\x08\x04"
HEAD = MAGIC + b"\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"  # 16 bytes, BSIZE follows
WINDOW = 65536                 # csrc/hbam_internal.h: SEG_WINDOW
CANDS = 4                      # SEG_CANDS
SEG_MIN = WINDOW + 64          # SEG_MIN
HOP_BYTES = 2048               # SEG_HOP_BYTES
F_NOCAND, F_MANY, F_DERAIL, F_CAP, F_STITCH = 1, 2, 4, 8, 16  # SEGF_*
STORED_OVERHEAD = 18 + 5 + 8   # header, one stored DEFLATE block header, footer
HBAM_EEOF, HBAM_EMORE = -5, -12  # include/hbam.h


def fake_header(bsize_plus_1):
    return HEAD + struct.pack("<H", bsize_plus_1 - 1)


def stored_member(chunk):
    """A BGZF member whose DEFLATE stream is one stored block: chunk's bytes lie verbatim at
    member offset 23."""
    chunk = bytes(chunk)
    assert len(chunk) + STORED_OVERHEAD <= 65536
    cd = b"\x01" + struct.pack("<HH", len(chunk), len(chunk) ^ 0xffff) + chunk
    assert zlib.decompress(cd, -15) == chunk
    return HEAD + struct.pack("<H", len(cd) + 25) + cd + struct.pack("<II", zlib.crc32(chunk), len(chunk))


class Group:
    """One member: a host record with `payload` bytes of opaque payload (random, or zeros when
    stored), then `trues` true records.  decoys: (payload offset, bytes)."""

    def __init__(self, payload, stored=False, decoys=(), trues=3, empties_before=0):
        self.payload, self.stored, self.decoys, self.trues = payload, stored, list(decoys), trues
        self.empties_before = empties_before


def build_file(groups, seed=1):
    """-> (file bytes, coff of every member incl. empties and the EOF block, header_len,
    payload file position of each stored group (None otherwise))."""
    rng = np.random.default_rng(seed)
    s = cc.BamStream()
    s.add_trues(20)
    edges, pay_u = [0], []
    for g in groups:
        body = bytearray(g.payload) if g.stored else bytearray(rng.integers(0, 256, g.payload, dtype=np.uint8).tobytes())
        for off, b in g.decoys:
            body[off:off + len(b)] = b
        pay_u.append(s.payload_start())
        s.add_host(bytes(body))
        s.add_trues(g.trues)
        edges.append(s.pos)
    u = s.bytes()
    out, pay_pos, at = [], [], 0
    for k, g in enumerate(groups):
        out += [cc.BGZF_EOF] * g.empties_before
        at += len(cc.BGZF_EOF) * g.empties_before
        chunk = u[edges[k]:edges[k + 1]]
        m = stored_member(chunk) if g.stored else cc.bgzf_member(chunk)
        pay_pos.append(at + 23 + pay_u[k] - edges[k] if g.stored else None)
        out.append(m)
        at += len(m)
    out.append(cc.BGZF_EOF)
    data = b"".join(out)
    coff, _ = cc.bgzf_layout(data)
    return data, coff, s.header_len, pay_pos


# ---- the model ---------------------------------------------------------------------------------------
def header_at(d, p, end):
    """k_scan_chunks' predicate"""
    return p + 18 <= end and d[p:p + 4] == MAGIC and d[p + 10:p + 12] == b"\x06\x00"


def candidates(d, lo, hi, end):
    out, p = [], d.find(MAGIC, lo, min(hi + 3, end))
    while p != -1 and p < hi:
        if header_at(d, p, end):
            out.append(p)
        p = d.find(MAGIC, p + 1, min(hi + 3, end))
    return out


def true_chain(d, start, end=None):
    """The dense path's answer (its host walk): the blocks from `start` and where the chain stops."""
    end = len(d) if end is None else end
    p, out = start, []
    while header_at(d, p, end):
        bl = struct.unpack_from("<H", d, p + 16)[0] + 1
        if bl < 18 or p + bl > end:
            break
        out.append(p)
        p += bl
    return out, p


def model(d, start, seg, end=None):
    """build_chain_sparse restated: per segment its begin, its window's candidates, how many of them
    the walker tried, its start, exit and block positions; the flags; and, when none is raised, the
    table and the chain's end."""
    end = len(d) if end is None else end
    assert seg >= SEG_MIN and start < end
    span = end - start
    nseg = max(1, span // seg)
    cap = seg // HOP_BYTES
    flags, segs = 0, []
    for w in range(nseg):
        b = start + w * seg
        stop = b + seg if w + 1 < nseg else None
        if w == 0:
            cands = [start]
        else:
            cands = candidates(d, b, min(b + WINDOW, end), end)
            if not cands:
                flags |= F_NOCAND
            if len(cands) > CANDS:
                flags |= F_MANY
                cands = []
        sg = dict(begin=b, cands=cands, tried=0, start=None, exit=None, pos=[])
        why = F_DERAIL if cands else 0
        for pf in cands:
            sg["tried"] += 1
            p, pos, ok = pf, [], True
            while stop is None or p < stop:
                if p + 18 > end:
                    break
                if not header_at(d, p, end):
                    ok = False
                    break
                bl = struct.unpack_from("<H", d, p + 16)[0] + 1
                if bl < 18:
                    ok = False
                    break
                if p + bl > end:
                    break
                if len(pos) >= cap:
                    ok, why = False, F_CAP
                    break
                pos.append(p)
                p += bl
            if ok:
                sg.update(start=pf, exit=p, pos=pos)
                break
            if why == F_CAP:
                break
        if sg["start"] is None:
            flags |= why
        segs.append(sg)
    for w in range(1, nseg):
        if segs[w]["start"] is None or segs[w - 1]["exit"] != segs[w]["start"]:
            flags |= F_STITCH
    out = dict(nseg=nseg, cap=cap, segs=segs, flags=flags, sparse=flags == 0)
    if flags == 0:
        out["coff"] = [p for sg in segs for p in sg["pos"]]
        out["end_pos"] = segs[-1]["exit"]
    return out


# ---- the cases ---------------------------------------------------------------------------------------
class Case:
    """window = the bytes handed to the library (file bytes [comp_base, comp_base + len(window)));
    `start` is relative to the window; seg = HBAM_CHAIN_SEG."""

    def __init__(self, name, data, seg, header_len, start=0, comp_base=0, window_len=None, v_start=None):
        self.name, self.seg, self.start, self.comp_base = name, int(seg), start, comp_base
        self.file_len = len(data)
        n = len(data) - comp_base if window_len is None else window_len
        self.window = bytes(data[comp_base:comp_base + n])
        self.file_end = comp_base + n >= len(data)
        self.v_start = ((comp_base + start) << 16 | (header_len if comp_base + start == 0 else 0)) if v_start is None else v_start
        self.v_end = (comp_base + n) << 16 | 0xffff

    @functools.lru_cache(None)
    def model(self):
        return model(self.window, self.start, self.seg)

    @functools.lru_cache(None)
    def truth(self):
        return true_chain(self.window, self.start)


def _plain_groups(n=20, seed=3):
    rng = np.random.default_rng(seed)
    return [Group(int(x)) for x in rng.integers(9000, 40000, n)]


@functools.lru_cache(None)
def plain_file():
    return build_file(_plain_groups())


def _k_after(coff, at):
    return min(k for k, c in enumerate(coff) if c >= at)


@functools.lru_cache(None)
def case_boundary(kind):
    """exact: member k starts on segment 1's begin.  one: it reaches 1 byte into segment 1 (its last
    byte is the segment's first).  most: it starts 1 byte before segment 1 (clen - 1 bytes inside)."""
    data, coff, hl, _ = plain_file()
    k = _k_after(coff, SEG_MIN + 1)
    seg = {"exact": coff[k], "one": coff[k + 1] - 1, "most": coff[k] + 1}[kind]
    c = Case("boundary_" + kind, data, seg, hl)
    c.k = k
    return c


@functools.lru_cache(None)
def case_full_block(kind):
    """A member of exactly 65,536 bytes.  at_begin: it starts on segment 1's begin and fills its
    window.  last_pos: it starts 1 byte before, so the window's only block start is its last
    position."""
    groups = _plain_groups(4, seed=4) + [Group(65536 - STORED_OVERHEAD - cc.BamStream.HOST_PREFIX, stored=True, trues=0)] + \
        _plain_groups(4, seed=5)
    data, coff, hl, _ = build_file(groups)
    k = 4
    assert coff[k + 1] - coff[k] == 65536 and coff[k] >= SEG_MIN
    c = Case("full_block_" + kind, data, coff[k] if kind == "at_begin" else coff[k] + 1, hl)
    c.k = k
    return c


@functools.lru_cache(None)
def case_one_segment(kind):
    """shorter: the file is shorter than one segment.  exact: exactly one.  almost_two: one or two
    bytes short of two (still one segment, the longest there is).  two: two segments (the second
    takes the odd byte, if any)."""
    data, coff, hl, _ = plain_file()
    n = len(data)
    seg = {"shorter": n + 1000, "exact": n, "almost_two": n // 2 + 1, "two": n // 2}[kind]
    return Case("one_segment_" + kind, data, seg, hl)


def _fake_file(decoys):
    groups = _plain_groups(3, seed=6) + [Group(30000, stored=True, decoys=decoys), Group(50000), Group(50000), Group(20000)]
    return build_file(groups, seed=7)


FAKE_AT = 1000  # payload offset of the first fake header


@functools.lru_cache(None)
def case_fake(kind):
    """A stored member whose payload holds a well-formed header exactly on segment 1's begin, before
    the window's true block start.  garbage: its hop lands on zeros.  second: on a second fake
    header, whose hop lands on zeros.  rejoin: on the next true block start.  many: five more fake
    headers follow it (more candidates than slots)."""
    _, coff, _, pay = _fake_file(())
    f = pay[3] + FAKE_AT
    decoys = {"garbage": [(FAKE_AT, fake_header(100))],
              "second": [(FAKE_AT, fake_header(100)), (FAKE_AT + 100, fake_header(200))],
              "rejoin": [(FAKE_AT, fake_header(coff[4] - f))],
              "many": [(FAKE_AT + 40 * i, fake_header(100)) for i in range(6)]}[kind]
    data, coff2, hl, pay2 = _fake_file(tuple(decoys))
    assert coff2 == coff and pay2 == pay and f >= SEG_MIN
    c = Case("fake_" + kind, data, f, hl)
    c.fake, c.next_true = f, coff[4]
    return c


@functools.lru_cache(None)
def case_empties():
    """40 empty members in segment 0, whose walker may take 32 hops."""
    g = _plain_groups(10, seed=8)
    g[1].empties_before = 40
    data, coff, hl, _ = build_file(g)
    return Case("empties_hop_cap", data, SEG_MIN, hl)


@functools.lru_cache(None)
def case_window_mid_block():
    """The window ends 100 bytes into a member and is not the file's end."""
    data, coff, hl, _ = plain_file()
    k = len(coff) - 3
    c = Case("window_mid_block", data, SEG_MIN + 500, hl, window_len=coff[k] + 100)
    c.k = k
    return c


@functools.lru_cache(None)
def case_truncated(kind):
    """The file's last member cut short.  body: 10 bytes of the EOF block missing.  header: only 10
    bytes of it left.  member: the last data member loses its tail (and the EOF block)."""
    data, coff, hl, _ = plain_file()
    n = {"body": len(data) - 10, "header": coff[-1] + 10, "member": coff[-1] - 1000}[kind]
    return Case("truncated_" + kind, data[:n], SEG_MIN + 500, hl)


@functools.lru_cache(None)
def case_corrupt():
    """A member in the middle of the file (well inside a segment) with a broken magic."""
    data, coff, hl, _ = plain_file()
    seg = SEG_MIN + 500
    k = _k_after(coff, seg + WINDOW)  # past segment 1's window
    bad = bytearray(data)
    bad[coff[k]] ^= 0xff
    c = Case("corrupt_header", bytes(bad), seg, hl)
    c.k, c.bad_at = k, coff[k]
    return c


@functools.lru_cache(None)
def case_bad_start():
    """The chain is asked for from a position 3 bytes into member 1."""
    data, coff, hl, _ = plain_file()
    return Case("bad_start", data, SEG_MIN + 500, hl, start=coff[1] + 3)


@functools.lru_cache(None)
def case_comp_base(kind):
    """Windows of a file that do not begin at its offset 0 (bench config #4's shape): from member 2
    to the file's end, and from member 2 to 100 bytes into a later member."""
    data, coff, hl, _ = plain_file()
    wl = None if kind == "to_end" else coff[len(coff) - 3] + 100 - coff[2]
    return Case("comp_base_" + kind, data, SEG_MIN + 500, hl, comp_base=coff[2], window_len=wl)


@functools.lru_cache(None)
def case_inner_start():
    """The chain starts at member 3 of the window (a split that begins inside it)."""
    data, coff, hl, _ = plain_file()
    return Case("inner_start", data, SEG_MIN + 500, hl, start=coff[3])


def all_cases():
    return ([case_boundary(k) for k in ("exact", "one", "most")] +
            [case_full_block(k) for k in ("at_begin", "last_pos")] +
            [case_one_segment(k) for k in ("shorter", "exact", "almost_two", "two")] +
            [case_fake(k) for k in ("garbage", "second", "rejoin", "many")] +
            [case_empties(), case_window_mid_block()] +
            [case_truncated(k) for k in ("body", "header", "member")] +
            [case_corrupt(), case_bad_start(), case_inner_start()] +
            [case_comp_base(k) for k in ("to_end", "mid_block")])


CASE_NAMES = [
    "boundary_exact", "boundary_one", "boundary_most", "full_block_at_begin", "full_block_last_pos",
    "one_segment_shorter", "one_segment_exact", "one_segment_almost_two", "one_segment_two",
    "fake_garbage", "fake_second", "fake_rejoin", "fake_many", "empties_hop_cap", "window_mid_block",
    "truncated_body", "truncated_header", "truncated_member", "corrupt_header", "bad_start", "inner_start",
    "comp_base_to_end", "comp_base_mid_block"]


@functools.lru_cache(None)
def by_name():
    d = {c.name: c for c in all_cases()}
    assert list(d) == CASE_NAMES
    return d
