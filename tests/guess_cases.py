"""The catalogue of crafted guess windows (builders and describe(): tests/guess_craft.py).

A Case holds one file, its guesses and what each guess claims: the side of the block cache's and the
listed scan's capacities it falls on (cached / listed, and the magic counts where the case is about
them), and the oracle's outcome class: "rec" (a true record start; `at` = the file offset of the
member it lies in, where the case pins that), "end" (no record: the guess returns its `end`) or a
negative error code that escapes guessNextBAMRecordStart.  test_guess_model.py asserts every claim
on the CPU; test_guess_gpu.py runs the same guesses on the device.

Families: A cache capacity, B list capacity, C listed/serial threshold, D scan patterns, E block
errors by position, F candidate loop, G chain memo.  Every file starts with the BGZF magic (the
guesser's constructor leaves the file's first four bytes in its buffer).
"""
import numpy as np

import guess_craft as gc
from guess_craft import File, N_REF

EDATA = -7
LISTED_MIN = 0xffff + 4      # bytes that must follow beg for the listed scan


class Case:
    def __init__(self, family, name, f, guesses, block=None, up=0, accepted0=None, n_accepted=None, chain=None,
                 chain_from=None, doc=""):
        self.family, self.name, self.doc = family, name, doc
        self.data = f if isinstance(f, bytes) else f.bytes()
        self.starts = set() if isinstance(f, bytes) else f.starts
        self.guesses = guesses
        self.n_ref = N_REF
        # the member describe() looks into, and what it must find there: the first accepted offset
        # from `up`, the number of accepted offsets, (op, n) for the number of record starts on the
        # chain from chain_from (default: the first accepted offset)
        self.block, self.up, self.accepted0, self.n_accepted, self.chain = block, up, accepted0, n_accepted, chain
        self.chain_from = chain_from
        assert self.data[:4] == gc.MAGIC
        assert len(self.data) <= 300 << 10, (name, len(self.data))

    def np(self):
        return np.frombuffer(self.data, np.uint8)

    def __repr__(self):
        return "%s:%s" % (self.family, self.name)


def G(beg, end, out, cached=True, listed=False, n_window=None, n_first=None, at=None, uoff=None):
    return dict(beg=beg, end=end, out=out, cached=cached, listed=listed, n_window=n_window, n_first=n_first,
                at=at, uoff=uoff)


def false_magic_block(f, n):
    """a stored member whose one record carries n harmless false magics"""
    return f.add(gc.record(name=b"host\0", body=gc.false_magic() * n), [0], level=0)


# ---- A: the window block cache's capacity -------------------------------------------------------------
def a_tiny(n):
    """n stored members of one 40-byte record each (the smallest member whose record the candidate
    loop tests).  From beg = 0 the window holds n magics, from beg = 1 one fewer."""
    f = File()
    for i in range(n):
        f.add(gc.record(pos=i, name=b"abc\0"), [0], level=0)
    e = f.pos
    gs = [G(0, e, "rec", n <= 256, n_window=n, at=0, uoff=0),
          G(1, e, "rec", n - 1 <= 256, n_window=n - 1, at=f.coff[1], uoff=0)]
    return Case("A", "tiny%d" % n, f, gs[:1] if n == 600 else gs)


def a_false(n):
    """n - 4 false magics inside a stored member, four ordinary members behind it: the scan from
    beg = 1 walks every false magic (n magics in the window); from beg = 0 the window holds n + 1."""
    f = File()
    false_magic_block(f, n - 4)
    f.chain(1, 4)
    e = f.pos
    gs = [G(1, e, "rec", n <= 256, n_window=n, at=f.coff[1], uoff=0),
          G(0, e, "rec", n + 1 <= 256, n_window=n + 1, at=0, uoff=0)]
    return Case("A", "false%d" % n, f, gs[:1] if n == 600 else gs)


# ---- B: the listed scan's capacity ---------------------------------------------------------------------
def b_list(n):
    """Exactly n magic positions in [0, first_end] of a window long enough for the listed scan."""
    def build(k):
        f = File()
        false_magic_block(f, k)
        f.chain(1, 4)
        f.filler(1 + LISTED_MIN + 4000)
        return f
    f = build(n - 8)
    have = gc.describe(f.bytes(), 1, f.pos)["n_first"]
    f = build(n - 8 + n - have)
    return Case("B", "list%d" % n, f, [G(1, f.pos, "rec", False, n <= 512, n_first=n, at=f.coff[1], uoff=0)])


# ---- C: the listed / serial threshold --------------------------------------------------------------------
def _c_file():
    f = File()
    f.ordinary(0)
    f.chain(1, 4)
    f.filler(90000)
    return f


def c_avail(avail):
    """The file cut so that `avail` bytes follow beg = 1; end - beg = 0xffff, 0x10000, 0x10003.  Only
    65539 bytes behind beg with end - beg >= 65539 list."""
    f = _c_file()
    data = f.bytes()[:1 + avail]
    c = Case("C", "avail%d" % avail, data,
             [G(1, 1 + s, "rec", listed=(avail >= LISTED_MIN and s >= LISTED_MIN), at=f.coff[1], uoff=0)
              for s in (0xffff, 0x10000, 0x10003)])
    c.starts = f.starts
    return c


def c_empty():
    """end <= beg, and beg one to three bytes before EOF"""
    f = _c_file()
    n = f.pos
    return Case("C", "empty", f, [G(100, 100, "end"), G(100, 50, "end"), G(n - 1, n, "end"), G(n - 2, n, "end"),
                                  G(n - 3, n, "end"), G(n, n, "end")])


def c_edge(d, pre):
    """The first real member at window offset first_end + d (first_end = 0xffff; beg = 1).  pre: the
    four magic bytes stand right in front of it; the member's zero MTIME makes them a harmless
    false magic (XLEN 0), after which the scan reads at p0 + 4 without the end test: the q == p rule.
    Without it the member is reached by an advance, and found only below first_end.  With it the
    member is found up to d = 3 (p0 = first_end - 1 is the last false magic an advance reaches);
    at d = 4 the false magic itself stands at first_end and the guess is `end`."""
    f = File()
    f.ordinary(0)
    t = 1 + 0xffff + d
    f.junk_to(t - 4)
    f.raw(gc.MAGIC if pre else b"\xaa" * 4)
    f.chain(1, 4)
    f.filler(t + 8000)
    found = d < 0 or (pre and d <= 3)
    return Case("C", "edge%+d%s" % (d, "pre" if pre else ""), f,
                [G(1, f.pos, "rec" if found else "end", listed=True, at=f.coff[1] if found else None)])


# ---- D: scan patterns ---------------------------------------------------------------------------------------
def _d_tail(f, listed):
    if listed:
        f.filler(1 + LISTED_MIN + 4000)
    return f.pos


def d_prefix(prefix, phase, listed):
    """A prefix of the magic right in front of a real member (1f 1f 8b 08 04 and its kin): the skip
    rule must step by one, two, one.  phase shifts where the 3-byte stride arrives."""
    f = File()
    f.ordinary(0)
    f.junk(20 + phase)
    f.raw(prefix)
    f.chain(1, 4)
    e = _d_tail(f, listed)
    return Case("D", "prefix%s/%d%s" % (prefix.hex(), phase, "L" if listed else ""), f,
                [G(1, e, "rec", listed=listed, at=f.coff[1], uoff=0)])


D_SUBFIELDS = {
    "before": dict(pre=gc.subfield(b"XY", b"abcd")),     # found by the scan, refused by the reader (XLEN != 6)
    "after": dict(post=gc.subfield(b"XY", b"abcd")),
    "after_over": dict(post=b"XY\x10\x00ab"),            # the subfield after BC passes sub_end: p != sub_end
    "before_over": dict(pre=b"XY\x40\x00"),              # BC is never reached
}


def d_subfield(which, listed):
    """Member 1's extra field is not the plain BC subfield; the guess lands in member 2."""
    f = File()
    f.ordinary(0)
    f.ordinary(1, **D_SUBFIELDS[which])
    f.chain(2, 4)
    e = _d_tail(f, listed)
    return Case("D", "sub_%s%s" % (which, "L" if listed else ""), f,
                [G(1, e, "rec", listed=listed, at=f.coff[2], uoff=0)])


def d_harmful(listed):
    """A harmful false magic before the first real member: the guess is `end`.  Listed setting: the
    window is cut (by end) 66000 bytes behind beg so that the 65535-byte subfield still leaves it;
    with the whole file as the window the same magic is harmless."""
    f = File()
    f.ordinary(0)
    f.junk_to(6000)
    f.raw(gc.harmful_magic())
    f.chain(1, 4)
    if not listed:
        return Case("D", "harmful", f, [G(1, f.pos, "end")])
    f.filler(160000)
    return Case("D", "harmfulL", f, [G(1, 1 + 66000, "end", listed=True),
                                     G(1, f.pos, "rec", listed=True, at=f.coff[1], uoff=0)])


def d_cut(phase):
    """The window ends 1, 2 and 3 bytes into the magic of the first real member: the last read is
    short and `buf` keeps bytes of the reads before.  The byte 04 stands right in front of the
    magic, behind 22 + phase junk bytes, so the 3-byte stride arrives in each of its three phases:
    in one of them a full read is `aa aa aa 04` (it ends in 04) and the next starts one byte before
    the magic (test_guess_model.py restates the scan and asserts the reads).  A stale 04 in buf[3]
    under a 3-byte tail 1f 8b 08 cannot come from the scan alone: the read before is at most 3
    bytes back, so its last byte is one of the tail's own."""
    f = File()
    f.ordinary(0)
    f.junk(22 + phase)
    f.raw(b"\x04")
    p = f.pos
    f.chain(1, 4)
    c = Case("D", "cut/%d" % phase, f, [G(1, p + k, "end") for k in (1, 2, 3)])
    c.magic_at = p
    return c


# ---- E: block errors by position ----------------------------------------------------------------------------
E_KINDS = ["crc", "stored_body", "comp_body", "isize_small", "isize_big", "bsize_small", "xlen", "trunc"]
E_EXTRA = [("bsize_neg", 1)]   # (kind, position): kinds run at one position only


def e_case(kind, where, uncached):
    """Five ordinary members, member `where` (0, 1, 2) damaged.  uncached: a stored member of 300
    harmless false magics stands in front and beg = 1, so every readBlock inflates in-lane.

    Outcomes the oracle gives (E_OUTCOME, asserted in test_guess_model.py).  Damage in member 0 is
    skipped whatever it is (the seek to the candidate block catches every Throwable): the guess
    lands in member 1; only trunc@0 leaves no whole member and gives `end`.  In member 1 or 2:
    crc, isize_small, isize_big (the stream ends short of 65537 bytes: "Did not inflate expected
    amount") and xlen (an extra subfield behind BC, so BSIZE is where the reader looks for it) are
    SAMFormatException: every chain into the member is skipped, then the member itself, and the
    guess lands behind it.  stored_body and comp_body are the inflater's error and escape as EDATA.
    bsize_small (BSIZE = 19, so the reader takes 20 bytes and BSIZE + 1 < 26) is a stored member
    whose payload length is a multiple of 256: the ISIZE the reader finds at blen - 4 is then
    13 00 01 00 = 65555, not negative, and Inflater.setInput with a negative length throws; it
    escapes as EDATA too.  bsize_neg is the same damage on a compressed member, where those four
    bytes read as a negative ISIZE (NegativeArraySizeException -> RuntimeIOException, skipped);
    it runs in position 1 only.  trunc@1 and trunc@2 give a record start, not `end`: the failed
    read leaves the stream at the window's end, the block before the cut stays current, and the
    second candidate in it decodes to a clean EOF.  So no kind gives all three outcomes; the
    family as a whole does."""
    f = File()
    beg = 0
    if uncached:
        false_magic_block(f, 300)
        beg = 1
    first = len(f.coff)
    cut = None
    for j in range(5):
        pay, offs = gc.ordinary_payload(j)
        kw = {}
        if j == where and kind == "bsize_small":
            pay, offs = _pad_to_256(j)
        if j == where:
            kw = {"crc": dict(crc_xor=1), "stored_body": dict(level=0, corrupt=True), "comp_body": dict(corrupt=True),
                  "isize_small": dict(isize=len(pay) - 1), "isize_big": dict(isize=65537),
                  "bsize_small": dict(bsize=19, level=0), "bsize_neg": dict(bsize=19), "xlen": dict(post=gc.subfield(b"XY", b"abcd")), "trunc": {}}[kind]
        p = f.add(pay, offs if not kw else (), **kw)
        if j == where and kind in ("bsize_small", "bsize_neg"):
            isz = int.from_bytes(f.parts[-1][16:20], "little", signed=True)
            assert (isz == 65555) if kind == "bsize_small" else (isz < 0), isz
        if j == where and kind == "trunc":
            cut = p + (f.pos - p) // 2
    end = cut if cut is not None else f.pos
    out, at = E_OUTCOME[kind][where]
    return Case("E", "%s@%d%s" % (kind, where, "U" if uncached else ""), f,
                [G(beg, end, out, cached=not uncached, at=None if at is None else f.coff[first + at])])


def _pad_to_256(j):
    """20 ordinary records, the last with aux bytes that make the payload a multiple of 256"""
    recs = [gc.ordinary(100 * j + i) for i in range(19)]
    n = sum(len(r) for r in recs)
    last = gc.ordinary(100 * j + 19)
    pad = -(n + len(last)) % 256
    if 0 < pad < 9:
        pad += 256
    recs.append(gc.ordinary(100 * j + 19, aux=pad) if pad else last)
    pay = b"".join(recs)
    assert len(pay) % 256 == 0
    offs, x = [], 0
    for r in recs:
        offs.append(x)
        x += len(r)
    return pay, offs


# (outcome, member the record lies in) per damaged position 0, 1, 2
_SKIP = [("rec", 1), ("rec", 2), ("rec", 3)]
E_OUTCOME = {
    "crc": _SKIP,
    "isize_small": _SKIP,
    "xlen": _SKIP,
    "stored_body": [("rec", 1), (EDATA, None), (EDATA, None)],
    "comp_body": [("rec", 1), (EDATA, None), (EDATA, None)],
    "isize_big": _SKIP,
    "bsize_small": [("rec", 1), (EDATA, None), (EDATA, None)],
    "bsize_neg": _SKIP,
    "trunc": [("end", None), ("rec", 0), ("rec", 1)],
}


# ---- F: the candidate loop ----------------------------------------------------------------------------------
def _f_case(name, payload, offs, accepted0, out_uoff=None, at_next=False, n_accepted=None, doc=""):
    f = File()
    f.add(payload, offs)
    f.chain(1, 3)
    return Case("F", name, f, [G(0, f.pos, "rec", at=f.coff[1] if at_next else 0,
                               uoff=0 if at_next else (accepted0 if out_uoff is None else out_uoff))],
                block=0, accepted0=accepted0, n_accepted=n_accepted, doc=doc)


def f_last(back):
    """The only acceptable record starts `back` bytes before the end of the inflated block: 40 is
    the last offset the loop tests, 39 is never tested."""
    rec = gc.record(name=b"abc\0"[40 - back:])
    assert len(rec) == back
    pay = b"\x80" * 200 + rec
    if back == 40:
        return _f_case("last40", pay, [200], 200, n_accepted=1)
    return _f_case("last39", pay, [], None, at_next=True, n_accepted=0)


def f_lane(k):
    """the first accepted offset k = 63, 64, 65 bytes past up: the last lane of the first step and
    the first two of the second"""
    recs, offs = gc.ordinary_payload(7, 6)
    return _f_case("lane%d" % k, b"\x80" * k + recs, [k + o for o in offs], k)


def f_probe(label, accept, **kw):
    """A probe record at offset 0 with one field at the edge of the test, true records behind it:
    accepted -> the guess is offset 0, refused -> the record behind it."""
    probe = gc.record(**kw)
    recs, offs = gc.ordinary_payload(3, 6)
    offs = [0] + [len(probe) + o for o in offs]
    return _f_case(label, probe + recs, offs, 0 if accept else len(probe))


def f_decoy():
    """A 38-byte decoy that passes the test and whose chain steps onto eight zero bytes (block_size
    0 < 32: SAMFormatException), in front of the true records."""
    recs, offs = gc.ordinary_payload(5, 6)
    return _f_case("decoy", gc.record(name=b"d\0") + bytes(8) + recs, [46 + o for o in offs], 0, out_uoff=46)


F_PROBES = ([("name0", True, dict(name=b"")), ("name255", True, dict(name=b"n" * 254 + b"\0")),
             ("lseq_max", False, dict(l_seq=0x7fffffff)), ("lseq_m1", True, dict(l_seq=-1))] +
            [("ref%d" % v, v in (-1, N_REF), dict(ref=v)) for v in (-2, -1, N_REF, N_REF + 1)] +
            [("mref%d" % v, v in (-1, N_REF), dict(mref=v)) for v in (-2, -1, N_REF, N_REF + 1)] +
            [("pos%d" % v, v == -1, dict(pos=v)) for v in (-2, -1)] +
            [("mpos%d" % v, v == -1, dict(mpos=v)) for v in (-2, -1)])


# ---- G: the chain memo -----------------------------------------------------------------------------------------
def _minimals(n, k0=0):
    return b"".join(gc.minimal(k0 + i) for i in range(n))


def _decoy_host(step):
    """A 76-byte true record whose body is a decoy that passes the test; the decoy's chain steps
    `step` bytes past the end of the host."""
    decoy = gc.record(name=b"d\0", block_size=38 - 4 + step)
    return gc.record(name=b"h\0", body=decoy)


def g_case(name, front, second, n=1700, hosts=(), out=("rec", 2), uncached=False, cut=False, chain=(">", 1024),
           doc=""):
    """Member 0: `front` bytes, then n minimal 37-byte records (hosts: {index: step} replaces a
    record by a decoy host).  `second`: how member 1 is damaged, so that every chain out of member
    0 ends the same way and the guesser walks member 0's starts one by one."""
    f = File()
    beg = 0
    if uncached:
        false_magic_block(f, 300)
        beg = 1
    first = len(f.coff)
    parts, offs, x = [front], [], len(front)
    for i in range(n):
        r = _decoy_host(hosts[i]) if i in hosts else gc.minimal(i)
        offs.append(x)
        parts.append(r)
        x += len(r)
    b0 = f.add(b"".join(parts), offs, level=1)
    if cut:
        # window exhaustion: two stored members of four large records; the window ends inside the second
        f.ordinary(1, n=4, aux=5000, level=0)
        p = f.ordinary(2, n=4, aux=5000, level=0)
        end = p + 100
    else:
        f.ordinary(1, **second)
        f.chain(2, 4)
        end = f.pos
    at = None if out[1] is None else f.coff[first + out[1]]
    return Case("G", name, f, [G(beg, end, out[0], cached=not uncached, at=at)], block=b0,
                accepted0=0 if front != b"\x80" else 1, chain=chain, chain_from=len(front), doc=doc)


# a decoy in front whose chain lands 4 bytes into the first true record (refID 0 as block_size)
_NEVER = gc.record(name=b"d\0", block_size=38 - 4 + 4)


def catalogue():
    c = []
    for n in (255, 256, 257, 600):
        c += [a_tiny(n), a_false(n)]
    c += [b_list(n) for n in (511, 512, 513)]
    c += [c_avail(65538), c_avail(65539), c_empty()]
    c += [c_edge(d, False) for d in (-1, 0, 1)] + [c_edge(d, True) for d in (-1, 0, 1, 2, 3, 4)]
    for listed in (False, True):
        phases = (0, 1, 2) if not listed else (0,)
        c += [d_prefix(p, ph, listed) for p in (b"\x1f", b"\x1f\x8b", b"\x1f\x8b\x08") for ph in phases]
        c += [d_subfield(w, listed) for w in D_SUBFIELDS]
        c.append(d_harmful(listed))
    c += [d_cut(ph) for ph in (0, 1, 2)]
    c += [e_case(k, w, u) for k in E_KINDS for w in (0, 1, 2) for u in (False, True)]
    c += [e_case(k, w, u) for k, w in E_EXTRA for u in (False, True)]
    c += [f_last(40), f_last(39), f_lane(63), f_lane(64), f_lane(65), f_decoy()]
    c += [f_probe(*p[:2], **p[2]) for p in F_PROBES]
    crc, body = dict(crc_xor=1), dict(corrupt=True)
    c += [
        g_case("long", b"", crc),
        g_case("junk_front", b"\x80", crc),
        g_case("join", b"", crc, hosts={500: 74, 1200: 74},
               doc="decoys whose chains join the true chain at its 503rd and 1203rd start"),
        g_case("never_join", _NEVER, crc, doc="the decoy's chain ends in SAMFormatException; the true chains "
               "in the CRC error of member 1"),
        g_case("never_join_edata", _NEVER, body, out=(EDATA, None),
               doc="the decoy's chain is skipped, the first true chain escapes with the inflater's error"),
        g_case("exhaust", b"", None, n=1100, cut=True, out=("rec", 1),
               doc="every chain out of member 0 runs out of bytes (ETRUNC); the guess is the second record of "
               "the stored member behind it, whose chain meets a clean EOF"),
        g_case("exhaustU", b"", None, n=40, cut=True, out=("rec", 1), uncached=True, chain=("<=", 1024),
               doc="the same with every block inflated in-lane: a chain's end lies in the scratch and is not "
               "memoised, so 40 starts (each candidate re-inflates two members in one lane; 1100 took 20 s)"),
    ]
    return c


_CAT = None


def cases():
    global _CAT
    if _CAT is None:
        _CAT = catalogue()
        names = [repr(x) for x in _CAT]
        assert len(set(names)) == len(names)
    return _CAT


def guesses():
    """[(case, guess dict)] in catalogue order"""
    return [(c, g) for c in cases() for g in c.guesses]


FAMILIES = "ABCDEFG"


# ---- BGZF-BCF ---------------------------------------------------------------------------------------------------
BCF_NAMES = ("many", "crc")
_BCF = None


def bcf_case(name):
    global _BCF
    if _BCF is None:
        _BCF = {x[0]: x for x in bcf_cases()}
    return _BCF[name]


def bcf_cases():
    """[(name, file bytes, [(beg, end)])]: a BGZF BCF cut into 320 small members (more than 256 magic
    positions in every window from the start), and one of 4000-byte members whose second has a
    wrong CRC."""
    import bcf_records
    u = bcf_records.bcf_stream(n_records=400, seed=3)
    out = []
    step = len(u) // 320 + 1
    many = b"".join(gc.block(u[i:i + step], level=0) for i in range(0, len(u), step))
    assert len(gc.magic_positions(many)) > 256
    out.append(("many", many, [(0, len(many)), (1, len(many)), (len(many) // 2, len(many))]))
    parts = [gc.block(u[i:i + 4000], crc_xor=(1 if i == 4000 else 0)) for i in range(0, len(u), 4000)]
    bad = b"".join(parts)
    p1 = len(parts[0])
    out.append(("crc", bad, [(0, len(bad)), (1, len(bad)), (p1, len(bad)), (p1 + 1, len(bad))]))
    return out


def over_64k_case():
    """A member that really inflates to more than 65536 bytes (ISIZE = 70150, right CRC) behind an
    ordinary one: legal for htsjdk, which guesses the first record of member 0; the device reader
    refuses such a member (HBAM_EUNSUPPORTED, a documented deviation), and that escapes the guess.
    Not part of the catalogue: device and oracle differ here by design.  -> (file bytes, beg, end)"""
    f = File()
    f.ordinary(0)
    pay, _ = gc.ordinary_payload(1, n=1150)
    assert len(pay) > 65536
    f.raw(gc.block(pay))
    f.chain(2, 3)
    return f.bytes(), 0, f.pos
