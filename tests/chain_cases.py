"""The crafted chain-walk cases (a-j) shared by the host model tests (test_chain_model.py) and the
device tests (test_chain_gpu.py).  Each case is a Case: the file, the split to read, the block
table the device walks, and the decoy offsets; built once per process."""
import functools

import chain_craft as cc

PLAIN_STEP = 65536  # plain BCF: the walk's blocks are 64 KiB segments from the window start
BGZF_STEP = 4000    # BGZF: cuts wherever the case wants them


class Case:
    def __init__(self, name, fmt, kind, s, cuts=(), empties=(), decoys=(), sblk=0, start_off=None, u=None):
        self.name, self.fmt, self.kind = name, fmt, kind
        self.u = s.bytes() if u is None else u
        self.header_len = s.header_len
        self.starts = list(s.starts)
        self.decoys = list(decoys)
        self.bgzf = kind == "bgzf"
        if self.bgzf:
            self.cuts = sorted(c for c in set(cuts) if 0 < c < len(self.u))
            self.data = cc.bgzf_pack_at(self.u, self.cuts, empties)
            self.coff, uoff = cc.bgzf_layout(self.data)
            off = s.header_len - uoff[sblk] if start_off is None else start_off
            self.v_start = self.coff[sblk] << 16 | off
            self.v_end = len(self.data) << 16 | 0xffff
            self.uoff = uoff[sblk:]
            self.r0 = uoff[sblk] + off
        else:
            self.data = self.u
            self.v_start, self.v_end = 0, len(self.u)
            self.r0 = s.header_len
            self.uoff = cc.plain_uoff(len(self.u), self.r0)
        self.h = dict(cc.BCF_H, header_len=s.header_len, bgzf=self.bgzf)

    def fmt_model(self):
        return cc.BamModel(self.u) if self.fmt == "bam" else cc.BcfModel(self.u)

    @functools.lru_cache(None)
    def model(self):
        return cc.model(self.fmt_model(), self.uoff, self.r0, len(self.u))

    def block_of(self, off):
        return max(b for b in range(len(self.uoff) - 1) if self.uoff[b] <= off)


def _stream(fmt):
    return cc.BamStream() if fmt == "bam" else cc.BcfStream()


def _base(fmt):
    return 38 if fmt == "bam" else 43


def _step(kind):
    return PLAIN_STEP if kind == "plain" else BGZF_STEP


def _cuts(kind, n=12):
    return [_step(kind) * k for k in range(1, n)]


VARIANTS = [("bam", "bgzf"), ("bcf", "bgzf"), ("bcf", "plain")]


LEAD_CUT = 2000  # lead=True (BGZF): one more cut before the first, so the decoy's block is not the second


@functools.lru_cache(None)
def case_a(fmt, kind, lead=False):
    """A decoy chain at a block start that stops inside the block; the true record comes later."""
    c = _cuts(kind)
    s = _stream(fmt)
    s.fill_to(c[0] - 1500)
    p0 = s.payload_start()
    s.add_host_with(c[0] + 1500 - p0, [(c[0], cc.decoy_chain(fmt, [_base(fmt)] * 5, stop=True))])
    s.fill_to(c[2] + 1000)
    return Case("a", fmt, kind, s, c + [LEAD_CUT] * lead, decoys=[c[0]])


@functools.lru_cache(None)
def case_b(fmt, kind):
    """One record spanning five blocks: the middle ones have no entry at all.  Minimum-size records
    (which the entry predicate rejects) follow it, so the block it ends in guesses a later record:
    the records in between are framed only if the repair carries block 0's exit across the blocks
    without an entry."""
    c = _cuts(kind)
    s = _stream(fmt)
    s.fill_to(c[0] - 1500)
    p0 = s.payload_start()
    s.add_host_with(c[3] + 500 - p0)
    for i in range(8):
        s.add(_min_rec(fmt)(i))
    s.fill_to(c[4] + 500)
    case = Case("b", fmt, kind, s, c)
    case.host_end = c[3] + 500
    return case


def _consistent(fmt, kind, stale, lead=False):
    """c: decoys laid contiguously over the cut c[1], so block 2's guess is block 1's false exit;
    the false chain then lands on a true record start of block 3.  d (stale): it lands instead on
    a second decoy chain inside block 3, whose guess is a third chain at its start."""
    c = _cuts(kind)
    base = _base(fmt)
    k = (c[1] - c[0]) // base + 6  # past the cut, then five more

    def build(last):
        s = _stream(fmt)
        s.fill_to(c[0] - 1500)
        p0 = s.payload_start()
        dec = [(c[0], cc.decoy_chain(fmt, [base] * (k - 1) + [last]))]
        end = c[1] + 2500
        if stale:
            end = c[2] + 2500
            dec += [(c[2], cc.decoy_chain(fmt, [base] * 5, stop=True)),
                    (c[2] + 600, cc.decoy_chain(fmt, [base] * 5, stop=True))]
        s.add_host_with(end - p0, dec)
        s.fill_to(c[3] + 1000)
        return s

    s = build(base)
    target = c[2] + 600 if stale else min(x for x in s.starts if x >= c[2])
    last_start = c[0] + base * (k - 1)
    assert c[1] < last_start < c[1] + 2000
    s = build(target - last_start)
    e = c[0] + base * ((c[1] - c[0] + base - 1) // base)  # the first decoy start at or after the cut
    return Case("d" if stale else "c", fmt, kind, s, c + [LEAD_CUT] * lead,
                decoys=[c[0], e] + ([c[2], c[2] + 600] if stale else []))


@functools.lru_cache(None)
def case_c(fmt, kind, lead=False):
    return _consistent(fmt, kind, False, lead)


@functools.lru_cache(None)
def case_d(fmt, kind):
    return _consistent(fmt, kind, True)


@functools.lru_cache(None)
def case_e(fmt):
    """More than 200 blocks of 512-1024 bytes, every second one starting on a decoy chain.  Four
    chains in five land on the next block's (true) guess, so that block is unmarked and the decoy
    block heads a run of its own; every fifth stops, so its run goes on through the next blocks.
    More than 64 run heads for k_chain_fix_par, over several workgroups."""
    s = _stream(fmt)
    base = _base(fmt)
    s.add_trues(4)
    cuts, decoys = [], []
    for i in range(110):
        a = s.payload_start() + 100
        s.add_host_with(420)
        cuts.append(a)
        decoys.append(a)
        while s.pos < a + 530:
            s.add_true()
        b = s.add_true() + 1
        cuts.append(b)
        while s.pos + s.HOST_PREFIX + 100 < b + 530:
            s.add_true()
        nxt = min(x for x in s.starts if x >= b)  # the guess of the block cut at b
        if i % 5 == 4:
            s.patch(a, cc.decoy_chain(fmt, [base] * 4, stop=True))
        else:
            s.patch(a, cc.decoy_chain(fmt, [base] * 3 + [nxt - a - 3 * base]))
    s.add_trues(3)
    return Case("e", fmt, "bgzf", s, cuts, decoys=decoys)


@functools.lru_cache(None)
def case_f(fmt, kind, hops):
    """A decoy chain at a block start whose hop number `hops` lands exactly on the end of the
    stream: the chain check accepts it without looking further."""
    c = _cuts(kind)
    base = _base(fmt)
    s = _stream(fmt)
    s.fill_to(c[0] - 1500)
    p0 = s.payload_start()
    end = c[0] + 3000
    s.add_host_with(end - p0, [(c[0], cc.decoy_chain(fmt, [base] * (hops - 1) + [end - c[0] - base * (hops - 1)]))])
    return Case("f%d" % hops, fmt, kind, s, c, decoys=[c[0]])


@functools.lru_cache(None)
def case_f_cut(fmt, kind, missing):
    """True records; the last `missing` bytes of the stream are not there."""
    s = _stream(fmt)
    s.add_trues(70)
    u = s.bytes()
    assert s.pos - s.starts[-1] > 37
    return Case("fcut%d" % missing, fmt, kind, s, even_cuts_for(kind, len(u) - missing, 1500), u=u[:len(u) - missing])


def even_cuts_for(kind, n, block):
    return cc.even_cuts(n, block) if kind == "bgzf" else ()


def _min_rec(fmt):
    return cc.bam_min_record if fmt == "bam" else cc.bcf_min_record


def _min_size(fmt):
    return 36 if fmt == "bam" else 35


@functools.lru_cache(None)
def case_g_plain():
    """BCF plain: four segments of 35-byte records (the predicate rejects every one of them)."""
    s = cc.BcfStream()
    n = (4 * 65536 - s.header_len) // 35
    for i in range(n):
        s.add(cc.bcf_min_record(i))
    return Case("g", "bcf", "plain", s)


@functools.lru_cache(None)
def case_g_full(fmt):
    """BGZF: the header in a block of its own, then blocks of 65536 bytes (the largest the decoder
    inflates) of minimum-size records."""
    s = _stream(fmt)
    size = _min_size(fmt)
    for i in range((3 * 65536 + 30000) // size):
        s.add(_min_rec(fmt)(i))
    h = s.header_len
    cuts = [h] + list(range(h + 65536, s.pos, 65536))
    return Case("gfull", fmt, "bgzf", s, cuts, sblk=1, start_off=0)


def g_counts(fmt):
    full = 65536 // _min_size(fmt)
    return list(range(1, 18)) + list(range(full - 7, full + 1))


@functools.lru_cache(None)
def case_g_counts(fmt):
    """BGZF blocks cut at record starts so that the blocks' start counts are g_counts(fmt): every
    n % 8 below 8, above 8, and next to a full block."""
    s = _stream(fmt)
    size = _min_size(fmt)
    for i in range(sum(g_counts(fmt)) + 5):
        s.add(_min_rec(fmt)(i))
    h = s.header_len
    cuts, p = [h], h
    for n in g_counts(fmt):
        p += n * size
        cuts.append(p)
    return Case("gcounts", fmt, "bgzf", s, cuts, sblk=1, start_off=0)


@functools.lru_cache(None)
def case_h_bgzf(fmt):
    """A cut at each byte of a record's size field (every tenth record one byte further), at a
    record start and one byte before one."""
    s = _stream(fmt)
    s.add_trues(130)
    nb = 4 if fmt == "bam" else 8
    cuts = [s.starts[10 * (k + 2)] + k for k in range(-1, nb)]
    return Case("h", fmt, "bgzf", s, cuts)


@functools.lru_cache(None)
def case_h_plain(k):
    """BCF plain: the segment boundary k bytes into a record (k = -1: one byte before it)."""
    s = cc.BcfStream()
    s.add_trues(40)
    nxt = len(cc._bcf_pool()[40])  # the true record that follows the host
    # host sized so that the second true record after it starts at 65536 - k
    s.add_host_with(65536 - k - nxt - s.payload_start())
    s.add_trues(40)
    assert s.starts[42] == 65536 - k, (s.starts[42], k)
    return Case("h%d" % k, "bcf", "plain", s)


@functools.lru_cache(None)
def case_i(fmt, kind, what):
    """A record that cannot be framed (BAM block_size < 32; BCF l_shared < 27 or l_indiv < 0) in
    a block that starts on a decoy, so the true chain reaches it only through the repair; good
    records (with perfectly good entry guesses) in the blocks after it."""
    c = _cuts(kind)
    s = _stream(fmt)
    s.fill_to(c[0] - 1500)
    p0 = s.payload_start()
    s.add_host_with(c[0] + 1500 - p0, [(c[0], cc.decoy_chain(fmt, [_base(fmt)] * 5, stop=True))])
    s.add_trues(3)
    bad = s.pos
    if fmt == "bam":
        s.raw(cc.bam_bad_record(20))
    elif what == "shared":
        s.raw(cc.bcf_bad_record(l_shared=26))
    else:
        s.raw(cc.bcf_bad_record(l_shared=28, l_indiv=-3))
    n_before = len(s.starts)
    s.fill_to(c[2] + 1000)
    case = Case("i_" + what, fmt, kind, s, c, decoys=[c[0]])
    case.bad, case.n_before = bad, n_before
    return case


I_VARIANTS = [("bam", "bgzf", "size"), ("bcf", "bgzf", "shared"), ("bcf", "bgzf", "indiv"),
              ("bcf", "plain", "shared"), ("bcf", "plain", "indiv")]
