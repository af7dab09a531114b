"""Crafted record streams for the record-chain walk (k_block_entry / k_block_walk / k_stitch_check /
k_chain_fix_par / k_chain_fix in csrc/hbam_kernels.hip, instantiated with BamFmt and BcfFmt), and a
host model of that walk.

Builders: bgzf_pack_at cuts BGZF members at chosen stream offsets (and inserts empty members);
BamStream / BcfStream lay out a header and records and know every record's stream offset.  Both
can add a "host" record with an opaque payload (BAM: a B:C aux array; BCF: an INFO character
string with an extended int32 count) into which chains of well-formed decoy records are placed at
chosen stream offsets, so a block that starts on one gets a wrong entry guess.

Model: model() restates the entry finder, the walk and the stitch check in plain Python for both
formats and returns, per block, the first entry guess, the first exit, the stitch mark, and the
chain after sequential repair.  It is an instrument: every case asserts with it that it has the
structure it claims (a wrong guess, an unmarked-but-wrong block, no entry at all, many run heads),
so a case that stops reaching the repair fails on the CPU instead of passing vacuously on the GPU.
"""
import struct
import zlib

import numpy as np

import bcf_records
import f4_records

NO_ENTRY = (1 << 64) - 1
CHAIN_STOP = (1 << 64) - 2
WALK_CAP = 1880            # csrc/hbam_internal.h
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_BLOCK = 65536          # the largest ISIZE the decoder inflates (k_isize32)


# ---- BGZF with chosen cuts ------------------------------------------------------------------------
def bgzf_member(chunk, level=5):
    chunk = bytes(chunk)
    assert len(chunk) <= MAX_BLOCK
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    cd = co.compress(chunk) + co.flush()
    assert len(cd) + 26 <= 65536, "member too large: lower-entropy payload or a smaller block"
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cd) + 25) + cd +
            struct.pack("<II", zlib.crc32(chunk), len(chunk)))


def bgzf_pack_at(u, cuts, empties=(), level=5):
    """BGZF members of the stream u cut at the stream offsets `cuts` (member k holds
    u[cuts[k-1]:cuts[k]]); an empty member goes before each member index in `empties` (index
    len(cuts) + 1: before the EOF block, an index listed twice: two of them); the EOF block ends
    the file."""
    cuts = sorted(set(int(c) for c in cuts))
    assert all(0 < c < len(u) for c in cuts), "cuts lie strictly inside the stream"
    edges = [0] + cuts + [len(u)]
    empties = sorted(empties)
    assert all(0 <= e <= len(edges) - 1 for e in empties)
    out = []
    for k in range(len(edges) - 1):
        out += [BGZF_EOF] * empties.count(k)
        out.append(bgzf_member(u[edges[k]:edges[k + 1]], level))
    out += [BGZF_EOF] * empties.count(len(edges) - 1)
    out.append(BGZF_EOF)
    return b"".join(out)


def bgzf_layout(comp):
    """(coff list, uoff list with the total at its end) of every member, the EOF block included:
    the block table the device walks."""
    coff, uoff, p, n = [], [0], 0, 0
    while p < len(comp):
        bs = struct.unpack_from("<H", comp, p + 16)[0] + 1
        coff.append(p)
        n += struct.unpack_from("<I", comp, p + bs - 4)[0]
        uoff.append(n)
        p += bs
    return coff, uoff


def even_cuts(n, block):
    return list(range(block, n, block))


# ---- record pools (true records reused with a patched position) --------------------------------------
_POOL = {}


def _bam_pool():
    if "bam" not in _POOL:
        rng = np.random.default_rng(21)
        _POOL["bam"] = [f4_records.record(b"read%03d" % i + b"x" * int(rng.integers(0, 9)), flag=int(rng.integers(0, 2)) * 16,
                                          ref=int(rng.integers(0, 4)), pos=0, cigar=((20 + i % 7, 0),), l_seq=20 + i % 7,
                                          aux=f4_records.aux_int("NM", "C", i % 200), seed=i) for i in range(64)]
    return _POOL["bam"]


def _bcf_pool():
    if "bcf" not in _POOL:
        rng = np.random.default_rng(22)
        _POOL["bcf"] = [bcf_records.record(rng, int(rng.integers(0, 25)), 0, 3, long_id=(i % 13 == 5)) for i in range(96)]
    return _POOL["bcf"]


class _Stream:
    """Header + records; starts[i] is record i's stream offset."""

    def __init__(self, header):
        self.parts = [header]
        self.pos = len(header)
        self.header_len = len(header)
        self.starts = []
        self._k = 0
        self._patches = []

    def add(self, rec):
        self.starts.append(self.pos)
        self.parts.append(bytes(rec))
        self.pos += len(rec)
        return self.starts[-1]

    def raw(self, b):
        """bytes that are no record of the builder's (a cut-short record, trailing garbage)"""
        self.parts.append(bytes(b))
        self.pos += len(b)

    def fill_to(self, offset):
        """true records until the next one would start at or after `offset`"""
        while self.pos < offset:
            self.add_true()
        return self.pos

    def add_trues(self, n):
        for _ in range(n):
            self.add_true()

    def patch(self, off, b):
        """overwrite bytes already laid out (a decoy whose size depends on what follows it)"""
        assert off + len(b) <= self.pos
        self._patches.append((off, bytes(b)))

    def bytes(self):
        u = bytearray(b"".join(self.parts))
        for off, b in self._patches:
            u[off:off + len(b)] = b
        return bytes(u)

    # a host record whose payload begins at payload_start() when added now
    def payload_start(self):
        return self.pos + self.HOST_PREFIX

    def add_host_with(self, payload_len, decoys=()):
        """Host record with a zero payload of payload_len bytes into which each (stream offset,
        bytes) of `decoys` is copied."""
        p0 = self.payload_start()
        pay = bytearray(payload_len)
        for off, b in decoys:
            assert p0 <= off and off + len(b) <= p0 + payload_len, (p0, off, len(b), payload_len)
            pay[off - p0:off - p0 + len(b)] = b
        return self.add_host(bytes(pay))


# ---- BAM ------------------------------------------------------------------------------------------------
N_REF = 4


def bam_header(n_ref=N_REF):
    refs = [(b"chr%d" % (i + 1), 1000000 + i) for i in range(n_ref)]
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", n_ref)]
    for nm, ln in refs:
        out += [struct.pack("<i", len(nm) + 1), nm, b"\0", struct.pack("<i", ln)]
    return b"".join(out)


def bam_decoy(size=38, pos=7, ref=0):
    """A well-formed 38-byte record (name "d", no CIGAR, no bases) whose block_size field claims
    `size` bytes in all: passes rec_plausible, and its chain step is size bytes long."""
    assert size >= 38
    r = bytearray(f4_records.record(b"d", flag=4, ref=ref, pos=pos, cigar=(), l_seq=0))
    assert len(r) == 38
    struct.pack_into("<i", r, 0, size - 4)
    return bytes(r)


def bam_min_record(pos, ref=0):
    """36 bytes: block_size 32, l_read_name 0, no CIGAR, no bases."""
    return struct.pack("<iiiBBHHHiiii", 32, ref, pos, 0, 0, 4680, 0, 4, 0, -1, -1, 0)


def bam_bad_record(block_size=20):
    return struct.pack("<i", block_size) + b"\x01" * max(block_size, 0)


class BamStream(_Stream):
    HOST_PREFIX = 4 + 32 + 5 + 3 + 1 + 4  # block_size, fixed, "host\0", XB B, C, count

    def __init__(self):
        super().__init__(bam_header())

    def add_true(self):
        r = bytearray(_bam_pool()[self._k % 64])
        struct.pack_into("<i", r, 8, 1000 + 3 * self._k)
        self._k += 1
        return self.add(r)

    def add_host(self, payload):
        p0 = self.payload_start()
        s = self.add(f4_records.record(b"host", flag=4, ref=-1, pos=-1, cigar=(), l_seq=0,
                                       aux=b"XBBC" + struct.pack("<I", len(payload)) + payload))
        assert s + self.HOST_PREFIX == p0
        return s


# ---- BCF ------------------------------------------------------------------------------------------------
BCF_H = dict(n_contig=25, n_sample=3, n_dict=6)


def bcf_header():
    text = bcf_records.header_text().encode() + b"\0"
    return b"BCF\x02\x01" + struct.pack("<I", len(text)) + text


def bcf_site_fixed(chrom, pos, n_allele=1, n_info=0, n_fmt=0, n_sample=3, rlen=1, qual=30.0):
    return (struct.pack("<iiif", chrom, pos, rlen, qual) +
            struct.pack("<iI", n_allele << 16 | n_info, (n_fmt & 0xff) << 24 | n_sample))


def bcf_min_record(pos, chrom=0, l_indiv=0):
    """35 bytes + l_indiv: l_shared 27 = the 24 fixed bytes, an empty ID (07), one empty allele
    (07) and an empty FILTER (00).  The genotype block is opaque (n_fmt 0)."""
    return struct.pack("<ii", 27, l_indiv) + bcf_site_fixed(chrom, pos) + b"\x07\x07\x00" + bytes(l_indiv)


def bcf_decoy(size=44, pos=7, chrom=0):
    """A well-formed record (passes bcf_pred and BcfFmt::plausible) of 43 bytes whose l_indiv
    claims the rest of `size`: ID "d", allele "A", FILTER empty, l_shared 30."""
    assert size >= 43
    shared = bcf_site_fixed(chrom, pos) + b"\x17d" + b"\x17A" + b"\x00" + b"\x00"  # one trailing byte inside l_shared
    assert len(shared) == 30
    return struct.pack("<ii", 30, size - 38) + shared + bytes(5)


def bcf_bad_record(l_shared=26, l_indiv=0, pos=5):
    body = (bcf_site_fixed(0, pos) + b"\x07\x17A\x00" + bytes(64))[:max(l_shared, 0)]
    return struct.pack("<ii", l_shared, l_indiv) + body + bytes(max(l_indiv, 0))


class BcfStream(_Stream):
    def __init__(self):
        super().__init__(bcf_header())
        self._host_head = (bcf_site_fixed(1, 0, n_allele=2, n_info=1) + bcf_records.typed_str("host") +
                           bcf_records.typed_str("A") + bcf_records.typed_str("C") + bcf_records.typed_ints([0]) +
                           bcf_records.typed_int(bcf_records.DICT["DP"]) + b"\xf7\x13")
        self.HOST_PREFIX = 8 + len(self._host_head) + 4

    def add_true(self):
        r = bytearray(_bcf_pool()[self._k % 96])
        struct.pack_into("<i", r, 12, 100 + 3 * self._k)
        self._k += 1
        return self.add(r)

    def add_host(self, payload):
        shared = self._host_head + struct.pack("<i", len(payload)) + payload
        return self.add(struct.pack("<ii", len(shared), 0) + shared)


def decoy_chain(fmt, sizes, stop=False):
    """Contiguous decoy records of the given chain-step sizes.  The last one's size may reach past
    its own bytes (the chain then leaves at start + sum(sizes)); stop=True appends bytes at which
    the chain stops (a size field no record can have)."""
    mk, base = (bam_decoy, 38) if fmt == "bam" else (bcf_decoy, 43)
    out = b""
    for i, s in enumerate(sizes):
        d = mk(s, pos=11 + i)
        out += d if i == len(sizes) - 1 else d + bytes(s - len(d))
    if stop:
        assert sizes[-1] == base
        out += bytes(8)  # block_size 0 / l_shared 0
    return out


# ---- the model -------------------------------------------------------------------------------------------
def _le32_all(a):
    """int32 little-endian value at every offset of the byte array (the last 3 padded with 0)"""
    p = np.concatenate([a, np.zeros(3, np.uint8)]).astype(np.uint32)
    return (p[:-3] | p[1:-2] << 8 | p[2:-1] << 16 | p[3:] << 24).view(np.int32)


class BamModel:
    """BamFmt: rec_plausible and the chain step r + 4 + block_size."""

    def __init__(self, u, n_ref=N_REF):
        self.u = bytes(u) + bytes(64)  # the device buffer has slack behind the stream
        self.n_ref = n_ref
        a = np.frombuffer(bytes(u), np.uint8)
        w = _le32_all(a)
        l12 = np.concatenate([a[12:], np.zeros(12, np.uint8)])
        self._cand = (w >= 32) & (l12 != 0)  # two conjuncts of plausible(): a prefilter, nothing more

    def plausible(self, x, hard_end):
        if x + 36 > hard_end:
            return False
        bs, rid, pos, L = struct.unpack_from("<iiiB", self.u, x)
        ncig, = struct.unpack_from("<H", self.u, x + 16)
        lseq, nid, npos = struct.unpack_from("<iii", self.u, x + 20)
        n = self.n_ref
        if bs < 32 or rid < -1 or rid >= n or nid < -1 or nid >= n or pos < -1 or npos < -1:
            return False
        if L == 0 or lseq < 0:
            return False
        if bs < 32 + L + 4 * ncig + lseq + (lseq + 1) // 2:
            return False
        if x + 36 + L > hard_end:
            return False
        return self.u[x + 36 + L - 1] == 0

    def next(self, r, hard_end):
        if r + 4 > hard_end:
            return CHAIN_STOP
        bs, = struct.unpack_from("<i", self.u, r)
        if bs < 32:
            return CHAIN_STOP
        return r + 4 + bs


class BcfModel:
    """BcfFmt: bcf_pred (BCFSplitGuesser.guessNextBCFPos' test) plus l_shared >= 27 and
    l_indiv >= 0, and the chain step r + 8 + l_shared + l_indiv."""

    def __init__(self, u, h=BCF_H):
        self.u = bytes(u) + bytes(64)
        self.n_contig, self.n_sample = h["n_contig"], h["n_sample"]
        a = np.frombuffer(bytes(u), np.uint8)
        w = _le32_all(a)
        b28 = np.concatenate([a[28:], np.zeros(28, np.uint8)])
        b32 = np.concatenate([a[32:], np.zeros(32, np.uint8)])
        self._cand = (w >= 27) & (b28 == (self.n_sample & 0xff)) & ((b32 & 15) == 7)

    def pred(self, x):
        u = self.u
        shared, indiv = struct.unpack_from("<II", u, x)
        if shared + indiv < 33:
            return False
        chrom, pos = struct.unpack_from("<ii", u, x + 8)
        if chrom < 0 or chrom >= self.n_contig or pos < 0:
            return False
        ai, = struct.unpack_from("<i", u, x + 24)
        if (ai >> 16) < 0 or (ai & 0xffff) < 0:
            return False
        if u[x + 28] != self.n_sample:
            return False
        idt = u[x + 32]
        if idt & 0x0f != 7:
            return False
        if idt & 0xf0 == 0xf0:
            t = u[x + 33] & 0x0f
            if t == 1:
                id_len = u[x + 34]
            elif t == 2:
                id_len, = struct.unpack_from("<H", u, x + 34)
            elif t == 3:
                id_len, = struct.unpack_from("<I", u, x + 34)
            else:
                return False
            if id_len < 15 or id_len > shared - (32 + (ai >> 16) + (ai & 0xffff) * 2):
                return False
        return True

    def plausible(self, x, hard_end):
        if x + 38 > hard_end:
            return False
        if not self.pred(x):
            return False
        ls, li = struct.unpack_from("<ii", self.u, x)
        return ls >= 27 and li >= 0

    def next(self, r, hard_end):
        if r + 8 > hard_end:
            return CHAIN_STOP
        ls, li = struct.unpack_from("<ii", self.u, r)
        if ls < 27 or li < 0:
            return CHAIN_STOP
        return r + 8 + ls + li


def _entry(f, b0, b1, hard_end):
    """k_block_entry for one block: the first offset in [b0, b1) that is plausible and whose next
    three hops are plausible or end exactly at hard_end."""
    for x in np.flatnonzero(f._cand[b0:min(b1, len(f._cand))]) + b0:
        x = int(x)
        if not f.plausible(x, hard_end):
            continue
        r, ok = x, True
        for _ in range(3):
            r = f.next(r, hard_end)
            if r == hard_end:
                break
            ok = r != CHAIN_STOP and f.plausible(r, hard_end)
            if not ok:
                break
        if ok:
            return x
    return NO_ENTRY


def _walk(f, b0, b1, r, hard_end):
    """walk_one: (record starts in [b0, b1), exit)"""
    if r in (NO_ENTRY, CHAIN_STOP):
        return [], r
    out = []
    while r < b1:
        out.append(r)
        r = f.next(r, hard_end)
        if r == CHAIN_STOP:
            break
    return out, r


def model(f, uoff, r0, hard_end=None):
    """uoff: block starts of the walked blocks plus the end (block 0 holds r0).  Returns dict:
    guess[b] first entry, exit0[b] first exit, marked[b] (first stitch check), entry[b] / chain
    after sequential repair, count[b], wrong[b] (guess != final entry), heads (run heads the
    parallel repair gets)."""
    nb = len(uoff) - 1
    if hard_end is None:
        hard_end = uoff[-1]
    guess = [r0] + [_entry(f, uoff[b], uoff[b + 1], hard_end) for b in range(1, nb)]
    cur = [_walk(f, uoff[b], uoff[b + 1], guess[b], hard_end) for b in range(nb)]
    exit0 = [e for _, e in cur]
    count0 = [len(s) for s, _ in cur]
    marked = [False] + [guess[b] != exit0[b - 1] for b in range(1, nb)]
    entry = list(guess)
    for b in range(1, nb):  # k_chain_fix
        if entry[b] != cur[b - 1][1]:
            entry[b] = cur[b - 1][1]
            cur[b] = _walk(f, uoff[b], uoff[b + 1], entry[b], hard_end)
    chain = [r for s, _ in cur for r in s]
    return dict(guess=guess, exit0=exit0, count0=count0, marked=marked, entry=entry, chain=chain,
                count=[len(s) for s, _ in cur], exit=[e for _, e in cur],
                wrong=[guess[b] != entry[b] for b in range(nb)],
                heads=[b for b in range(1, nb) if marked[b] and not marked[b - 1]])


def plain_uoff(n, first=0):
    """64 KiB segments of a plain BCF window of n bytes, from the segment holding `first`"""
    nseg = (n + 65535) >> 16
    return [min(i << 16, n) for i in range(first >> 16, nseg + 1)]
