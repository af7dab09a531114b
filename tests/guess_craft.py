"""Crafted guess windows for the split guessers (csrc/hbam_guess.hip: k_guess_cands / k_guess_clamp /
k_guess_cand_blocks, k_guess_bam_wave, k_guess_bgzf) and a static description of each window.

Builders: block() writes one BGZF member with a chosen deflate level (0 = one stored deflate block),
extra gzip subfields before / after `BC`, and every kind of damage the reader distinguishes (wrong
CRC, ISIZE, BSIZE, a corrupt deflate body); record() writes a BAM record with every length and id
field free; false_magic() / harmful_magic() are byte strings the magic scan trips over; File lays
members and raw bytes out and knows the virtual offset of every true record.

describe() is computed from the bytes alone (zlib + numpy; neither the oracle nor the device): the
window length, first_end, the magic counts that decide the block cache (GC_CAP = 256) and the listed
scan (GW_MAG = 512), and, for a named block, the offsets guessNextBAMPos accepts and the number of
record starts on the chain from an offset (GW_MEMO = 1024).  It is an instrument: test_guess_model.py
asserts with it that every case of guess_cases.py reaches the path it claims, so a case that stops
doing so fails on the CPU instead of passing vacuously on the GPU.
"""
import struct
import zlib

import numpy as np

MAGIC = b"\x1f\x8b\x08\x04"
GC_CAP, GW_MAG, GW_MEMO = 256, 512, 1024       # csrc/hbam_guess.hip
MAX_BYTES_READ = 3 * 0xffff + 0xfffe           # BAMSplitGuesser.java:103
N_REF = 4


# ---- BGZF members ---------------------------------------------------------------------------------
def stored(payload):
    """one final stored deflate block"""
    assert len(payload) <= 0xffff
    return b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + bytes(payload)


def subfield(si, data):
    return bytes(si) + struct.pack("<H", len(data)) + bytes(data)


def block(payload, level=6, pre=b"", post=b"", crc_xor=0, isize=None, bsize=None, corrupt=False, xlen=None):
    """One BGZF member of `payload`.  level 0: a stored deflate block.  pre / post: raw bytes of the
    extra field before / after the BC subfield (XLEN counts them unless `xlen` is given).  crc_xor:
    xor-ed into the CRC.  isize / bsize: the value written instead of the true one.  corrupt: the
    deflate body is damaged so that inflate itself fails (stored: LEN / NLEN disagree; compressed:
    the reserved block type 3)."""
    payload = bytes(payload)
    if level == 0:
        cd = stored(payload)
        if corrupt:
            cd = cd[:3] + bytes([cd[3] ^ 0x10]) + cd[4:]
    else:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        cd = co.compress(payload) + co.flush()
        if corrupt:
            cd = bytes([cd[0] | 0x06]) + cd[1:]
    x = len(pre) + 6 + len(post) if xlen is None else xlen
    total = 12 + len(pre) + 6 + len(post) + len(cd) + 8
    assert total <= 65536, total
    return (MAGIC + b"\0\0\0\0\0\xff" + struct.pack("<H", x) + bytes(pre) + b"BC\x02\x00" +
            struct.pack("<H", (total - 1 if bsize is None else bsize) & 0xffff) + bytes(post) + cd +
            struct.pack("<II", zlib.crc32(payload) ^ crc_xor, len(payload) if isize is None else isize))


def false_magic():
    """Harmless: the magic and eight zero bytes read as a header with XLEN = 0; the scan moves on."""
    return MAGIC + bytes(8)


def harmful_magic():
    """A header whose first subfield claims 65535 bytes: guessNextBGZFPos' seek leaves the window
    (IOException -> null) unless 65551 more bytes follow."""
    return MAGIC + bytes(6) + struct.pack("<H", 8) + b"XY\xff\xff" + bytes(4)


# ---- BAM records -----------------------------------------------------------------------------------
def record(ref=0, pos=100, name=b"r\0", n_cigar=0, l_seq=0, mref=-1, mpos=-1, body=b"", block_size=None,
           name_len=None, flag=4):
    """block_size .. tlen, then `name` and `body` verbatim.  l_read_name, n_cigar, l_seq and block_size
    are written as given whatever bytes follow."""
    nl = len(name) if name_len is None else name_len
    bs = 32 + len(name) + len(body) if block_size is None else block_size
    return (struct.pack("<iiiBBHHHiiii", bs, ref, pos, nl, 0, 4680, n_cigar, flag, l_seq, mref, mpos, 0) +
            bytes(name) + bytes(body))


def ordinary(i, aux=0):
    """A mapped record: 6-byte name, one CIGAR op, 10 bases, `aux` more bytes."""
    body = struct.pack("<I", 10 << 4) + bytes([0x12, 0x48, 0x21, 0x84, 0x11]) + bytes([30 + i % 7] * 10)
    if aux:
        body += b"XBBC" + struct.pack("<I", aux - 8) + bytes([0x41 + i % 26]) * (aux - 8)
    return record(ref=1 + i % 3, pos=1000 + 3 * i, name=b"q%04d\0" % (i % 10000), n_cigar=1, l_seq=10,
                  mref=i % N_REF, mpos=1200 + 3 * i, body=body, flag=99)


def minimal(i):
    """37 bytes: a one-byte name (the NUL), nothing else."""
    return record(ref=0, pos=i, name=b"\0")


def ordinary_payload(k, n=20, aux=0):
    """n ordinary records -> (payload, record offsets)"""
    recs = [ordinary(100 * k + j, aux) for j in range(n)]
    offs = np.cumsum([0] + [len(r) for r in recs])[:-1]
    return b"".join(recs), [int(o) for o in offs]


class File:
    """Members and raw bytes in file order.  starts: virtual offsets of every true record (a record
    the builder laid out whole inside one member's payload)."""

    def __init__(self):
        self.parts, self.pos, self.starts, self.coff = [], 0, set(), []

    def add(self, payload, offs=(), **kw):
        """a member of `payload` whose true records start at `offs`; returns its file offset"""
        p = self.pos
        self.raw(block(payload, **kw))
        self.coff.append(p)
        self.starts.update(p << 16 | o for o in offs)
        return p

    def ordinary(self, k, n=20, aux=0, **kw):
        pay, offs = ordinary_payload(k, n, aux)
        return self.add(pay, offs, **kw)

    def chain(self, k0, n_blocks, **kw):
        return [self.ordinary(k0 + j, **kw) for j in range(n_blocks)]

    def filler(self, until, k0=900):
        """stored members of ordinary records until the file holds at least `until` bytes"""
        while self.pos < until:
            self.ordinary(k0, n=300, aux=40, level=0)
            k0 += 1

    def raw(self, b):
        self.parts.append(bytes(b))
        self.pos += len(b)

    def junk(self, n):
        """bytes no scan rule reacts to"""
        self.raw(b"\xaa" * n)

    def junk_to(self, offset):
        assert offset >= self.pos, (offset, self.pos)
        self.junk(offset - self.pos)

    def bytes(self):
        return b"".join(self.parts)


# ---- the static description --------------------------------------------------------------------------
def magic_positions(a):
    a = np.frombuffer(bytes(a), np.uint8)
    if len(a) < 4:
        return np.zeros(0, np.int64)
    return np.flatnonzero((a[:-3] == 0x1f) & (a[1:-2] == 0x8b) & (a[2:-1] == 8) & (a[3:] == 4))


def scan_reads(w, p, end):
    """The reads of guessNextBGZFPos' magic scan (BAMSplitGuesser.java:224-242) over the window w
    from p: [(position, bytes read, buf[0:4] after the read)], up to the read that matches the
    magic or the advance that reaches `end`.  A short read leaves the rest of buf as it was."""
    buf, out = bytearray(MAGIC), []
    while p <= len(w):
        got = bytes(w[p:p + 4])
        buf[:len(got)] = got
        out.append((p, len(got), bytes(buf)))
        n = int.from_bytes(buf, "little")
        if n == 0x04088b1f:
            break
        p += 1 if n >> 8 == 0x088b1f else 2 if n >> 16 == 0x8b1f else 3
        if p >= end:
            break
    return out


def _i32(x):
    return ((np.asarray(x, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def accepted(u, n_ref, csize=None, up=0):
    """Offsets c >= up of the inflated block u that guessNextBAMPos' test accepts
    (BAMSplitGuesser.java:301-398): c + 39 < csize, refID and mate refID in [-1, n_ref], both
    positions >= -1, a NUL at the end of the read name inside csize, and block_size >= 32 +
    l_read_name + 4 * n_cigar + l_seq + (l_seq + 1) / 2 in Java int arithmetic."""
    u = bytes(u)
    csize = len(u) if csize is None else csize
    last = min(csize, len(u)) - 40
    if last < up:
        return []
    a = np.frombuffer(u + bytes(300), np.uint8).astype(np.int64)
    w = _i32(a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24)
    c = np.arange(up, last + 1)
    ok = (w[c + 4] >= -1) & (w[c + 4] <= n_ref) & (w[c + 8] >= -1)
    ok &= (w[c + 24] >= -1) & (w[c + 24] <= n_ref) & (w[c + 28] >= -1)
    nl = a[c + 12]
    nul = c + 35 + nl
    ok &= (nul < csize) & (a[np.minimum(nul, len(a) - 1)] == 0)
    ls = w[c + 20]
    half = np.trunc(_i32(ls + 1) / 2).astype(np.int64)   # Java's / truncates toward zero
    zero_min = _i32(_i32(32 + nl + (a[c + 16] | a[c + 17] << 8) * 4) + _i32(ls + half))
    ok &= w[c] >= zero_min
    return [int(x) for x in c[ok]]


def member_at(data, p):
    """(total length, inflated payload or None) of the member whose header stands at file offset p,
    read the way BlockCompressedInputStream does (XLEN 6, BSIZE at +16)"""
    if p + 18 > len(data):
        return 0, None
    bl = struct.unpack_from("<H", data, p + 16)[0] + 1
    if bl < 26 or p + bl > len(data) or data[p:p + 4] != MAGIC or data[p + 10:p + 12] != b"\x06\x00":
        return bl, None
    try:
        u = zlib.decompressobj(-15).decompress(bytes(data[p + 18:p + bl - 8]))
    except zlib.error:
        return bl, None
    crc, isz = struct.unpack_from("<II", data, p + bl - 8)
    return bl, u if (len(u) == isz and zlib.crc32(u) == crc) else None


def chain_starts(data, p, off):
    """Record starts inside the member at p on the chain from payload offset `off`: block_size
    fields walked over the inflated stream of the members that follow p back to back, counted
    while the record starts inside p and is whole in that stream."""
    bl, u = member_at(data, p)
    assert u is not None
    first = len(u)
    q = p + bl
    while len(u) < first + (1 << 17):
        bl, v = member_at(data, q)
        if v is None or not bl:
            break
        u += v
        q += bl
    n, x = 0, off
    while x < first and x + 4 <= len(u):
        bs = struct.unpack_from("<i", u, x)[0]
        if bs < 32 or x + 4 + bs > len(u):
            break
        n += 1
        x += 4 + bs
    return n


def walks_to_block_end(data, v):
    """the virtual offset v starts a record chain that ends exactly at the end of its member"""
    bl, u = member_at(data, v >> 16)
    if u is None:
        return False
    x = v & 0xffff
    if x >= len(u):
        return False
    while x < len(u):
        if x + 4 > len(u):
            return False
        bs = struct.unpack_from("<i", u, x)[0]
        if bs < 32:
            return False
        x += 4 + bs
    return x == len(u)


def describe(data, beg, end, n_ref=N_REF, block=None, up=0, chain_from=None):
    """The paths k_guess_bam_wave takes for guess (beg, end) of the file `data`.  block: file offset
    of a member to describe too (accepted offsets from `up`, chain length from chain_from or the first of
    them)."""
    want = min(int(_i32(end - beg)), MAX_BYTES_READ)      # the (int) cast of BAMSplitGuesser.java:118
    total = max(0, min(want, len(data) - beg)) if beg >= 0 else 0
    first_end = min(int(_i32(end - beg)), 0xffff)
    w = bytes(data[beg:beg + total]) if total else b""
    mp = magic_positions(w)
    n_first = int((mp <= first_end).sum())
    d = dict(total=total, first_end=first_end, n_window=len(mp), n_first=n_first, cached=len(mp) <= GC_CAP,
             # a negative first_end (end < beg) never lists: the kernel asks first_end >= 0 too
             listed=first_end >= 0 and total >= first_end + 4 and n_first <= GW_MAG)
    if block is not None:
        bl, u = member_at(data, block)
        assert u is not None, "the described member must inflate"
        csize = struct.unpack_from("<i", data, block + bl - 4)[0]
        d["accepted"] = accepted(u, n_ref, csize, up)
        x = chain_from if chain_from is not None else (d["accepted"][0] if d["accepted"] else None)
        d["chain"] = chain_starts(data, block, x) if x is not None else 0
    return d
