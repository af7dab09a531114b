"""Plain-Python restatement of the reference's text VCF read path, for the tests only (the product
never imports it): the header parse, VCFRecordReader's split rule as the streaming loop of
VCFRecordReader.java:72-142 over an AsciiLineReaderIterator, the decode subset, the key, a
MurmurHash3 written from util/MurmurHash3.java:108-171, and a generator of VCF text."""
import random
import re

HBAM_OK, HBAM_ETRIBBLE, HBAM_ERUNTIME = 0, -14, -15

_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M
    k ^= k >> 33
    return k


def murmur_chars(chars, seed=0):
    """MurmurHash3.murmurhash3(CharSequence, int) -> signed 64-bit, line by line from the Java."""
    ch = [ord(c) for c in chars]
    n = len(ch)
    nblocks = n // 8
    h1 = h2 = seed & _M
    c1, c2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
    for i in range(nblocks):
        i0, i1 = (i * 2 + 0) * 4, (i * 2 + 1) * 4
        k1 = ch[i0] | ch[i0 + 1] << 16 | ch[i0 + 2] << 32 | ch[i0 + 3] << 48
        k2 = ch[i1] | ch[i1 + 1] << 16 | ch[i1 + 2] << 32 | ch[i1 + 3] << 48
        k1 = (k1 * c1) & _M; k1 = _rotl(k1, 31); k1 = (k1 * c2) & _M; h1 ^= k1
        h1 = _rotl(h1, 27); h1 = (h1 + h2) & _M; h1 = (h1 * 5 + 0x52dce729) & _M
        k2 = (k2 * c2) & _M; k2 = _rotl(k2, 33); k2 = (k2 * c1) & _M; h2 ^= k2
        h2 = ((h2 << 31) & _M) | (h1 >> (64 - 31)); h2 = (h2 + h1) & _M; h2 = (h2 * 5 + 0x38495ab5) & _M
    k1 = k2 = 0
    t = n & 7
    # the switch falls through; the indices are charAt(0..6): the start of the string
    if t >= 7: k2 ^= ch[6] << 32
    if t >= 6: k2 ^= ch[5] << 16
    if t >= 5:
        k2 ^= ch[4] << 0
        k2 = (k2 * c2) & _M; k2 = _rotl(k2, 33); k2 = (k2 * c1) & _M; h2 ^= k2
    if t >= 4: k1 ^= ch[3] << 48
    if t >= 3: k1 ^= ch[2] << 32
    if t >= 2: k1 ^= ch[1] << 16
    if t >= 1:
        k1 ^= ch[0] << 0
        k1 = (k1 * c1) & _M; k1 = _rotl(k1, 31); k1 = (k1 * c2) & _M; h1 ^= k1
    h1 ^= n; h2 ^= n
    h1 = (h1 + h2) & _M
    h2 = (h2 + h1) & _M
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = (h1 + h2) & _M
    return h1 - (1 << 64) if h1 >> 63 else h1


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


class LineIter:
    """AsciiLineReaderIterator over an AsciiLineReader opened at `open_at`: position() is the offset
    of the next unread line from there (the number of bytes consumed at the end of input)."""

    def __init__(self, data, open_at):
        self.d, self.open_at, self.p = data, open_at, min(open_at, len(data))

    def has_next(self):
        return self.p < len(self.d)

    def position(self):
        return self.p - self.open_at

    def peek(self):
        p = self.p
        line = self.next()
        self.p = p
        return line

    def next(self):
        nl = self.d.find(b"\n", self.p)
        if nl < 0:
            line, self.p = self.d[self.p:], len(self.d)
            return line
        line = self.d[self.p:nl]
        if line.endswith(b"\r"):
            line = line[:-1]
        self.p = nl + 1
        return line


class NoHeader(IOError):
    pass


class EmptyFile(IOError):
    pass


def _contig_id(line):
    body = line[line.index(b"<") + 1:line.rindex(b">")]
    parts, cur, quoted = [], bytearray(), False
    for b in body:
        c = bytes([b])
        if c == b'"':
            quoted = not quoted
        elif c == b"," and not quoted:
            parts.append(bytes(cur))
            cur = bytearray()
        else:
            cur += c
    parts.append(bytes(cur))
    for p in parts:
        k, _, v = p.partition(b"=")
        if k.strip() == b"ID":
            return v
    return None


def parse_header(data):
    """-> (header bytes, contigDict: ID bytes -> ordinal, data_start)"""
    it = LineIter(data, 0)
    contig, i = {}, 0
    while it.has_next():
        line = it.next()
        if line.startswith(b"##"):
            if line.startswith(b"##contig=<"):
                cid = _contig_id(line)
                if cid is not None:
                    contig[cid] = i
                    i += 1
            continue
        if line.startswith(b"#CHROM"):
            return data[:it.p], contig, it.p
        break
    raise NoHeader("No VCF header found")


_POS = re.compile(rb"^[+-]?[0-9]+$")


def decode(line, contig):
    """-> (status, tab[8], chrom, pos, ref_len, key): the subset of VCFCodec.decode + the key"""
    tab, at = [], -1
    while len(tab) < 8:
        at = line.find(b"\t", at + 1)
        if at < 0:
            break
        tab.append(at)
    ntab = len(tab)
    tab += [len(line)] * (8 - ntab)
    if line.startswith(b"#"):
        return HBAM_ERUNTIME, tab, 0, 0, 0, 0
    if ntab < 7:
        return HBAM_ETRIBBLE, tab, 0, 0, 0, 0
    f = line[tab[0] + 1:tab[1]]
    if not _POS.match(f) or not -(1 << 31) <= int(f) <= (1 << 31) - 1:
        return HBAM_ETRIBBLE, tab, 0, 0, 0, 0
    pos = int(f)
    name = line[:tab[0]]
    chrom = contig.get(name)
    if chrom is None:
        chrom = _i32(murmur_chars(name.decode("latin-1"), 0))
    low = _i32(pos - 1)
    key = ((chrom << 32) & _M) | (low & _M)  # (long)chromIdx << 32 | (long)(start - 1): sign-extended
    key = key - (1 << 64) if key >> 63 else key
    return HBAM_OK, tab, chrom, pos, tab[3] - tab[2] - 1, key


def read_split(data, start, length, parsed=None, position_rule_only=False):
    """VCFRecordReader.initialize + the nextKeyValue loop -> dict of lists; the first line that does
    not decode ends the split with its status (position_rule_only: it is skipped instead, which
    leaves the lines the split's position rule alone selects)."""
    _, contig, data_start = parsed or parse_header(data)
    if start != 0:
        it = LineIter(data, start - 1)
        if it.has_next():
            it.next()  # "skip incomplete line!"
    else:
        it = LineIter(data, 0)
        it.p = data_start
        if not it.has_next() or it.peek().startswith(b"#"):
            raise EmptyFile("Empty VCF file")
    out = dict(n=0, status=HBAM_OK, line_off=[], line_len=[], tab=[], chrom=[], pos=[], ref_len=[], key=[],
               lines=[])
    while it.has_next() and it.position() < length:
        off = it.p
        line = it.next()
        st, tab, chrom, pos, ref_len, key = decode(line, contig)
        if st != HBAM_OK:
            if position_rule_only:
                continue
            out["status"] = st
            break
        out["n"] += 1
        for k, v in (("line_off", off), ("line_len", len(line)), ("tab", tab), ("chrom", chrom), ("pos", pos),
                     ("ref_len", ref_len), ("key", key), ("lines", line)):
            out[k].append(v)
    return out


def file_splits(n, split_size):
    """Hadoop FileInputFormat.getSplits for one file (SPLIT_SLOP 1.1) -> [(start, length)]"""
    out, rem = [], n
    while rem / split_size > 1.1:
        out.append((n - rem, split_size))
        rem -= split_size
    if rem:
        out.append((n - rem, rem))
    return out


def lost_lines(data, split_size, splits=None):
    """Offsets of the data lines that the position rule gives to no split of this size.  (A split
    that begins inside the header also meets '#' lines, where the reference's decode fails: that
    ends such a split, and is left out of this count.)"""
    parsed = parse_header(data)
    whole = read_split(data, 0, len(data), parsed)["line_off"]
    got = []
    for s, ln in (file_splits(len(data), split_size) if splits is None else splits):
        try:
            got += read_split(data, s, ln, parsed, position_rule_only=True)["line_off"]
        except EmptyFile:
            pass
    assert len(got) == len(set(got))
    return sorted(set(whole) - set(got))


N_CONTIGS = 30


def gen_vcf(n_lines=20000, seed=5, crlf=False, long_lines=(3000, 12000), long_bytes=200_000):
    """VCF text: 30 header contigs; CHROM names absent from the header of every length 1..20;
    POS 0, 2147483647 and +5; lines under 64 bytes and lines with exactly 8 fields; two lines of
    about long_bytes; positions in random order with ties; a last line without a newline."""
    rng = random.Random(seed)
    eol = "\r\n" if crlf else "\n"
    out = ["##fileformat=VCFv4.1"]
    for i in range(N_CONTIGS):
        out.append('##contig=<ID=chr%d,length=%d,species="Homo sapiens, modern">' % (i + 1, 1000000 + i))
    out.append('##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">')
    out.append('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">')
    samples = ["S%03d" % i for i in range(12)]
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples))
    absent = ["".join(rng.choice("ABCDEFGHJKLMNPQRSTUVWXYZ_0123456789") for _ in range(k)) for k in range(1, 21)]
    special_pos = ["0", "2147483647", "+5"]
    for i in range(n_lines):
        r = rng.random()
        chrom = absent[i % 20] if i % 37 == 0 else "chr%d" % rng.randint(1, N_CONTIGS)
        pos = special_pos[(i // 101) % 3] if i % 101 == 0 else str(rng.randint(1, 5000))
        ref = rng.choice(["A", "C", "G", "T", "GTC", "ACGTACGT"])
        alt = rng.choice(["A", "C", "G,T", "."])
        if i in long_lines:
            gts = "\t".join("%d|%d:%d" % (rng.randint(0, 1), rng.randint(0, 1), rng.randint(0, 99))
                            for _ in range(long_bytes // 7))
            line = "%s\t%s\trs%d\t%s\t%s\t50\tPASS\tDP=%d\tGT:GQ\t%s" % (chrom, pos, i, ref, alt, i, gts)
        elif r < 0.1:
            line = "%s\t%s\t.\t%s\t%s\t.\t.\t." % (chrom, pos, ref, alt)  # 8 fields, under 64 bytes
        else:
            gts = "\t".join("%d/%d:%d:%d,%d" % (rng.randint(0, 1), rng.randint(0, 1), rng.randint(0, 99),
                                              rng.randint(0, 60), rng.randint(0, 60)) for _ in samples)
            line = "%s\t%s\trs%d\t%s\t%s\t%d\tPASS\tDP=%d;AF=0.5\tGT:GQ:HQ\t%s" % (
                chrom, pos, i, ref, alt, rng.randint(1, 99), rng.randint(1, 500), gts)
        out.append(line)
    return eol.join(out).encode()  # no newline after the last line
