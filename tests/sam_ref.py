"""Plain-Python restatement of the SAM text read path, for the tests only (the product never
imports it), written from the rules of include/hbam.h and not from the device code: a renderer of
BAM records as SAM text, the line -> BAM record encoder with its error codes (float32 rounding done
exactly with fractions.Fraction), the key with the seeded MurmurHash3 chain of
BAMRecordReader.getKey :88-95, and the split rule of SAMRecordReader / WorkaroundingStream as the
begin-offset rule.  htsjdk is not in the reference tree: the rules are restated from memory
(DESIGN.md lists them), so parity is between two restatements."""
import re
import struct
from fractions import Fraction

import numpy as np

import vcf_ref

HBAM_OK, HBAM_EFORMAT, HBAM_EUNSUPPORTED, HBAM_EINVAL, HBAM_EMORE = 0, -3, -9, -11, -12

SEQ_TABLE = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
_REF_OPS = (0, 2, 3, 7, 8)
_M = (1 << 64) - 1
_INT = re.compile(rb"[+-]?[0-9]+")
_CIGAR = re.compile(rb"([0-9]+)([MIDNSHP=X])")
_FLOAT = re.compile(rb"([+-]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?")
_INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_INT_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535),
              "i": (-(1 << 31), (1 << 31) - 1), "I": (0, (1 << 32) - 1)}


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


# ---- BAM records -> SAM text ------------------------------------------------------------------
def split_records(ubuf, n=None):
    """The records (block_size + record) of a packed record stream."""
    b, out, p = bytes(ubuf), [], 0
    while p < len(b) and (n is None or len(out) < n):
        bs = struct.unpack_from("<i", b, p)[0]
        out.append(b[p:p + 4 + bs])
        p += 4 + bs
    return out


def fields(rec):
    """A BAM record's fields as a dict (name without the NUL, cigar as u32 words, aux raw)."""
    (bs, ref, pos, lrn, mapq, bin_, ncig, flag, lseq, nref, npos, tlen) = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    p = 36
    name = rec[p:p + lrn - 1]
    p += lrn
    cigar = list(struct.unpack_from("<%dI" % ncig, rec, p))
    p += 4 * ncig
    seq = rec[p:p + (lseq + 1) // 2]
    p += (lseq + 1) // 2
    qual = rec[p:p + lseq]
    p += lseq
    return dict(block_size=bs, ref=ref, pos=pos, l_read_name=lrn, mapq=mapq, bin=bin_, n_cigar=ncig, flag=flag,
                l_seq=lseq, nref=nref, npos=npos, tlen=tlen, name=name, cigar=cigar, seq=seq, qual=qual,
                aux=rec[p:4 + bs])


def float_text(bits):
    """The shortest decimal text that reads back as this float32."""
    return str(np.frombuffer(struct.pack("<I", bits), np.float32)[0])


def decode_aux(aux):
    """-> [(tag, kind, value)]: integers of every width become kind 'i'; floats are their bits."""
    out, p = [], 0
    while p < len(aux):
        tag, t = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if t == "A":
            out.append((tag, "A", aux[p:p + 1]))
            p += 1
        elif t in _INT_FMT:
            w = struct.calcsize(_INT_FMT[t])
            out.append((tag, "i", struct.unpack_from(_INT_FMT[t], aux, p)[0]))
            p += w
        elif t == "f":
            out.append((tag, "f", struct.unpack_from("<I", aux, p)[0]))
            p += 4
        elif t in "ZH":
            e = aux.index(b"\0", p)
            out.append((tag, t, aux[p:e]))
            p = e + 1
        elif t == "B":
            sub = chr(aux[p])
            cnt = struct.unpack_from("<i", aux, p + 1)[0]
            p += 5
            fmt = "<I" if sub == "f" else _INT_FMT[sub]
            w = struct.calcsize(fmt)
            out.append((tag, "B" + sub, tuple(struct.unpack_from(fmt, aux, p + w * k)[0] for k in range(cnt))))
            p += w * cnt
        else:
            raise ValueError("aux type %r" % t)
    return out


def render(bam_records, refs):
    """BAM records (block_size + record each) -> their SAM lines (bytes, no line ends).  Floats
    are written in the shortest form that round-trips the float32, integers of every width as i."""
    lines = []
    for rec in bam_records:
        f = fields(rec)
        rname = refs[f["ref"]] if f["ref"] >= 0 else b"*"
        if f["nref"] < 0:
            rnext = b"*"
        elif f["nref"] == f["ref"]:
            rnext = b"="
        else:
            rnext = refs[f["nref"]]
        cigar = b"".join(b"%d%c" % (w >> 4, CIGAR_OPS[w & 15]) for w in f["cigar"]) or b"*"
        ls = f["l_seq"]
        if ls == 0:
            seq = qual = b"*"
        else:
            codes = np.frombuffer(f["seq"], np.uint8)
            nib = np.empty(2 * len(codes), np.uint8)
            nib[0::2], nib[1::2] = codes >> 4, codes & 15
            seq = np.frombuffer(SEQ_TABLE, np.uint8)[nib[:ls]].tobytes()
            q = np.frombuffer(f["qual"], np.uint8)
            qual = b"*" if q[0] == 0xff else (q + 33).astype(np.uint8).tobytes()
        cols = [f["name"], b"%d" % f["flag"], rname, b"%d" % (f["pos"] + 1), b"%d" % f["mapq"], cigar, rnext,
                b"%d" % (f["npos"] + 1), b"%d" % f["tlen"], seq, qual]
        for tag, kind, v in decode_aux(f["aux"]):
            if kind == "i":
                cols.append(tag + b":i:%d" % v)
            elif kind == "f":
                cols.append(tag + b":f:" + float_text(v).encode())
            elif kind in "AZH":
                cols.append(tag + b":" + kind.encode() + b":" + v)
            else:
                vals = [float_text(x).encode() if kind == "Bf" else b"%d" % x for x in v]
                cols.append(tag + b":B:" + b",".join([kind[1:].encode()] + vals))
        lines.append(b"\t".join(cols))
    return lines


def header_text(text, refs):
    """A SAM text header: `text` ('@' lines), with @SQ lines for `refs` (name, length) when it has none."""
    lines = [ln for ln in bytes(text).split(b"\n") if ln.startswith(b"@")]
    if not any(ln.startswith(b"@SQ") for ln in lines):
        lines += [b"@SQ\tSN:%s\tLN:%d" % (n, ln) for n, ln in refs]
    return lines


def sam_file(header_lines, lines, eol=b"\n", last_eol=True):
    body = eol.join(list(header_lines) + list(lines))
    return body + (eol if last_eol and body else b"")


# ---- SAM line -> BAM record ---------------------------------------------------------------------
def float32_bits(text):
    """Decimal text -> the bits of the nearest float32 (ties to even), exactly; None outside the
    domain of include/hbam.h (at most 9 significant digits once leading and trailing zeros are
    dropped, decimal exponent in [-20, 20] once they are an integer; zero with any exponent)."""
    m = _FLOAT.fullmatch(text)
    if not m or not (m.group(2) or m.group(3)):
        return None
    sign = 0x80000000 if m.group(1) == b"-" else 0
    ip, fp = m.group(2), m.group(3) or b""
    e = -len(fp) + (int(m.group(4)) if m.group(4) else 0)
    sig = (ip + fp).lstrip(b"0")
    if not sig:
        return sign
    e += len(sig) - len(sig.rstrip(b"0"))
    sig = sig.rstrip(b"0")
    if len(sig) > 9 or not -20 <= e <= 20:
        return None
    v = Fraction(int(sig)) * Fraction(10) ** e
    e2 = 0  # v = f x 2^e2 with 2^23 <= f < 2^24
    while v >= 1 << 24:
        v /= 2
        e2 += 1
    while v < 1 << 23:
        v *= 2
        e2 -= 1
    mant = v.numerator // v.denominator
    rem = v - mant
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and mant & 1):
        mant += 1
    if mant == 1 << 24:
        mant >>= 1
        e2 += 1
    return sign | (127 + 23 + e2) << 23 | (mant & 0x7fffff)


def int_tag(v):
    """The type and bytes of an i tag's value: the narrowest type, in htsjdk's order."""
    if v > (1 << 31) - 1:
        t = "I"
    elif v > 65535:
        t = "i"
    elif v > 32767:
        t = "S"
    elif v > 255:
        t = "s"
    elif v > 127:
        t = "C"
    elif v >= -128:
        t = "c"
    elif v >= -32768:
        t = "s"
    else:
        t = "i"
    return t, struct.pack(_INT_FMT[t], v)


def _parse_int(b, lo=-(1 << 31), hi=(1 << 31) - 1):
    if not _INT.fullmatch(b):
        return None
    v = int(b)
    return v if lo <= v <= hi else None


def _encode_tag(f):
    if len(f) < 6 or f[2:3] != b":" or f[4:5] != b":":
        return HBAM_EFORMAT
    tag, t, v = f[:2], chr(f[3]), f[5:]
    if t == "A":
        return tag + b"A" + v if len(v) == 1 else HBAM_EFORMAT
    if t == "Z":
        return tag + b"Z" + v + b"\0"
    if t == "i":
        x = _parse_int(v, -(1 << 31), (1 << 32) - 1)
        if x is None:
            return HBAM_EFORMAT
        ty, raw = int_tag(x)
        return tag + ty.encode() + raw
    if t == "f":
        bits = float32_bits(v)
        return HBAM_EUNSUPPORTED if bits is None else tag + b"f" + struct.pack("<I", bits)
    if t == "B":
        parts = v.split(b",")
        sub = parts[0].decode("latin-1")
        if sub not in "cCsSiIf" or len(sub) != 1:
            return HBAM_EFORMAT
        vals = []
        for p in parts[1:]:
            if not p:
                return HBAM_EFORMAT
            if sub == "f":
                bits = float32_bits(p)
                if bits is None:
                    return HBAM_EUNSUPPORTED
                vals.append(struct.pack("<I", bits))
            else:
                x = _parse_int(p, *_INT_RANGE[sub])
                if x is None:
                    return HBAM_EFORMAT
                vals.append(struct.pack(_INT_FMT[sub], x))
        return tag + b"B" + sub.encode() + struct.pack("<i", len(vals)) + b"".join(vals)
    return HBAM_EUNSUPPORTED if t == "H" else HBAM_EFORMAT


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def parse_line(line, dictionary):
    """-> a dict of the parsed line, or an error code.  Checked in field order, the tags left to
    right, the SEQ and QUAL bytes last; the first failure is the line's code."""
    f = line.split(b"\t")
    if len(f) < 11 or any(len(x) == 0 for x in f[:11]):
        return HBAM_EFORMAT
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if len(qname) > 254:
        return HBAM_EUNSUPPORTED
    flag = _parse_int(flag)
    if flag is None:
        return HBAM_EFORMAT
    ref = -1 if rname == b"*" else dictionary.get(rname, -1)
    pos, mapq = _parse_int(pos), _parse_int(mapq)
    if pos is None or mapq is None:
        return HBAM_EFORMAT
    ops = []
    if cigar != b"*":
        at = 0
        while at < len(cigar):
            m = _CIGAR.match(cigar, at)
            if not m or int(m.group(1)) >= 1 << 28:
                return HBAM_EFORMAT
            ops.append(int(m.group(1)) << 4 | CIGAR_OPS.index(m.group(2)))
            at = m.end()
        if len(ops) > 65535:
            return HBAM_EUNSUPPORTED
    if rnext == b"=":
        nref = ref
    else:
        nref = -1 if rnext == b"*" else dictionary.get(rnext, -1)
    pnext, tlen = _parse_int(pnext), _parse_int(tlen)
    if pnext is None or tlen is None:
        return HBAM_EFORMAT
    lseq = 0 if seq == b"*" else len(seq)
    if qual != b"*" and (seq == b"*" or len(qual) != lseq):
        return HBAM_EFORMAT
    aux = []
    for t in f[11:]:
        a = _encode_tag(t)
        if isinstance(a, int):
            return a
        aux.append(a)
    bases = b"" if seq == b"*" else seq.upper().replace(b".", b"N")
    if any(c not in SEQ_TABLE for c in bases):
        return HBAM_EFORMAT
    if qual != b"*" and min(qual) < 33:
        return HBAM_EFORMAT
    quals = b"" if qual == b"*" else bytes((c - 33) & 0xff for c in qual)
    return dict(name=qname, flag=flag, ref=ref, pos=_i32(pos - 1), mapq=mapq, ops=ops, nref=nref,
                npos=_i32(pnext - 1), tlen=tlen, bases=bases, quals=quals, l_seq=lseq, aux=b"".join(aux),
                cigar_text=cigar)


def encode(p):
    """BAMRecordCodec.encode of a parsed line -> block_size + record"""
    reflen = sum(w >> 4 for w in p["ops"] if (w & 15) in _REF_OPS) & 0xffffffff
    pos0 = p["pos"]
    end = 0 if p["flag"] & 4 else _i32(pos0 + reflen)
    if end <= 0:
        end = _i32(pos0 + 1)
    bin_ = reg2bin(pos0, end)
    codes = [SEQ_TABLE.index(c) for c in p["bases"]] + [0]
    packed = bytes(codes[2 * k] << 4 | codes[2 * k + 1] for k in range((p["l_seq"] + 1) // 2))
    qual = p["quals"] if p["quals"] or not p["l_seq"] else b"\xff" * p["l_seq"]
    var = (p["name"] + b"\0" + b"".join(struct.pack("<I", w) for w in p["ops"]) + packed + qual + p["aux"])
    fixed = struct.pack("<iiBBHHHiiii", p["ref"], pos0, len(p["name"]) + 1, p["mapq"] & 0xff, bin_ & 0xffff,
                        len(p["ops"]), p["flag"] & 0xffff, p["l_seq"], p["nref"], p["npos"], p["tlen"])
    return struct.pack("<i", len(fixed) + len(var)) + fixed + var


def parse_encode(line, dictionary):
    """A SAM line -> its BAM record bytes (block_size + record), or an error code."""
    p = parse_line(line, dictionary)
    return p if isinstance(p, int) else encode(p)


# ---- the key --------------------------------------------------------------------------------
def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M
    return k ^ (k >> 33)


def murmur_bytes(key, seed=0):
    """MurmurHash3.murmurhash3(byte[], int) (util/MurmurHash3.java:32-102) -> signed 64-bit; the
    block step rotates h2 as h2 << 31 | h1 >>> 33 (:59), as the reference does."""
    key = bytes(key)
    n = len(key)
    h1 = h2 = seed & _M  # (long)seed: sign-extended
    c1, c2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
    nb = n // 16
    for i in range(nb):
        k1, k2 = struct.unpack_from("<QQ", key, 16 * i)
        k1 = (k1 * c1) & _M; k1 = _rotl(k1, 31); k1 = (k1 * c2) & _M; h1 ^= k1
        h1 = _rotl(h1, 27); h1 = (h1 + h2) & _M; h1 = (h1 * 5 + 0x52dce729) & _M
        k2 = (k2 * c2) & _M; k2 = _rotl(k2, 33); k2 = (k2 * c1) & _M; h2 ^= k2
        h2 = ((h2 << 31) & _M) | (h1 >> 33); h2 = (h2 + h1) & _M; h2 = (h2 * 5 + 0x38495ab5) & _M
    tail = key[16 * nb:]
    k1 = int.from_bytes(tail[:8], "little")
    k2 = int.from_bytes(tail[8:], "little")
    if len(tail) > 8:
        k2 = (k2 * c2) & _M; k2 = _rotl(k2, 33); k2 = (k2 * c1) & _M; h2 ^= k2
    if tail:
        k1 = (k1 * c1) & _M; k1 = _rotl(k1, 31); k1 = (k1 * c2) & _M; h1 ^= k1
    h1 ^= n; h2 ^= n
    h1 = (h1 + h2) & _M
    h2 = (h2 + h1) & _M
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = (h1 + h2) & _M
    return h1 - (1 << 64) if h1 >> 63 else h1


def key(p):
    """BAMRecordReader.getKey of a parsed line (parse_line's dict)."""
    start = _i32(p["pos"] + 1)
    if not (p["flag"] & 4 or p["ref"] < 0 or start < 0):
        hi, lo = p["ref"], p["pos"]
    else:
        h = _i32(vcf_ref.murmur_chars(p["name"].decode("latin-1"), 0))
        h = _i32(murmur_bytes(p["bases"], h))
        h = _i32(murmur_bytes(p["quals"], h))
        h = _i32(vcf_ref.murmur_chars(p["cigar_text"].decode("latin-1"), h))
        hi, lo = 0x7fffffff, h
    k = ((hi << 32) & _M) | (lo & _M)  # the low int is sign-extended
    return k - (1 << 64) if k >> 63 else k


# ---- the split rule --------------------------------------------------------------------------
def data_start(data):
    """The offset of the first byte after the last '@' line of the header."""
    p = 0
    while p < len(data) and data[p:p + 1] == b"@":
        nl = data.find(b"\n", p)
        p = len(data) if nl < 0 else nl + 1
    return p


def dictionary(data):
    """@SQ SN -> ordinal"""
    d = {}
    for ln in bytes(data[:data_start(data)]).split(b"\n"):
        if ln.startswith(b"@SQ"):
            for f in ln.rstrip(b"\r").split(b"\t")[1:]:
                if f.startswith(b"SN:"):
                    d[f[3:]] = len(d)
                    break
    return d


def all_lines(data):
    """(offset, line without its end) of every data line"""
    out, p = [], data_start(data)
    while p < len(data):
        nl = data.find(b"\n", p)
        e = len(data) if nl < 0 else nl
        line = data[p:e]
        if nl >= 0 and line.endswith(b"\r"):
            line = line[:-1]
        out.append((p, line))
        p = e + 1
    return out


def read_split(data, start, length):
    """The lines of FileSplit [start, start + length): those whose first byte b satisfies
    max(start, data_start) <= b < start + length."""
    lo = max(start, data_start(data))
    return [(o, ln) for o, ln in all_lines(data) if lo <= o < start + length]


def decode_split(data, start, length, dic=None):
    """What hbam_sam_decode_split returns for the split, from the rules: n, status, the record
    bytes, rec_off, key and voffset; the first failing line ends it."""
    dic = dictionary(data) if dic is None else dic
    out = dict(n=0, status=HBAM_OK, records=[], key=[], voffset=[])
    for off, line in read_split(data, start, length):
        p = parse_line(line, dic)
        if isinstance(p, int):
            out["status"] = p
            break
        out["n"] += 1
        out["records"].append(encode(p))
        out["key"].append(key(p))
        out["voffset"].append(off)
    out["ubuf"] = np.frombuffer(b"".join(out["records"]), np.uint8)
    ro = np.zeros(out["n"] + 1, np.uint64)
    ro[1:] = np.cumsum([len(r) for r in out["records"]])
    out["rec_off"] = ro
    out["key"] = np.array(out["key"], np.int64)
    out["voffset"] = np.array(out["voffset"], np.uint64)
    return out
