"""The VCF text rules of hbam_vcf_render (include/hbam.h), restated in plain Python for the
tests: htsjdk's VCFEncoder and BCF2 value decoders as the project states them (parity unpinned).
Nothing here imports hadoop_bam.

parse_header(text) -> the header's contigs, samples, string dictionary and INFO / FORMAT lines;
render(record, hdr) -> (status, line, deferred) of one record; render_stream(records, hdr, perm) ->
what the device call returns for them: text (a deferred line empty), lines (every line in full, the
deferred ones as the host renderer writes them), line_off, deferred, status and n."""
import struct
from decimal import ROUND_HALF_UP, Decimal

OK, EUNSUPPORTED, ETRIBBLE, ERUNTIME = 0, -9, -14, -15
MAX_INFO, MAX_FILTER, MAX_FORMAT, MAX_PLOIDY = 64, 64, 16, 16
MISSING_FLOAT = 0x7F800001
_WIDTH = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
_INTFMT = {1: "<b", 2: "<h", 3: "<i"}
_INTMISS = {1: -128, 2: -32768, 3: -(1 << 31)}
_KINDS = ("GT", "DP", "GQ", "AD", "PL", "FT")


class Fail(Exception):
    def __init__(self, code):
        Exception.__init__(self, "status %d" % code)
        self.code = code


# ---- header ------------------------------------------------------------------------------------
def _attr(line, name):
    """The value of name= in a ##XXX=<...> line: name stands behind '<' or ','; the value ends at
    ',' or '>'."""
    at = 0
    while True:
        at = line.find(name + "=", at)
        if at < 0:
            return None
        if at > 0 and line[at - 1] in "<,":
            v = line[at + len(name) + 1:]
            for i, ch in enumerate(v):
                if ch in ",>":
                    return v[:i]
            return v
        at += 1


def parse_header(text):
    text = text.decode("latin-1") if isinstance(text, bytes) else text
    h = {"contigs": [], "samples": [], "dict": ["PASS"], "info": {}, "format": {}}
    for line in text.split("\n"):
        if line.startswith("##contig=<"):
            h["contigs"].append(_attr(line, "ID"))
        elif line.startswith(("##FILTER=<", "##INFO=<", "##FORMAT=<")):
            i = _attr(line, "ID")
            if i is None:
                continue
            if i != "PASS" and i not in h["dict"]:
                h["dict"].append(i)
            which = "info" if line.startswith("##INFO") else "format" if line.startswith("##FORMAT") else None
            if which and i not in h[which]:
                h[which][i] = (_attr(line, "Number"), _attr(line, "Type"))
        elif line.startswith("#CHROM"):
            h["samples"] = line.split("\t")[9:]
    order = sorted(range(len(h["dict"])), key=lambda i: h["dict"][i].encode("latin-1"))
    h["rank"] = [0] * len(order)
    for r, i in enumerate(order):
        h["rank"][i] = r
    return h


# ---- numbers -----------------------------------------------------------------------------------
def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits & 0xffffffff))[0]


def _special(d):
    if d != d:
        return "NaN"
    if d in (float("inf"), float("-inf")):
        return "Infinity" if d > 0 else "-Infinity"
    return None


def _fixed(d, places):
    return str(Decimal(d).quantize(Decimal(1).scaleb(-places), rounding=ROUND_HALF_UP))


def _sci3(d):
    """Java's %.3e: d.ddde[+-]xx, HALF_UP."""
    D = Decimal(d)
    sign, a = ("-" if D < 0 else ""), abs(D)
    e = a.adjusted()
    m = a.scaleb(-e).quantize(Decimal("0.001"), rounding=ROUND_HALF_UP)
    if m >= 10:
        m, e = (m / 10).quantize(Decimal("0.001"), rounding=ROUND_HALF_UP), e + 1
    return "%s%se%s%02d" % (sign, m, "+" if e >= 0 else "-", abs(e))


def format_vcf_double(bits):
    """formatVCFDouble of the float32 widened to double.  (A NaN is below nothing: it takes the %.2f
    branch, where Java prints NaN.)"""
    d = _f32(bits)
    if _special(d):
        return _special(d)
    if d < 1:
        if d < 0.01:
            return _sci3(d) if abs(d) >= 1e-20 else "0.00"
        return _fixed(d, 3)
    return _fixed(d, 2)


def float_on_device(bits):
    d = _f32(bits)
    if bits & 0x7fffffff == 0:
        return True
    return not (bits >> 31) and not _special(d) and 0.01 <= d < 1e7


def qual_text(bits):
    if bits == MISSING_FLOAT:
        return "."
    q = _f32(bits)
    d = (q / -10.0) * -10.0 + 0.0
    s = _special(d) or _fixed(d, 2)
    return s[:-3] if s.endswith(".00") else s


def qual_on_device(bits):
    if bits == MISSING_FLOAT:
        return True
    q = _f32(bits)
    if (bits >> 31) or _special(q) or q >= 1e7:
        return False
    x = 8 * q
    return not (x == int(x) and int(x) % 2 == 1)


# ---- typed values --------------------------------------------------------------------------------
def _typed(b, end, at, mult=1):
    """(t, k, off) of the descriptor at `at` in a block that ends at `end`."""
    if at >= end:
        raise Fail(ETRIBBLE)
    d = b[at]
    at += 1
    t, k = d & 15, d >> 4
    if k == 15:
        if at >= end:
            raise Fail(ETRIBBLE)
        t2 = b[at] & 15
        at += 1
        if t2 not in _INTFMT:
            raise Fail(ERUNTIME)
        if end - at < _WIDTH[t2]:
            raise Fail(ETRIBBLE)
        k = max(0, struct.unpack_from(_INTFMT[t2], b, at)[0])
        at += _WIDTH[t2]
    if k == 0:
        return t, 0, at
    if t not in _WIDTH:
        raise Fail(ERUNTIME)
    if k * _WIDTH[t] * mult > end - at:
        raise Fail(ETRIBBLE)
    return t, k, at


def _ints(b, t, k, off):
    return [struct.unpack_from(_INTFMT[t], b, off + i * _WIDTH[t])[0] for i in range(k)]


def _string(b, k, off):
    return bytes(b[off:off + k]).rstrip(b"\0")


def _value(b, t, k, off):
    """decodeTypedValue -> (text or None for null, the device can write it)."""
    if k == 0:
        return None, True
    if t == 7:
        s = _string(b, k, off)
        if not s:
            return None, True
        return (s[1:] if s.startswith(b",") else s).decode("latin-1"), True
    if t == 5:
        v = [x for x in struct.unpack_from("<%dI" % k, b, off) if x != MISSING_FLOAT]
        if not v:
            return None, True
        return ",".join(format_vcf_double(x) for x in v), all(float_on_device(x) for x in v)
    v = [x for x in _ints(b, t, k, off) if x != _INTMISS[t]]
    return (",".join("%d" % x for x in v) if v else None), True


def _int_array(b, t, k, off):
    """decodeIntArray: the values before the first missing one, None for none."""
    out = []
    for x in _ints(b, t, k, off) if k else []:
        if x == _INTMISS[t]:
            break
        out.append(x)
    return out or None


def _allele(s):
    sym = (s.startswith(b"<") and s.endswith(b">")) or b"[" in s or b"]" in s or s.startswith(b".") or s.endswith(b".")
    return s if sym else bytes(c - 32 if 97 <= c <= 122 else c for c in s)


# ---- one record ----------------------------------------------------------------------------------
def render(rec, hdr):
    """-> (status, line bytes or None, deferred)."""
    try:
        line, deferred = _render(bytes(rec), hdr)
        return OK, line, deferred
    except Fail as e:
        return e.code, None, False


def _render(b, hdr):
    names, rank = hdr["dict"], hdr["rank"]
    if len(b) < 8:
        raise Fail(ETRIBBLE)
    ls, li = struct.unpack_from("<ii", b, 0)
    if ls < 24 or li < 0 or 8 + ls + li > len(b):
        raise Fail(ETRIBBLE)
    send, end = 8 + ls, 8 + ls + li
    chrom, pos, _, qual, nai, nfs = struct.unpack_from("<iiiIII", b, 8)
    n_allele, n_info, n_sample, n_fmt = nai >> 16, nai & 0xffff, nfs & 0xffffff, nfs >> 24
    if not 0 <= chrom < len(hdr["contigs"]):
        raise Fail(ERUNTIME)
    if n_sample != len(hdr["samples"]) or n_allele < 1:
        raise Fail(ETRIBBLE)
    deferred = False
    cols = [hdr["contigs"][chrom].encode("latin-1"), b"%d" % (((pos + 1 + (1 << 31)) & 0xffffffff) - (1 << 31))]
    t, k, at = _typed(b, send, 32)
    if k and t != 7:
        raise Fail(ERUNTIME)
    cols.append(_string(b, k, at) or b".")
    at += k
    alleles = []
    for _ in range(n_allele):
        t, k, at = _typed(b, send, at)
        if k and t != 7:
            raise Fail(ERUNTIME)
        s = _string(b, k, at)
        if not s:
            raise Fail(ERUNTIME)
        alleles.append(_allele(s))
        at += k
    cols += [alleles[0], b",".join(alleles[1:]) or b"."]
    cols.append(qual_text(qual).encode())
    deferred |= not qual_on_device(qual)
    # FILTER
    t, k, at = _typed(b, send, at)
    if k and t not in _INTFMT:
        raise Fail(ERUNTIME)
    fl = _ints(b, t, k, at) if k else []
    if any(not 0 <= e < len(names) for e in fl):
        raise Fail(ERUNTIME)
    at += k * _WIDTH.get(t, 0)
    deferred |= len(fl) > MAX_FILTER
    cols.append(";".join(names[e] for e in sorted(set(fl), key=lambda e: rank[e])).encode("latin-1") or b".")
    # INFO
    info, seen = {}, []
    for _ in range(n_info):
        t, k, at = _typed(b, send, at)
        if not (k == 1 and t in _INTFMT):
            raise Fail(ERUNTIME)
        key = _ints(b, t, 1, at)[0]
        if not 0 <= key < len(names):
            raise Fail(ERUNTIME)
        if names[key] not in hdr["info"]:
            raise Fail(ETRIBBLE)
        at += _WIDTH[t]
        t, k, at = _typed(b, send, at)
        info[key] = (t, k, at)  # a repeated key: the last one wins
        seen.append(key)
        at += k * _WIDTH.get(t, 0)
    deferred |= n_info > MAX_INFO or len(set(seen)) != len(seen)
    parts = []
    for key in sorted(info, key=lambda e: rank[e]):
        number, typ = hdr["info"][names[key]]
        if typ == "Flag" or number == "0":
            parts.append(names[key])
            continue
        text, dev = _value(b, *info[key])
        deferred |= not dev
        text = "." if text is None else text
        parts.append(names[key] + ("=" + text if text else ""))
    cols.append(";".join(parts).encode("latin-1") or b".")
    # the genotype fields' headers
    fields, at, gt = [], send, None
    deferred |= n_fmt > MAX_FORMAT
    for f in range(n_fmt):
        t, k, at = _typed(b, end, at)
        if not (k == 1 and t in _INTFMT):
            raise Fail(ERUNTIME)
        key = _ints(b, t, 1, at)[0]
        at += _WIDTH[t]
        if not 0 <= key < len(names) or names[key] not in hdr["format"]:
            raise Fail(ERUNTIME)
        t, k, at = _typed(b, end, at, n_sample)
        kind = names[key] if names[key] in _KINDS else "generic"
        ints = k == 0 or t in _INTFMT
        if kind == "GT":
            if not ints or gt is not None:
                raise Fail(ERUNTIME)
            gt = f
            deferred |= k > MAX_PLOIDY
        elif kind in ("DP", "GQ"):
            if k != 1:
                raise Fail(EUNSUPPORTED)
            if not ints:
                raise Fail(ERUNTIME)
        elif kind in ("AD", "PL"):
            if not ints:
                raise Fail(ERUNTIME)
        elif kind == "FT" or not ints:
            deferred = True
        fields.append((key, kind, t, k, at))
        at += k * _WIDTH.get(t, 0) * n_sample
    if n_sample == 0:
        return b"\t".join(cols) + b"\n", deferred
    # the samples' values
    def at_sample(fd, s):
        key, kind, t, k, off = fd
        o = off + s * k * _WIDTH.get(t, 0)
        if kind in ("GT", "AD", "PL"):
            return _int_array(b, t, k, o)
        if kind in ("DP", "GQ"):
            x = _ints(b, t, 1, o)[0]
            return None if x == _INTMISS[t] else x
        return _value(b, t, k, o)[0]

    vals = [[at_sample(fd, s) for fd in fields] for s in range(n_sample)]
    for s in range(n_sample):
        if gt is not None:
            _, _, t, k, off = fields[gt]
            for x in _int_array(b, t, k, off + s * k * _WIDTH.get(t, 0)) or []:
                if not 0 <= (x >> 1) <= n_allele:
                    raise Fail(ERUNTIME)
    present = [f for f in range(n_fmt) if f != gt and any(vals[s][f] is not None for s in range(n_sample))]
    gt_key = (gt is not None and any(vals[s][gt] is not None for s in range(n_sample))) or not present
    if gt_key and (gt is None or any(vals[s][gt] is None for s in range(n_sample))):
        raise Fail(ERUNTIME)
    keys = sorted(present, key=lambda f: (rank[fields[f][0]], f))
    for f in keys:
        key, kind = fields[f][0], fields[f][1]
        if kind == "generic" and hdr["format"][names[key]][0] == "G" and any(vals[s][f] is None for s in range(n_sample)):
            deferred = True
    cols.append(":".join((["GT"] if gt_key else []) + [names[fields[f][0]] for f in keys]).encode("latin-1"))
    for s in range(n_sample):
        out = []
        for f in keys:
            key, kind = fields[f][0], fields[f][1]
            v = vals[s][f]
            if v is None:
                cnt = 1
                if kind == "generic":
                    number = hdr["format"][names[key]][0]
                    cnt = {"A": n_allele - 1, "R": n_allele, ".": 1, "G": 1}.get(number)
                    cnt = int(number) if cnt is None else cnt
                out.append(",".join(["."] * max(cnt, 1)))
            elif isinstance(v, list):
                out.append(",".join("%d" % x for x in v))
            else:
                out.append("%d" % v if isinstance(v, int) else v)
        while out and not out[-1].strip(".,"):
            out.pop()
        if gt_key:
            enc = vals[s][gt]
            sep = "|" if enc[0] & 1 else "/"
            out.insert(0, sep.join("." if x >> 1 == 0 else "%d" % ((x >> 1) - 1) for x in enc))
        cols.append(":".join(out).encode("latin-1"))
    return b"\t".join(cols) + b"\n", deferred


# ---- a stream of records: what the device call returns ---------------------------------------------
def render_stream(records, hdr, perm=None):
    order = range(len(records)) if perm is None else perm
    text, lines, line_off, deferred, status = [], [], [0], [], OK
    for k, i in enumerate(order):
        st, line, d = render(records[i], hdr)
        if st != OK:
            status = st
            break
        lines.append(line)
        if d:
            deferred.append(k)
        else:
            text.append(line)
        line_off.append(line_off[-1] + (0 if d else len(line)))
    return {"text": b"".join(text), "lines": lines, "line_off": line_off, "deferred": deferred,
            "status": status, "n": len(lines)}
