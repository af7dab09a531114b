"""VCF text output over the MI355X C ABI: VCFRecordWriter (VCFRecordWriter.java),
KeyIgnoringVCFRecordWriter, VCFOutputFormat (VCFOutputFormat.java), KeyIgnoringVCFOutputFormat
(KeyIgnoringVCFOutputFormat.java:55-117), same names, argument meaning and exceptions.

The lines are rendered on the device (hbam_vcf_render, hbam_vcftext.hip) from BCF2 records: htsjdk's
VCFEncoder over what its BCF2 decoders read, restated from memory (htsjdk is not in the reference
tree: parity unpinned; include/hbam.h and DESIGN.md list the rules).  The device hands a record to
the host where the text is not provably the rule's (should_defer lists when): render_record writes
that line and the writer splices it in.  Output is VCF text only: BCFRecordWriter is not restated."""
import os
import struct
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

from . import _lib
from .bcf import BCFDecodeRuntimeException, TribbleException, read_bcf_header
from .formats import Configuration, IllegalArgumentException, IOException, SeekableFile, context, raise_for
from .sam_text import spliced_pieces
from .vcf import VCFFormat, VCFRecord, read_vcf_header

OUTPUT_VCF_FORMAT_PROPERTY = "hadoopbam.vcf.output-format"
WRITE_HEADER_PROPERTY = "hadoopbam.vcf.write-header"
_FLUSH_BYTES = 256 << 20  # host record bytes buffered before a device render
_MISSING_FLOAT = 0x7F800001
_W = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
_PACK = {1: "b", 2: "h", 3: "i", 5: "I"}
_INT_MISSING = {1: -0x80, 2: -0x8000, 3: -0x80000000}


class VCFUnsupportedException(RuntimeError):
    """HBAM_EUNSUPPORTED out of the VCF renderer: a DP or GQ vector whose length is not 1."""


def _fail(code, msg):
    if code == _lib.HBAM_ETRIBBLE:
        raise TribbleException(msg)
    if code == _lib.HBAM_ERUNTIME:
        raise BCFDecodeRuntimeException(msg)
    if code == _lib.HBAM_EUNSUPPORTED:
        raise VCFUnsupportedException(msg)
    raise_for(code, msg)


# ---- the header --------------------------------------------------------------------------------------
def _line_attr(line, name):
    """name=value inside ##XXX=<...>: name directly behind '<' or ','; the value ends at ',' or '>'
    (as bcf_header_text in hbam_bcf_api.hip reads ID)."""
    start = 0
    while True:
        i = line.find(name + b"=", start)
        if i < 0:
            return None
        if i and line[i - 1:i] in (b"<", b","):
            rest = line[i + len(name) + 1:]
            j = min([x for x in (rest.find(b","), rest.find(b">")) if x >= 0] or [len(rest)])
            return rest[:j]
        start = i + 1


class VCFHeader:
    """What the renderer needs of a VCF header: the text as it stands, the contigs (the ##contig IDs
    in line order), the samples (the #CHROM line's columns behind FORMAT), the string dictionary in
    the order bcf_header_text (hbam_bcf_api.hip) builds it (PASS, then the FILTER / INFO / FORMAT IDs
    by first occurrence) and the INFO / FORMAT lines' Number and Type."""

    def __init__(self, text):
        self.text = bytes(text)
        self.contigs, self.samples, self.dictionary = [], [], [b"PASS"]
        self.info, self.format = {}, {}
        for line in self.text.split(b"\n"):
            if line.startswith(b"##contig=<"):
                self.contigs.append(_line_attr(line, b"ID") or b"")
            elif line.startswith((b"##FILTER=<", b"##INFO=<", b"##FORMAT=<")):
                ident = _line_attr(line, b"ID")
                if ident is None:
                    continue
                if ident != b"PASS" and ident not in self.dictionary:
                    self.dictionary.append(ident)
                table = self.info if line.startswith(b"##INFO") else self.format if line.startswith(b"##FORMAT") else None
                if table is not None:
                    table.setdefault(ident, (_line_attr(line, b"Number"), _line_attr(line, b"Type")))
            elif line.startswith(b"#CHROM"):
                self.samples = line.rstrip(b"\r").split(b"\t")[9:]
        order = sorted(range(len(self.dictionary)), key=lambda i: self.dictionary[i])
        self.rank = [0] * len(order)
        for r, i in enumerate(order):
            self.rank[i] = r
        self.counts = {"n_contig": len(self.contigs), "n_sample": len(self.samples), "n_dict": len(self.dictionary)}
        self._meta = None

    def info_flag(self, ident):
        """the INFO line is Type=Flag or Number=0: the entry is written as KEY alone"""
        number, typ = self.info[ident]
        return typ == b"Flag" or number == b"0"

    def format_kind(self, ident):
        return ident.decode("latin-1") if ident in (b"GT", b"DP", b"GQ", b"AD", b"PL", b"FT") else "generic"

    def meta(self):
        """hbam_vcf_meta as host arrays (Context.vcf_render's `meta`)."""
        if self._meta is None:
            def cat(names):
                off = np.zeros(len(names) + 1, np.uint32)
                off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
                return np.frombuffer(b"".join(names) or b"\0", np.uint8), off
            flags = np.zeros(max(len(self.dictionary), 1), np.uint32)
            number = np.zeros(max(len(self.dictionary), 1), np.int32)
            for i, ident in enumerate(self.dictionary):
                f = 0
                if ident in self.info:
                    f |= _lib.HBAM_VCF_HAS_INFO | (_lib.HBAM_VCF_INFO_FLAG if self.info_flag(ident) else 0)
                if ident in self.format:
                    f |= _lib.HBAM_VCF_HAS_FORMAT
                    f |= _lib.HBAM_VCF_KINDS.get(self.format_kind(ident), 0) << _lib.HBAM_VCF_KIND_SHIFT
                    num = (self.format[ident][0] or b".").decode("latin-1")
                    number[i] = _lib.HBAM_VCF_NUMBER[num] if num in _lib.HBAM_VCF_NUMBER else int(num)
                flags[i] = f
            cn, co = cat(self.contigs)
            dn, do = cat(self.dictionary)
            self._meta = {"contig_names": cn, "contig_off": co, "dict_names": dn, "dict_off": do,
                          "dict_rank": np.array(self.rank or [0], np.uint32), "dict_flags": flags,
                          "dict_number": number}
        return self._meta


def read_vcf_header_from(path_or_bytes, ctx=None):
    """VCFHeaderReader.readHeaderFrom: the header of a BCF file (BGZF or plain, its text through
    hbam_bcf_header_text) or of a text VCF file -> VCFHeader."""
    ss = SeekableFile(path_or_bytes)
    try:
        if ss.read_at(0, 1) == b"#":
            return VCFHeader(read_vcf_header(ss, str(path_or_bytes)[:80])[0])
        ctx = ctx or context(None)
        n = min(ss.length, 1 << 20)
        while True:
            t = ctx.bcf_header_text(ss.read_at(0, n))
            if not isinstance(t, int):
                return VCFHeader(t)
            if t != _lib.HBAM_EMORE or n >= ss.length:
                _fail(t, "cannot read the BCF header")
            n = min(ss.length, 4 * n)
    finally:
        ss.close()


# ---- the host renderer ---------------------------------------------------------------------------------
class _Bytes:
    """A block of the record: typed values are read in order, every extent checked against its end."""

    def __init__(self, rec, at, end):
        self.b, self.at, self.end = rec, at, end

    def descriptor(self, mult=1):
        """-> (type, count); the cursor stands at the first value"""
        if self.at >= self.end:
            raise TribbleException("a typed value past its block")
        d = self.b[self.at]
        self.at += 1
        t, k = d & 15, d >> 4
        if k == 15:
            if self.at >= self.end:
                raise TribbleException("a typed value past its block")
            t2 = self.b[self.at] & 15
            self.at += 1
            if t2 not in _INT_MISSING:
                raise BCFDecodeRuntimeException("a count that is no integer")
            if self.end - self.at < _W[t2]:
                raise TribbleException("a typed value past its block")
            k = max(struct.unpack_from("<" + _PACK[t2], self.b, self.at)[0], 0)
            self.at += _W[t2]
        if k:
            if t not in _W:
                raise BCFDecodeRuntimeException("unknown value type %d" % t)
            if k * _W[t] * mult > self.end - self.at:
                raise TribbleException("a typed value past its block")
        return t, k

    def raw(self, t, k):
        """k raw values of type t: ints, float bit patterns, or the bytes of a string"""
        if k == 0:
            v = b"" if t == 7 else ()
        elif t == 7:
            v = self.b[self.at:self.at + k]
        else:
            v = struct.unpack_from("<%d%s" % (k, _PACK[t]), self.b, self.at)
        self.at += k * _W.get(t, 0)
        return v

    def key(self, n_dict):
        t, k = self.descriptor()
        if k != 1 or t not in _INT_MISSING:
            raise BCFDecodeRuntimeException("a dictionary key that is no single integer")
        v = self.raw(t, 1)[0]
        if not 0 <= v < n_dict:
            raise BCFDecodeRuntimeException("dictionary offset %d" % v)
        return v


class _Float:
    def __init__(self, bits):
        self.bits = bits

    @property
    def value(self):
        return struct.unpack("<f", struct.pack("<I", self.bits))[0]

    def on_device(self):
        """the device's domain for an INFO float: +-0, and 0.01 <= v < 10^7"""
        if self.bits & 0x7fffffff == 0:
            return True
        v = self.value
        return self.bits >> 31 == 0 and v == v and 0.01 <= v < 1e7


def _decimal_fixed(d, places):
    return format(Decimal(d).quantize(Decimal(10) ** -places, rounding=ROUND_HALF_UP), "f")


def _nonfinite(d):
    return "NaN" if d != d else "Infinity" if d == float("inf") else "-Infinity" if d == float("-inf") else None


def format_vcf_double(d):
    """htsjdk's formatVCFDouble with %-formats done in decimal, HALF_UP (Java's Formatter rounds
    HALF_UP).  A NaN is not below 1: it takes %.2f, which prints NaN."""
    if _nonfinite(d):
        return _nonfinite(d)
    if d >= 1:
        return _decimal_fixed(d, 2)
    if d >= 0.01:
        return _decimal_fixed(d, 3)
    if abs(d) < 1e-20:
        return "0.00"
    x = Decimal(d)
    exp = abs(x).adjusted()
    mant = abs(x).scaleb(-exp).quantize(Decimal("0.001"), rounding=ROUND_HALF_UP)
    if mant >= 10:
        exp += 1
        mant = (mant / 10).quantize(Decimal("0.001"), rounding=ROUND_HALF_UP)
    return "%s%se%s%02d" % ("-" if x < 0 else "", format(mant, "f"), "-" if exp < 0 else "+", abs(exp))


def format_qual(bits):
    if bits == _MISSING_FLOAT:
        return "."
    d = (_Float(bits).value / -10.0) * -10.0 + 0.0
    s = _nonfinite(d) or _decimal_fixed(d, 2)
    return s[:-3] if s.endswith(".00") else s


def _qual_on_device(bits):
    if bits == _MISSING_FLOAT:
        return True
    q = _Float(bits).value
    if bits >> 31 or q != q or q >= 1e7:
        return False
    return not ((8 * q) % 2 == 1)


def _decode(t, raw):
    """decodeTypedValue: None, an int, a _Float, bytes, or a list of ints / _Floats"""
    if t == 7:
        s = bytes(raw).rstrip(b"\0")
        if not s:
            return None
        return s[1:] if s[:1] == b"," else s
    if t == 5:
        vals = [_Float(x) for x in raw if x != _MISSING_FLOAT]
    else:
        vals = [x for x in raw if x != _INT_MISSING[t]]
    if not vals:
        return None
    return vals[0] if len(raw) == 1 else vals


def _int_array(t, raw):
    out = []
    for x in raw:
        if x == _INT_MISSING[t]:
            break
        out.append(x)
    return out or None


def _text(v):
    """formatVCFField"""
    if v is None:
        return "."
    if isinstance(v, list):
        return ",".join(_text(x) for x in v)
    if isinstance(v, _Float):
        return format_vcf_double(v.value)
    if isinstance(v, bytes):
        return v.decode("latin-1")
    return "%d" % v


def _floats_on_device(v):
    return all(x.on_device() for x in (v if isinstance(v, list) else [v]) if isinstance(x, _Float))


class _Record:
    """One record decoded and checked, in the order hbam_vcf_render checks it."""

    def __init__(self, rec, header):
        H = self.header = header
        rec = bytes(rec)
        if len(rec) < 8:
            raise TribbleException("a record cut inside its lengths")
        ls, li = struct.unpack_from("<ii", rec, 0)
        if ls < 24 or li < 0 or 8 + ls + li > len(rec):
            raise TribbleException("a record that runs past the bytes given")
        self.chrom, pos, _, self.qual, nai, nfs = struct.unpack_from("<iiiIII", rec, 8)
        self.pos1 = ((pos + 1 + 0x80000000) & 0xffffffff) - 0x80000000
        self.n_allele, n_info = nai >> 16, nai & 0xffff
        self.n_sample, n_fmt = nfs & 0xffffff, nfs >> 24
        if not 0 <= self.chrom < len(H.contigs):
            raise BCFDecodeRuntimeException("CHROM %d outside the contigs" % self.chrom)
        if self.n_sample != len(H.samples) or self.n_allele < 1:
            raise TribbleException("sample or allele count")
        nd = len(H.dictionary)
        s = _Bytes(rec, 32, 8 + ls)

        def a_string(what):
            t, k = s.descriptor()
            if k and t != 7:
                raise BCFDecodeRuntimeException("%s is no string" % what)
            return bytes(s.raw(7, k)).rstrip(b"\0")
        self.ident = a_string("ID")
        self.alleles = []
        for _ in range(self.n_allele):
            a = a_string("an allele")
            if not a:
                raise BCFDecodeRuntimeException("an empty allele")
            self.alleles.append(a)
        t, k = s.descriptor()
        if k and t not in _INT_MISSING:
            raise BCFDecodeRuntimeException("FILTER is no integer vector")
        self.filters = list(s.raw(t, k))
        if any(not 0 <= e < nd for e in self.filters):
            raise BCFDecodeRuntimeException("FILTER offset outside the dictionary")
        self.info, self.n_info, self.info_repeated = {}, n_info, False
        for _ in range(n_info):
            key = s.key(nd)
            if H.dictionary[key] not in H.info:
                raise TribbleException("INFO key %r without a header line" % H.dictionary[key])
            t, k = s.descriptor()
            self.info_repeated |= key in self.info
            self.info[key] = _decode(t, s.raw(t, k)) if k else None
        # the genotype fields: (key, kind, type, count, [raw values per sample])
        g = _Bytes(rec, 8 + ls, 8 + ls + li)
        self.fields, self.gt = [], None
        for f in range(n_fmt):
            key = g.key(nd)
            ident = H.dictionary[key]
            if ident not in H.format:
                raise BCFDecodeRuntimeException("FORMAT key %r without a header line" % ident)
            t, k = g.descriptor(self.n_sample)
            kind, ints = H.format_kind(ident), (k == 0 or t in _INT_MISSING)
            if kind == "GT":
                if not ints or self.gt is not None:
                    raise BCFDecodeRuntimeException("GT of another type, or twice")
                self.gt = f
            elif kind in ("DP", "GQ"):
                if k != 1:
                    raise VCFUnsupportedException("%s vector of length %d" % (kind, k))
                if not ints:
                    raise BCFDecodeRuntimeException("%s is no integer" % kind)
            elif kind in ("AD", "PL") and not ints:
                raise BCFDecodeRuntimeException("%s is no integer vector" % kind)
            self.fields.append((key, kind, t, k, [g.raw(t, k) for _ in range(self.n_sample)]))
        # the samples
        self.values = []
        for key, kind, t, k, rows in self.fields:
            if kind in ("GT", "AD", "PL"):
                col = [_int_array(t, r) for r in rows]
            elif kind in ("DP", "GQ"):
                col = [None if r[0] == _INT_MISSING[t] else r[0] for r in rows]
            else:
                col = [_decode(t, r) if k else None for r in rows]
            self.values.append(col)
        if self.gt is not None:
            for call in self.values[self.gt]:
                if any(not 0 <= (e >> 1) <= self.n_allele for e in call or ()):
                    raise BCFDecodeRuntimeException("a GT allele outside the record's alleles")
        self.keys = sorted((f for f in range(n_fmt) if f != self.gt and any(v is not None for v in self.values[f])),
                           key=lambda f: (H.rank[self.fields[f][0]], f))
        self.gt_key = False
        if self.n_sample:
            self.gt_key = not self.keys or (self.gt is not None and any(v is not None for v in self.values[self.gt]))
            if self.gt_key and (self.gt is None or any(v is None for v in self.values[self.gt])):
                raise BCFDecodeRuntimeException("GT is a FORMAT key and a sample has none")

    def should_defer(self):
        """The one deferral predicate: what hbam_vcf_render leaves to the host (include/hbam.h)."""
        H = self.header
        if not _qual_on_device(self.qual):
            return True
        if len(self.filters) > _lib.HBAM_VCF_MAX_FILTER or self.n_info > _lib.HBAM_VCF_MAX_INFO or self.info_repeated:
            return True
        if any(not _floats_on_device(v) for k, v in self.info.items() if not H.info_flag(H.dictionary[k])):
            return True
        if len(self.fields) > _lib.HBAM_VCF_MAX_FORMAT:
            return True
        for f, (key, kind, t, k, _) in enumerate(self.fields):
            if kind == "FT" or (k and t in (5, 7)) or (kind == "GT" and k > _lib.HBAM_VCF_MAX_PLOIDY):
                return True
            if kind == "generic" and H.format[H.dictionary[key]][0] == b"G" and f in self.keys and \
                    any(v is None for v in self.values[f]):
                return True
        return False

    def _null_text(self, f):
        key, kind = self.fields[f][:2]
        n = 1
        if kind == "generic":
            number = self.header.format[self.header.dictionary[key]][0] or b"."
            n = {b"A": self.n_allele - 1, b"R": self.n_allele, b".": 1, b"G": 1}.get(number)
            n = int(number) if n is None else n
        return ",".join("." * max(n, 1))

    def line(self):
        H = self.header
        sym = lambda a: (a[:1] == b"<" and a[-1:] == b">") or b"[" in a or b"]" in a or a[:1] == b"." or a[-1:] == b"."  # noqa: E731
        alleles = [a if sym(a) else a.upper() for a in self.alleles]
        flt = sorted(set(self.filters), key=lambda e: H.rank[e])
        info = []
        for key in sorted(self.info, key=lambda e: H.rank[e]):
            ident = H.dictionary[key]
            text = "" if H.info_flag(ident) else _text(self.info[key])
            info.append(ident.decode("latin-1") + ("=" + text if text else ""))
        cols = [H.contigs[self.chrom].decode("latin-1"), "%d" % self.pos1, self.ident.decode("latin-1") or ".",
                alleles[0].decode("latin-1"), b",".join(alleles[1:]).decode("latin-1") or ".", format_qual(self.qual),
                ";".join(H.dictionary[e].decode("latin-1") for e in flt) or ".", ";".join(info) or "."]
        if self.n_sample:
            cols.append(":".join((["GT"] if self.gt_key else []) +
                                 [H.dictionary[self.fields[f][0]].decode("latin-1") for f in self.keys]))
            for s in range(self.n_sample):
                vals = [self._null_text(f) if self.values[f][s] is None else _text(self.values[f][s]) for f in self.keys]
                while vals and not vals[-1].replace(".", "").replace(",", ""):
                    vals.pop()
                if self.gt_key:
                    call = self.values[self.gt][s]
                    vals.insert(0, ("|" if call[0] & 1 else "/").join("." if e >> 1 == 0 else "%d" % ((e >> 1) - 1) for e in call))
                cols.append(":".join(vals))
        return "\t".join(cols).encode("latin-1") + b"\n"


def render_record(record_bytes, header):
    """One BCF2 record (l_shared | l_indiv | site | genotypes) -> its VCF line with the '\\n', by the
    full rule list of hbam_vcf_render (include/hbam.h): the host renderer of the lines the device
    defers, every float and FORMAT type included.  Numbers are formatted with `decimal`, HALF_UP.
    TribbleException / BCFDecodeRuntimeException / VCFUnsupportedException where the device reports
    HBAM_ETRIBBLE / HBAM_ERUNTIME / HBAM_EUNSUPPORTED."""
    return _Record(record_bytes, header).line()


def should_defer(record_bytes, header):
    """Whether hbam_vcf_render defers this (valid) record to render_record."""
    return _Record(record_bytes, header).should_defer()


# ---- writers ---------------------------------------------------------------------------------------------
def _addr(p):
    import ctypes as C
    if p is None or isinstance(p, int):
        return p or 0
    if hasattr(p, "data_ptr"):
        return int(p.data_ptr())
    return int(C.cast(p, C.c_void_p).value or 0)


class VCFRecordWriter:
    """VCFRecordWriter.java: a VCF text part.  The header text is written as it stands when
    write_header is true, as vcf_sort does: htsjdk's re-serialised header (VCFWriter.writeHeader's own
    ordering and added lines) is not restated.  Records are BCF2 records: host ones are buffered and
    rendered on the device in batches, a decode's device columns are rendered where they stand
    (write_device); only the text and a deferred record's bytes cross to the host.  A VCFRecord (a
    text line) would need re-encoding through VCFCodec, which is not restated."""

    def __init__(self, output, header, write_header=True, ctx=None):
        self._own = isinstance(output, (str, os.PathLike))
        self.orig = open(output, "wb") if self._own else output
        self._ctx = ctx
        self.header = header
        self.buf, self.sizes = bytearray(), []
        if write_header:
            self.writeHeader(header)

    @property
    def ctx(self):  # the device is opened when the first record is rendered
        if self._ctx is None:
            self._ctx = context(None)
        return self._ctx

    def writeHeader(self, header):
        self.orig.write(header.text)

    def write(self, key, value):  # KeyIgnoringVCFRecordWriter.write: the key is ignored
        if isinstance(value, VCFRecord):
            raise NotImplementedError("a text VCF record is not re-encoded: write BCF records")
        self.write_encoded(value.toBCFBytes())

    def write_encoded(self, raw):
        """Already-encoded BCF2 records, back to back, in order."""
        raw = bytes(raw)
        p = 0
        while p < len(raw):
            if len(raw) - p < 8:
                raise TribbleException("a record cut inside its lengths")
            ls, li = struct.unpack_from("<ii", raw, p)
            if ls < 0 or li < 0 or p + 8 + ls + li > len(raw):
                raise TribbleException("a record runs past the bytes given")
            self.sizes.append(8 + ls + li)
            p += 8 + ls + li
        self.buf += raw
        if len(self.buf) >= _FLUSH_BYTES:
            self._flush()

    def _emit(self, res, record_at):
        """The render's text with the deferred lines spliced in; the first failing record in output
        order ends the output, whether the device or the host renderer found it."""
        if res["rc"]:
            raise_for(res["rc"], res.get("error", ""))
        for piece in spliced_pieces(res, lambda k: render_record(record_at(k), self.header)):
            self.orig.write(piece)
        if res["status"] != _lib.HBAM_OK:
            _fail(res["status"], "record %d of the batch" % res["err_record"])

    def _flush(self):
        if not self.sizes:
            return
        ro = np.zeros(len(self.sizes) + 1, np.uint64)
        ro[1:] = np.cumsum(self.sizes, dtype=np.uint64)
        buf = bytes(self.buf)
        self.buf, self.sizes = bytearray(), []
        res = self.ctx.vcf_render(buf, len(buf), ro[:-1], len(ro) - 1, self.header.counts, self.header.meta(),
                                  on_device=False)
        self._emit(res, lambda k: buf[int(ro[k]):int(ro[k + 1])])

    def write_device(self, cols, perm=None, n=None):
        """The records of a BCF decode left on the device (Context.bcf_decode_split_device's struct, or
        a dict with data, data_len, rec_off and n_records); perm: device u32 indices, line k = record
        perm[k]; n: the lines to write (default: every record)."""
        self._flush()
        get = (lambda k: cols[k]) if isinstance(cols, dict) else (lambda k: getattr(cols, k))
        data, data_len, rec_off = _addr(get("data")), int(get("data_len")), _addr(get("rec_off"))
        n = int(get("n_records")) if n is None else int(n)
        perm = None if perm is None else _addr(perm)
        res = self.ctx.vcf_render(data, data_len, rec_off, n, self.header.counts, self.header.meta(), perm=perm,
                                  on_device=True)

        def record_at(k):
            i = int(self.ctx._d2h(perm + 4 * k, 1, np.uint32)[0]) if perm is not None else k
            o = int(self.ctx._d2h(rec_off + 8 * i, 1, np.uint64)[0])
            ls, li = self.ctx._d2h(data + o, 2, np.uint32)
            return self.ctx._d2h(data + o, 8 + int(ls) + int(li), np.uint8).tobytes()
        self._emit(res, record_at)
        return res

    def close(self, ctx=None):
        self._flush()
        self.orig.flush()
        if self._own:
            self.orig.close()


class KeyIgnoringVCFRecordWriter(VCFRecordWriter):
    """KeyIgnoringVCFRecordWriter.java: writes only the value of (key, VariantContextWritable)."""


# ---- output formats ------------------------------------------------------------------------------------
def _format_value_of(s):
    """VCFFormat.valueOf: IllegalArgumentException for any other name."""
    if s not in (VCFFormat.VCF, VCFFormat.BCF):
        raise IllegalArgumentException("No enum constant VCFFormat.%s" % s)
    return s


class VCFOutputFormat:
    """VCFOutputFormat.java: built from a Configuration (hadoopbam.vcf.output-format read by
    VCFFormat.valueOf, None when unset) or from a VCFFormat (None: IllegalArgumentException)."""
    OUTPUT_VCF_FORMAT_PROPERTY = OUTPUT_VCF_FORMAT_PROPERTY

    def __init__(self, conf_or_fmt):
        if isinstance(conf_or_fmt, dict):
            s = conf_or_fmt.get(OUTPUT_VCF_FORMAT_PROPERTY)
            self.format = None if s is None else _format_value_of(s)
        else:
            if conf_or_fmt is None:
                raise IllegalArgumentException("null VCFFormat")
            self.format = _format_value_of(conf_or_fmt)


class KeyIgnoringVCFOutputFormat(VCFOutputFormat):
    """KeyIgnoringVCFOutputFormat.java:55-117.  (fmt), (conf) and (conf, path): without the property
    the second raises, the third infers the format from the path's extension."""
    WRITE_HEADER_PROPERTY = WRITE_HEADER_PROPERTY

    def __init__(self, conf_or_fmt, path=None):
        super().__init__(conf_or_fmt)
        self.conf = conf_or_fmt if isinstance(conf_or_fmt, dict) else Configuration()
        self.header = None
        if self.format is None:
            if path is None:
                raise IllegalArgumentException("unknown VCF format: OUTPUT_VCF_FORMAT_PROPERTY not set")
            self.format = VCFFormat.inferFromFilePath(path)
            if self.format is None:
                raise IllegalArgumentException("unknown VCF format: %s" % path)

    def getHeader(self):
        return self.header

    def setHeader(self, header):
        self.header = header

    def readHeaderFrom(self, path, conf=None, ctx=None):
        self.header = read_vcf_header_from(path, ctx or context(conf or self.conf))

    def getRecordWriter(self, out, conf=None, ctx=None):
        if self.header is None:
            raise IOException("Can't create a RecordWriter without the VCF header")
        conf = self.conf if conf is None else conf
        # Configuration.getBoolean: "true" / "false" in any case, anything else is the default (true)
        v = str(conf.get(WRITE_HEADER_PROPERTY, "")).strip().lower()
        write_header = {"true": True, "false": False}.get(v, True)
        if self.format == VCFFormat.BCF:
            raise NotImplementedError("BCFRecordWriter is not restated: VCF text output only")
        return KeyIgnoringVCFRecordWriter(out, self.header, write_header, ctx)
