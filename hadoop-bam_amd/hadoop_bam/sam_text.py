"""SAM text output over the MI355X C ABI: SAMRecordWriter (SAMRecordWriter.java),
KeyIgnoringSAMRecordWriter, AnySAMOutputFormat (AnySAMOutputFormat.java:46-57),
KeyIgnoringAnySAMOutputFormat (KeyIgnoringAnySAMOutputFormat.java:61-139) and the View plugin's
default job (cli/plugins/View.java:85-222), same names, argument meaning and exceptions.

The lines are rendered on the device (hbam_sam_render, hbam_samtext.hip) from packed BAM records:
htsjdk's SAMTextWriter.writeAlignment, restated from memory (htsjdk is not in the reference tree:
parity unpinned, DESIGN.md lists the rules).  The device hands a record to the host when it holds
an H tag or a float whose Float.toString is not trivially exact: render_record writes that line and
the writer splices it in.  java_float_to_string is Float.toString as JDK 19 and later print it
(unpinned)."""
import os
import struct
import sys
from fractions import Fraction

import numpy as np

from . import _lib
from ._window import read_growing_window
from .formats import Configuration, IllegalArgumentException, IOException, SAMFormatException, context, raise_for
from .output import KeyIgnoringBAMRecordWriter, read_sam_header
from .sam import SAMFormat, read_sam_text_header

OUTPUT_SAM_FORMAT_PROPERTY = "hadoopbam.anysam.output-format"
WRITE_HEADER_PROPERTY = "hadoopbam.anysam.write-header"
_FLUSH_BYTES = 256 << 20  # host record bytes buffered before a device render
_SEQ = b"=ACMGRSVTWYHKDBN"
_OPS = b"MIDNSHP=X"
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


# ---- Float.toString ----------------------------------------------------------------------------
def _exp10(v):
    """e with 10^e <= v < 10^(e + 1)"""
    e = 0
    while Fraction(10) ** (e + 1) <= v:
        e += 1
    while Fraction(10) ** e > v:
        e -= 1
    return e


def _shortest_digits(bits):
    """(digits, e): the fewest decimal digits d1 d2 ... with d1.d2... x 10^e reading back as the
    positive finite float32 `bits`, the closest such to its value; exact (fractions)."""
    ex, m = (bits >> 23) & 0xff, bits & 0x7fffff
    if ex == 0:
        num, sh = m, -149
    else:
        num, sh = m | 0x800000, ex - 150
    v = Fraction(num) * Fraction(2) ** sh
    # the reals that round to v: half a step each way (a power of two has the shorter step below),
    # the ends included when the mantissa is even
    up = Fraction(2) ** sh / 2
    down = up / 2 if (m == 0 and ex > 1) else up
    lo, hi, closed = v - down, v + up, (m & 1) == 0
    e = _exp10(v)
    for nd in range(1, 10):
        scale = Fraction(10) ** (e - nd + 1)
        q = v / scale
        f = q.numerator // q.denominator
        # the decimals of this length on either side of v: at a power of two the interval is
        # lopsided, and the farther one may be the only one inside it
        inside = [d for d in (f, f + 1)
                  if lo < d * scale < hi or (closed and (d * scale == lo or d * scale == hi))]
        if inside:
            d = min(inside, key=lambda d: (abs(d * scale - v), d & 1))  # the closest; a tie: the even one
            s, ee = str(d), e
            if len(s) > nd:  # rounded up to the next power of ten
                ee += 1
            return s.rstrip("0") or "0", ee
    raise AssertionError("nine digits always round-trip a float32")


def java_float_to_string(bits):
    """Float.toString of the float32 with these bits, in Java's layout (JDK 19+ behaviour,
    unpinned): NaN, Infinity, -Infinity; plain decimal for 1e-3 <= |v| < 1e7, else d.dddE[-]x; at
    least one digit after the point; the shortest digits that read back as the same float32, and
    where one digit would do, the value rounded to two."""
    bits &= 0xffffffff
    sign = "-" if bits >> 31 else ""
    mag = bits & 0x7fffffff
    if mag > 0x7f800000:
        return "NaN"
    if mag == 0x7f800000:
        return sign + "Infinity"
    if mag == 0:
        return sign + "0.0"
    digits, e = _shortest_digits(mag)
    if len(digits) == 1:
        v = Fraction(struct.unpack("<f", struct.pack("<I", mag))[0])  # float32 -> double is exact
        e = _exp10(v)  # (the one digit may be the 1 of the next power of ten: 9.8E-45, not 1.0E-44)
        q = v / Fraction(10) ** (e - 1)
        d = q.numerator // q.denominator
        if q - d >= Fraction(1, 2):
            d += 1
        s = str(d)
        if len(s) > 2:
            e += 1
        digits = s.rstrip("0") or "0"
    if -3 <= e < 7:
        if e >= 0:
            whole, frac = digits[:e + 1].ljust(e + 1, "0"), digits[e + 1:]
        else:
            whole, frac = "0", "0" * (-e - 1) + digits
        return sign + whole + "." + (frac or "0")
    return sign + digits[0] + "." + (digits[1:] or "0") + "E%d" % e


# ---- the host renderer (deferred lines) ----------------------------------------------------------
def _tag_text(rec, p, end):
    """The tags rec[p:end] -> [b"XX:T:value"]."""
    out = []
    while p < end:
        if end - p < 3:
            raise SAMFormatException("a tag runs past the record")
        tag, t = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if t == "A":
            if p >= end:
                raise SAMFormatException("a tag runs past the record")
            out.append(tag + b":A:" + rec[p:p + 1])
            p += 1
        elif t in _INT or t == "f":
            w = 4 if t == "f" else struct.calcsize(_INT[t])
            if end - p < w:
                raise SAMFormatException("a tag runs past the record")
            if t == "f":
                out.append(tag + b":f:" + java_float_to_string(struct.unpack_from("<I", rec, p)[0]).encode())
            else:
                out.append(tag + b":i:%d" % struct.unpack_from(_INT[t], rec, p)[0])
            p += w
        elif t in "ZH":
            z = rec.find(b"\0", p, end)
            if z < 0:
                raise SAMFormatException("a %s tag without its NUL" % t)
            out.append(tag + b":" + t.encode() + b":" + rec[p:z])
            p = z + 1
        elif t == "B":
            if end - p < 5:
                raise SAMFormatException("a tag runs past the record")
            sub, cnt = chr(rec[p]), struct.unpack_from("<i", rec, p + 1)[0]
            if sub not in _INT and sub != "f":
                raise SAMFormatException("unknown B subtype %r" % sub)
            w = 4 if sub == "f" else struct.calcsize(_INT[sub])
            p += 5
            if cnt < 0 or w * cnt > end - p:
                raise SAMFormatException("a B array runs past the record")
            if sub == "f":
                vals = [java_float_to_string(x).encode() for x in struct.unpack_from("<%dI" % cnt, rec, p)]
            else:
                vals = [b"%d" % x for x in struct.unpack_from("<%d%s" % (cnt, _INT[sub][1]), rec, p)]
            out.append(tag + b":B:" + b",".join([sub.encode()] + vals))
            p += w * cnt
        else:
            raise SAMFormatException("unknown tag type %r" % t)
    return out


def render_record(record_bytes, names):
    """One BAM record (block_size + record) -> its SAM line with the '\\n', by the rules of
    hbam_sam_render (include/hbam.h) with every float as java_float_to_string: the host renderer of
    the lines the device defers.  names = the dictionary names (bytes).  SAMFormatException /
    IllegalArgumentException where the device reports HBAM_EFORMAT / HBAM_EREFID."""
    rec = bytes(record_bytes)
    if len(rec) < 36:
        raise SAMFormatException("a record shorter than its fixed fields")
    bs, ref, pos, lrn, mapq, _, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    if bs < 32 or 4 + bs > len(rec) or lrn == 0 or lseq < 0:
        raise SAMFormatException("malformed record")
    if bs < 32 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq:
        raise SAMFormatException("block_size shorter than the record's fields")
    if not (-1 <= ref < len(names) and -1 <= nref < len(names)):
        raise IllegalArgumentException("reference index not in the dictionary")
    end = 4 + bs
    p = 36 + lrn
    ops = struct.unpack_from("<%dI" % ncig, rec, p)
    if any(w & 15 > 8 for w in ops):
        raise IllegalArgumentException("unknown CIGAR operator")
    p += 4 * ncig
    cigar = b"".join(b"%d%c" % (w >> 4, _OPS[w & 15]) for w in ops) or b"*"
    if lseq == 0:
        seq = qual = b"*"
    else:
        packed = np.frombuffer(rec, np.uint8, (lseq + 1) // 2, p)
        nib = np.empty(2 * len(packed), np.uint8)
        nib[0::2], nib[1::2] = packed >> 4, packed & 15
        seq = np.frombuffer(_SEQ, np.uint8)[nib[:lseq]].tobytes()
        q = np.frombuffer(rec, np.uint8, lseq, p + (lseq + 1) // 2)
        if q[0] == 0xff:
            qual = b"*"
        elif int(q.max()) > 93:
            raise IllegalArgumentException("quality value above 93")
        else:
            qual = (q + 33).astype(np.uint8).tobytes()
    p += (lseq + 1) // 2 + lseq
    i32 = lambda x: ((x + (1 << 31)) & 0xffffffff) - (1 << 31)  # noqa: E731
    rname = names[ref] if ref >= 0 else b"*"
    rnext = b"=" if (nref >= 0 and nref == ref) else (names[nref] if nref >= 0 else b"*")
    cols = [rec[36:36 + lrn - 1], b"%d" % flag, bytes(rname), b"%d" % i32(pos + 1), b"%d" % mapq, cigar,
            bytes(rnext), b"%d" % i32(npos + 1), b"%d" % tlen, seq, qual] + _tag_text(rec, p, end)
    return b"\t".join(cols) + b"\n"


def spliced_pieces(res, render_at):
    """The pieces of a render's host copy (Context.sam_render's or vcf_render's dict) in output
    order: the device's text up to each deferred line, then render_at(k) for that line's output
    position k, then the rest."""
    text, lo, at = res["text"], res["line_off"], 0
    for k in res["deferred"]:
        cut = int(lo[int(k)])
        yield text[at:cut]
        yield render_at(int(k))
        at = cut
    yield text[at:]


def splice(res, record_at, names):
    """The host copy of a render (Context.sam_render's dict) with its deferred lines filled in:
    record_at(k) = the bytes of the record of output position k."""
    if not len(res["deferred"]):
        return res["text"]
    return b"".join(spliced_pieces(res, lambda k: render_record(record_at(k), names)))


def header_text(header):
    """The text a SAM file begins with: header.text with a final '\\n', and @SQ lines from the
    dictionary when the text has none."""
    lines = [ln for ln in header.text.split(b"\n") if ln.startswith(b"@")]
    if not any(ln.startswith(b"@SQ") for ln in lines):
        lines += [b"@SQ\tSN:%s\tLN:%d" % (n, ln) for n, ln in header.refs]
    return b"".join(ln + b"\n" for ln in lines)


# ---- writers -------------------------------------------------------------------------------------
class SAMRecordWriter:
    """SAMRecordWriter.java: a SAM text part; the header text is written when write_header.  Host
    records are buffered and rendered on the device in batches; records already on the device
    (write_device) are rendered where they stand."""

    def __init__(self, output, header, write_header=True, ctx=None):
        self._own = isinstance(output, (str, os.PathLike))
        self.orig = open(output, "wb") if self._own else output
        self.ctx = ctx or _lib.Context(0)
        self.header = header
        self.names = [n for n, _ in header.refs]
        self.buf, self.sizes = bytearray(), []
        if write_header:
            self.writeHeader(header)

    def writeHeader(self, header):
        self.orig.write(header_text(header))

    def writeAlignment(self, rec):
        self.write_encoded(rec.toBAMBytes())

    def write(self, key, value):  # KeyIgnoringSAMRecordWriter.write: the key is ignored
        self.writeAlignment(value.get())

    def write_encoded(self, raw):
        """Already-encoded records (block_size-prefixed BAM records), in order."""
        raw = bytes(raw)
        p = 0
        while p < len(raw):
            if len(raw) - p < 4:
                raise SAMFormatException("a record cut inside its block_size")
            n = 4 + struct.unpack_from("<i", raw, p)[0]
            if n < 4 or p + n > len(raw):
                raise SAMFormatException("a record runs past the bytes given")
            self.sizes.append(n)
            p += n
        self.buf += raw
        if len(self.buf) >= _FLUSH_BYTES:
            self._flush()

    def _emit(self, res, record_at):
        if res["rc"]:
            raise_for(res["rc"], res.get("error", ""))
        self.orig.write(splice(res, record_at, self.names))
        if res["status"] != _lib.HBAM_OK:
            raise_for(res["status"], "record %d of the batch" % res["err_record"])

    def _flush(self):
        if not self.sizes:
            return
        ro = np.zeros(len(self.sizes) + 1, np.uint64)
        ro[1:] = np.cumsum(self.sizes, dtype=np.uint64)
        buf = bytes(self.buf)
        self.buf, self.sizes = bytearray(), []
        res = self.ctx.sam_render(buf, ro, len(ro) - 1, self.names, on_device=False)
        self._emit(res, lambda k: buf[int(ro[k]):int(ro[k + 1])])

    def write_device(self, ubuf, rec_off, n, perm=None):
        """n records on the device (device pointers: a decode's ubuf / rec_off, a sorted run's
        payload / offsets; perm: device u32 indices, line k = record perm[k]).  Only a deferred
        record's bytes cross to the host."""
        self._flush()
        keep = None
        if hasattr(ubuf, "data_ptr"):  # a torch tensor: the 64 readable bytes behind it (Context._ptr)
            p, _, _, keep = self.ctx._ptr(ubuf)
            ubuf = int(p.value or 0)
        rec_off, perm = _addr(rec_off), (None if perm is None else _addr(perm))
        res = self.ctx.sam_render(ubuf, rec_off, n, self.names, perm=perm, on_device=True)

        def record_at(k):
            i = int(self.ctx._d2h(_addr(perm) + 4 * k, 1, np.uint32)[0]) if perm is not None else k
            o = self.ctx._d2h(_addr(rec_off) + 8 * i, 2, np.uint64)
            return self.ctx._d2h(_addr(ubuf) + int(o[0]), int(o[1] - o[0]), np.uint8).tobytes()
        self._emit(res, record_at)
        del keep

    def close(self, ctx=None):
        self._flush()
        self.orig.flush()
        if self._own:
            self.orig.close()


def _addr(p):
    """A device pointer as an int (an int, a ctypes pointer or a torch tensor)."""
    import ctypes as C
    if isinstance(p, int):
        return p
    if hasattr(p, "data_ptr"):
        return int(p.data_ptr())
    return int(C.cast(p, C.c_void_p).value or 0)


class KeyIgnoringSAMRecordWriter(SAMRecordWriter):
    """KeyIgnoringSAMRecordWriter.java: writes only the value of (key, SAMRecordWritable)."""


# ---- output formats -------------------------------------------------------------------------------
def _format_value_of(s):
    """SAMFormat.valueOf: IllegalArgumentException for any other name."""
    if s not in (SAMFormat.SAM, SAMFormat.BAM):
        raise IllegalArgumentException("No enum constant SAMFormat.%s" % s)
    return s


class AnySAMOutputFormat:
    """AnySAMOutputFormat.java:46-57: built from a Configuration (hadoopbam.anysam.output-format read
    by SAMFormat.valueOf, None when unset) or from a SAMFormat (None: IllegalArgumentException)."""
    OUTPUT_SAM_FORMAT_PROPERTY = OUTPUT_SAM_FORMAT_PROPERTY

    def __init__(self, conf_or_fmt):
        if isinstance(conf_or_fmt, dict):
            s = conf_or_fmt.get(OUTPUT_SAM_FORMAT_PROPERTY)
            self.format = None if s is None else _format_value_of(s)
        else:
            if conf_or_fmt is None:
                raise IllegalArgumentException("null SAMFormat")
            self.format = _format_value_of(conf_or_fmt)


class KeyIgnoringAnySAMOutputFormat(AnySAMOutputFormat):
    """KeyIgnoringAnySAMOutputFormat.java:61-139.  (fmt), (conf) and (conf, path): without the
    property the second raises, the third infers the format from the path's extension."""
    WRITE_HEADER_PROPERTY = WRITE_HEADER_PROPERTY

    def __init__(self, conf_or_fmt, path=None):
        super().__init__(conf_or_fmt)
        self.conf = conf_or_fmt if isinstance(conf_or_fmt, dict) else Configuration()
        self.header = None
        self.writeHeader_ = True
        if self.format is None:
            if path is None:
                raise IllegalArgumentException("unknown SAM format: OUTPUT_SAM_FORMAT_PROPERTY not set")
            self.format = SAMFormat.inferFromFilePath(path)
            if self.format is None:
                raise IllegalArgumentException("unknown SAM format: %s" % path)

    def getWriteHeader(self):
        return self.writeHeader_

    def setWriteHeader(self, b):
        self.writeHeader_ = bool(b)

    def getSAMHeader(self):
        return self.header

    def setSAMHeader(self, header):
        self.header = header

    def readSAMHeaderFrom(self, path, conf=None, ctx=None):
        self.header = _read_any_header(path, ctx or context(conf or self.conf))

    def getRecordWriter(self, out, conf=None, ctx=None):
        if self.header is None:
            raise IOException("Can't create a RecordWriter without the SAM header")
        conf = self.conf if conf is None else conf
        # Configuration.getBoolean: "true" / "false" in any case, anything else is the default
        v = str(conf.get(WRITE_HEADER_PROPERTY, "")).strip().lower()
        write_header = {"true": True, "false": False}.get(v, self.writeHeader_)
        if self.format == SAMFormat.BAM:
            return KeyIgnoringBAMRecordWriter(out, self.header, write_header, ctx)
        return KeyIgnoringSAMRecordWriter(out, self.header, write_header, ctx)


def _read_any_header(path, ctx):
    """SAMHeaderReader.readSAMHeaderFrom for either format (by the first byte)."""
    with open(path, "rb") as f:
        first = f.read(1)
    if first == b"\x1f":
        return read_sam_header(path, ctx)
    return read_sam_text_header(path)[2]


# ---- View ------------------------------------------------------------------------------------------
VIEW_WINDOW_BYTES = 1 << 30    # a BAM is decoded in windows of this many compressed bytes
VIEW_SPLIT_BYTES = 256 << 20   # a SAM file in FileSplits of this many bytes


def _bam_header(path, ctx):
    """SAMHeaderReader.readSAMHeaderFrom over a growing prefix of the file -> (SAMFileHeader, the
    first record's virtual offset): the header's BGZF blocks are inflated on the device."""
    from .output import SAMFileHeader
    flen = os.path.getsize(path)
    k = min(flen, 1 << 20)
    with open(path, "rb") as f:
        while True:
            f.seek(0)
            data = np.frombuffer(f.read(k), np.uint8)
            h = ctx.parse_header(data)
            blocks, have = [], 0
            if isinstance(h, dict):
                for b in _lib.bgzf_blocks(data):
                    blocks.append(b)
                    have += b[2]
                    if have >= h["header_ulen"]:
                        break
                if have >= h["header_ulen"]:
                    break
            if k >= flen:
                break
            k = min(flen, 4 * k)
    if not isinstance(h, dict):
        raise_for(h, ctx.last_error() or "cannot read the SAM header")
    if have < h["header_ulen"]:
        raise_for(_lib.HBAM_ETRUNC, "the file ends inside its header")
    sub = {x: np.array([b[j] for b in blocks]) for j, x in enumerate(("coff", "clen", "isize", "crc"))}
    rc, u, _, _ = ctx.inflate(data, sub, check_crc=False)
    if rc:
        raise_for(rc, ctx.last_error())
    return SAMFileHeader.from_bam_bytes(u[:int(h["header_ulen"])].tobytes()), int(h["first_voffset"])


def _view_bam(ctx, path, header, first_voffset, w):
    """The whole BAM as one split, streamed window by window from positioned reads of the file
    (hbam_split_open_reader): each window's device columns are rendered where they stand."""
    with open(path, "rb") as f:
        flen, fd = os.path.getsize(path), f.fileno()
        d = None
        for d in ctx.split_stream_reader(lambda off, n: os.pread(fd, n, off), flen, first_voffset,
                                         (flen << 16) | 0xffff, len(header.refs), VIEW_WINDOW_BYTES, host=False):
            w.write_device(d.ubuf, d.rec_off, int(d.n_records))
        if d is not None and int(d.status) != _lib.HBAM_OK:  # the last window carries the split's status
            raise_for(int(d.status), "record %d of the last window" % int(d.n_records))


def _view_sam(ctx, path, header, data_start, w):
    """The SAM file split by split (SAMInputFormat's FileSplits; the first one covers the header):
    only a split's window is read, its lines become records on the device and are rendered there."""
    from .formats import SeekableFile
    from .sam import SAM_WINDOW_TAIL
    ss = SeekableFile(path)
    try:
        names = [n for n, _ in header.refs]
        table = ctx.vcf_contig_table(names)
        start = 0
        while start < ss.length:
            length = min(ss.length - start, max(VIEW_SPLIT_BYTES, data_start + 1 - start))

            def call(window, base):  # the columns left on the device
                rc, d = ctx.sam_decode_split_device(window, start, length, data_start, table, len(names),
                                                    text_base=base, file_len=ss.length)
                if rc:
                    raise_for(rc, ctx.last_error())
                return d

            base = min(start - 1 if start else data_start, ss.length)
            d, _ = read_growing_window(ss, base, start, length, SAM_WINDOW_TAIL, call)
            w.write_device(d.ubuf, d.rec_off, int(d.n_records))
            if int(d.status) != _lib.HBAM_OK:  # HBAM_EMORE with the whole rest of the file in the window too
                raise_for(int(d.status), "line %d of the split at %d" % (int(d.n_records), start))
            start += length
    finally:
        ss.close()


def view(path, regions=(), out=None, header_only=False, fmt=None, conf=None):
    """cli/plugins/View.java:85-222: print a SAM or BAM file, or regions of an indexed BAM, as SAM
    text to `out` (a binary stream; stdout by default).  -> the plugin's return code: 0; 1 for fmt
    BAM (no longer supported there either); 4 when the file cannot be opened, parsed or read to its
    end, regions are asked of a SAM file, or the BAM has no index; 5 when some region was invalid,
    after the valid ones were written.  The records stay on the device and only the windows asked
    for are read: a BAM is streamed window by window, a SAM file decoded split by split, and each
    decode's columns are rendered where they stand; a region goes through the index chunks and
    hbam_overlap_filter (IndexedBAMReader.query_columns), whose index list is the renderer's perm."""
    from .index import IndexedBAMReader, parse_region
    out = out if out is not None else sys.stdout.buffer
    err = sys.stderr
    ctx = context(conf)
    try:
        with open(path, "rb") as f:
            binary = SAMFormat.inferFromData(f.read(1)) == SAMFormat.BAM
    except Exception as e:  # noqa: BLE001 - View.java catches Exception here
        err.write("view :: Could not open '%s': %s\n" % (path, e))
        return 4
    data_start = first_voffset = 0
    try:
        if binary:
            header, first_voffset = _bam_header(path, ctx)
        else:
            _, data_start, header = read_sam_text_header(path)
    except Exception as e:  # noqa: BLE001
        err.write("view :: Could not parse '%s': %s\n" % (path, e))
        return 4
    if (SAMFormat.SAM if fmt is None else _format_value_of(str(fmt).upper())) == SAMFormat.BAM:
        err.write("BAM output inside view no longer supported\n")
        return 1
    w = SAMRecordWriter(out, header, True, ctx)
    if not regions or header_only:
        if not header_only:
            try:
                if binary:
                    _view_bam(ctx, path, header, first_voffset, w)
                else:
                    _view_sam(ctx, path, header, data_start, w)
            except Exception as e:  # noqa: BLE001
                w.close()
                err.write("view :: Failed to read '%s': %s\n" % (path, e))
                return 4
        w.close()
        return 0
    if not binary:
        err.write("view :: Cannot output regions from SAM file\n")
        return 4
    try:
        reader = IndexedBAMReader(str(path), ctx)
    except IOException:
        err.write("view :: Cannot output regions from BAM file lacking an index\n")
        return 4
    errors = False
    for region in regions:
        try:
            r, beg, end = parse_region(header, region)
        except IllegalArgumentException as e:
            err.write("view :: %s\n" % e)
            errors = True
            continue
        try:
            for d, k, idx in reader.query_columns(r, beg, end):
                w.write_device(d.ubuf, d.rec_off, k, idx)
        except Exception as e:  # noqa: BLE001
            w.close()
            err.write("view :: Failed to read '%s': %s\n" % (path, e))
            return 4
    w.close()
    return 5 if errors else 0
