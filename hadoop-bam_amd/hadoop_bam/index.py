"""BAI index build and indexed region queries over the MI355X C ABI.

Mirrors the reference's Index plugin (cli/plugins/Index.java:61-127: every record fed to [htsjdk]
BAMIndexer, which writes <file>.bai) and the region branch of its View plugin
(cli/plugins/View.java:164-221: reader.queryOverlapping(name, beg, end) per region argument).

The index is built on the device from the columns of a whole-file decode (hbam_bai_build); a
query decodes only the chunks the index names (hbam_decode_split over their virtual-offset ranges),
filters the records on the device (hbam_overlap_filter) and copies the kept records alone to the
host.  Reading a .bai and choosing the chunks of a region (BAMIndex) is host code.

htsjdk is not in the reference tree: its rules are restated from memory here and in
csrc/hbam_bai.hip, parity unpinned (DESIGN.md lists them)."""
import os
import re
import struct

import numpy as np

from . import _lib
from .consumers import _raise  # raise_for, with HBAM_EINDEX as consumers.IndexOutOfBoundsException
from .formats import BAMRecordBytes, IllegalArgumentException, IOException, SAMFormatException

BAI_MAGIC = b"BAI\x01"
META_BIN = 37450       # [htsjdk] GenomicIndexUtil.MAX_BINS: the metadata pseudo-bin
LINEAR_SHIFT = 14      # 16 KiB windows
_MAX_POS = 0x1FFFFFFF  # positions a BAI can index (2^29 - 1)
_LEVEL_BASE = (0, 1, 9, 73, 585, 4681)


def reg2bins(beg, end):
    """The bins that may hold a read overlapping the 0-based half-open range [beg, end)
    (SAM spec 5.3; [htsjdk] GenomicIndexUtil.regionToBins), ascending."""
    end -= 1
    out = [0]
    for lvl, shift in ((1, 26), (2, 23), (3, 20), (4, 17), (5, 14)):
        out.extend(range(_LEVEL_BASE[lvl] + (beg >> shift), _LEVEL_BASE[lvl] + (end >> shift) + 1))
    return out


def linear_window(p):
    """[htsjdk] LinearIndex.convertToLinearIndexOffset of a 1-based position."""
    return (0 if p <= 0 else p - 1) >> LINEAR_SHIFT


def same_or_adjacent(a, b):
    """[htsjdk] BlockCompressedFilePointerUtil.areInSameOrAdjacentBlocks (the + 1 is on the byte
    address of the BGZF block)."""
    return (a >> 16) == (b >> 16) or (a >> 16) + 1 == (b >> 16)


class _Reference:
    __slots__ = ("bins", "meta", "linear")

    def __init__(self):
        self.bins = {}     # bin -> [(beg, end), ...] in file order
        self.meta = None   # (first offset, last offset, aligned, unaligned)
        self.linear = np.zeros(0, np.uint64)


class BAMIndex:
    """A parsed .bai ([htsjdk] AbstractBAMFileIndex / CachingBAMFileIndex)."""

    def __init__(self, raw):
        raw = bytes(raw)
        if raw[:4] != BAI_MAGIC:
            raise SAMFormatException("Invalid file header in BAM index: %r" % raw[:4])
        p = 4

        def take(fmt):
            nonlocal p
            n = struct.calcsize(fmt)
            if p + n > len(raw):
                raise SAMFormatException("Premature end of BAM index at byte %d" % p)
            v = struct.unpack_from(fmt, raw, p)
            p += n
            return v

        (n_ref,) = take("<i")
        if n_ref < 0:
            raise SAMFormatException("Negative reference count in BAM index")
        self.refs = []
        for _ in range(n_ref):
            r = _Reference()
            (n_bin,) = take("<i")
            if n_bin < 0:
                raise SAMFormatException("Negative bin count in BAM index")
            for _ in range(n_bin):
                b, n_chunk = take("<Ii")
                if n_chunk < 0 or p + 16 * n_chunk > len(raw):
                    raise SAMFormatException("Premature end of BAM index at byte %d" % p)
                v = np.frombuffer(raw, "<u8", 2 * n_chunk, p)
                p += 16 * n_chunk
                chunks = [(int(v[2 * k]), int(v[2 * k + 1])) for k in range(n_chunk)]
                if b == META_BIN and n_chunk == 2:
                    r.meta = (chunks[0][0], chunks[0][1], chunks[1][0], chunks[1][1])
                else:
                    r.bins[b] = chunks
            (n_intv,) = take("<i")
            if n_intv < 0 or p + 8 * n_intv > len(raw):
                raise SAMFormatException("Premature end of BAM index at byte %d" % p)
            r.linear = np.frombuffer(raw, "<u8", n_intv, p).astype(np.uint64)
            p += 8 * n_intv
            self.refs.append(r)
        rest = len(raw) - p
        if rest == 0:
            self.n_no_coor = None  # older writers leave it out
        elif rest >= 8:
            (self.n_no_coor,) = take("<Q")
        else:
            raise SAMFormatException("Premature end of BAM index at byte %d" % p)

    def to_bytes(self):
        """The .bai serialisation ([htsjdk] BinaryBAMIndexWriter), bins in ascending number."""
        out = [BAI_MAGIC, struct.pack("<i", len(self.refs))]
        for r in self.refs:
            out.append(struct.pack("<i", len(r.bins) + (1 if r.meta is not None else 0)))
            for b in sorted(r.bins):
                out.append(struct.pack("<Ii", b, len(r.bins[b])))
                out.extend(struct.pack("<QQ", beg, end) for beg, end in r.bins[b])
            if r.meta is not None:
                out.append(struct.pack("<IiQQQQ", META_BIN, 2, *r.meta))
            out.append(struct.pack("<i", len(r.linear)))
            out.append(r.linear.astype("<u8").tobytes())
        if self.n_no_coor is not None:
            out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)

    def span_overlapping(self, ref, beg=0, end=0):
        """[htsjdk] getSpanOverlapping(referenceIndex, startPos, endPos) (1-based inclusive; <= 0:
        from the first base / to the end): the merged, sorted, disjoint chunks [(vbeg, vend), ...]
        that hold every record overlapping the region."""
        if ref < 0 or ref >= len(self.refs):
            return []
        r = self.refs[ref]
        b0 = 0 if beg <= 0 else beg - 1
        e0 = _MAX_POS if end <= 0 else min(end, _MAX_POS)
        if b0 >= e0:
            if b0 > _MAX_POS:
                return []
            e0 = b0 + 1
        chunks = []
        for b in reg2bins(b0, e0):
            chunks.extend(r.bins.get(b, ()))
        if not chunks:
            return []
        w = linear_window(beg)
        min_off = int(r.linear[w]) if w < len(r.linear) else 0
        chunks = sorted(c for c in chunks if c[1] > min_off)
        out = []
        for cb, ce in chunks:
            if out and (cb <= out[-1][1] or same_or_adjacent(out[-1][1], cb)):
                if ce > out[-1][1]:
                    out[-1][1] = ce
            else:
                out.append([cb, ce])
        return [(a, b) for a, b in out]


def _load(src):
    """(uint8 array or memmap, path or None)"""
    if isinstance(src, (str, os.PathLike)):
        path = os.fspath(src)
        if os.path.getsize(path) == 0:
            return np.zeros(0, np.uint8), path
        return np.memmap(path, np.uint8, "r"), path
    if isinstance(src, np.ndarray):
        return np.ascontiguousarray(src, dtype=np.uint8), None
    return np.frombuffer(bytes(src), np.uint8), None


class BAMIndexer:
    """The Index plugin (cli/plugins/Index.java:61-127) on the device: index(bam) builds the .bai
    of a BAM file given as a path or as bytes."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def index(self, bam, out_path=None):
        ctx = self.ctx or _lib.Context(0)
        data, path = _load(bam)
        rc, bai, err = ctx.bai_index(np.asarray(data))
        if rc:
            _raise(rc, ctx.last_error() if err is None else "%s (record %d)" % (ctx.last_error(), err))
        if out_path is None and path is not None:
            out_path = path + ".bai"
        if out_path is not None:
            with open(out_path, "wb") as f:
                f.write(bai)
        return bai


def parse_region(header, region):
    """A region argument of the View plugin, "name", "name:beg-end" (View.java:179-212) ->
    (reference index, beg, end); a bare name gives beg = end = 0.  The string is cut at ':' and '-'
    as StringTokenizer(region, ":-") does; a coordinate is what Integer.parseInt accepts and must
    not be negative (View.parseCoordinate :239-249, which takes no thousands separators); a begin
    without an end is refused (end = -1, :186-191); the name is looked up in the dictionary first,
    then read as an index into it (:202-205).  Raises IllegalArgumentException where View reports
    the region as an error."""
    tok = [t for t in re.split("[:-]", str(region)) if t]
    if not tok:
        raise IllegalArgumentException("Empty region")

    def coordinate(s):
        if not re.fullmatch(r"[+-]?[0-9]+", s) or not -(1 << 31) <= int(s) < (1 << 31) or int(s) < 0:
            raise IllegalArgumentException("Not a valid coordinate: '%s'" % s)
        return int(s)

    beg = end = 0
    if len(tok) > 1:
        beg = coordinate(tok[1])
        if len(tok) < 3:
            raise IllegalArgumentException("Not a valid coordinate: '' (a range needs its end)")
        end = coordinate(tok[2])
        if end < beg:
            raise IllegalArgumentException("Invalid range, cannot end before start: '%d-%d'" % (beg, end))
    names = [n.decode("latin-1") if isinstance(n, bytes) else str(n) for n, _ in header.getSequenceDictionary()]
    name = tok[0]
    if name in names:
        return names.index(name), beg, end
    if re.fullmatch(r"[+-]?[0-9]+", name) and 0 <= int(name) < len(names):
        return int(name), beg, end
    raise IllegalArgumentException("Not a valid sequence name or index: '%s'" % name)


class IndexedBAMReader:
    """[htsjdk] SamReader.queryOverlapping / queryContained over a BAM and its .bai, as View.java
    :214-218 uses them.  `bam` is a path or the file's bytes; `index` a BAMIndex or .bai bytes, by
    default <path>.bai (then <path minus .bam>.bai).  A query returns the records in file order as
    BAMRecordBytes, each with its virtual offset in .voffset; last_query holds what the query read."""

    def __init__(self, bam, ctx=None, index=None):
        self.ctx = ctx or _lib.Context(0)
        self.data, self.path = _load(bam)
        if index is None:
            if self.path is None:
                raise IOException("Cannot query a BAM lacking an index")
            cands = [self.path + ".bai"]
            if self.path.endswith(".bam"):
                cands.append(self.path[:-4] + ".bai")
            found = [p for p in cands if os.path.exists(p)]
            if not found:
                raise IOException("Cannot query a BAM file lacking an index: %s" % self.path)
            with open(found[0], "rb") as f:
                index = f.read()
        self.index = index if isinstance(index, BAMIndex) else BAMIndex(index)
        self.header = self._read_header()
        self.names = [n.decode("latin-1") for n, _ in self.header.getSequenceDictionary()]
        self.n_ref = len(self.names)
        self.last_query = {}

    def _read_header(self):
        """SAMHeaderReader.readSAMHeaderFrom from the file's first BGZF blocks alone (whatever
        follows them, a cut file included, is not looked at): parsed and inflated on the device."""
        from .output import SAMFileHeader
        data, k = self.data, min(len(self.data), 1 << 20)
        while True:
            h = self.ctx.parse_header(data[:k])
            if isinstance(h, dict) or k >= len(data):
                break
            k = min(len(data), 4 * k)
        if not isinstance(h, dict):
            _raise(h, "cannot read SAM header")
        blocks, have = [], 0
        for b in _lib.bgzf_blocks(data[:k]):
            blocks.append(b)
            have += b[2]
            if have >= h["header_ulen"]:
                break
        sub = {x: np.array([b[j] for b in blocks]) for j, x in enumerate(("coff", "clen", "isize", "crc"))}
        rc, u, _, _ = self.ctx.inflate(data[:k], sub, check_crc=False)
        if rc:
            _raise(rc, self.ctx.last_error())
        return SAMFileHeader.from_bam_bytes(u[:int(h["header_ulen"])].tobytes())

    def _reference(self, ref):
        if isinstance(ref, (int, np.integer)):
            if not 0 <= int(ref) < self.n_ref:
                raise IllegalArgumentException("Reference index %d not found in sequence dictionary." % ref)
            return int(ref)
        name = ref.decode("latin-1") if isinstance(ref, bytes) else str(ref)
        if name not in self.names:
            raise IllegalArgumentException("Unknown reference sequence '%s'" % name)
        return self.names.index(name)

    def query_overlapping(self, ref, beg=0, end=0):
        return self._query(ref, beg, end, False)

    def query_contained(self, ref, beg=0, end=0):
        return self._query(ref, beg, end, True)

    def query_region(self, region, contained=False):
        """A View region argument (parse_region) -> the records."""
        r, beg, end = parse_region(self.header, region)
        return self._query(r, beg, end, contained)

    def _decode_chunk(self, vbeg, vend):
        """Device columns of the records in [vbeg, vend): the window starts at vbeg's BGZF block and
        ends with vend's; a last record running past it (HBAM_EMORE) widens the window."""
        flen = len(self.data)

        def block_end(off):  # BSIZE of the BGZF block at off
            if off + 18 > flen:
                return flen
            return min(flen, off + (int(self.data[off + 16]) | int(self.data[off + 17]) << 8) + 1)

        cb = vbeg >> 16
        ce = block_end(vend >> 16)
        while True:
            rc, d = self.ctx.decode_split_device(self.data[cb:ce], vbeg, vend, self.n_ref, comp_base=cb,
                                                 file_len=flen)
            if rc:
                _raise(rc, self.ctx.last_error())
            self.last_query["comp_bytes"] += ce - cb
            if int(d.status) != _lib.HBAM_EMORE:
                return d
            if ce >= flen:  # the chunk runs past the end of the file: the file is cut short
                _raise(_lib.HBAM_ETRUNC, "chunk %#x-%#x ends past the end of the file" % (vbeg, vend))
            self.last_query["widened"] += 1
            for _ in range(4):  # a read of up to ~250 kB of blocks more per round
                ce = block_end(ce)

    def query_columns(self, ref, beg=0, end=0, contained=False):
        """The query on the device, chunk by chunk: yields (d, k, idx) per index chunk, d the device
        columns of the chunk's decode and idx a device u32 list of the k records of d that overlap
        (or are contained in) the region, ascending (hbam_overlap_filter): what hbam_gather_records
        and hbam_sam_render take as perm.  All three are valid until the next chunk is asked for.  A
        chunk whose decode ended in a status raises it once the chunk has been handed out."""
        r = self._reference(ref)
        chunks = self.index.span_overlapping(r, beg, end)
        self.last_query = {"chunks": chunks, "comp_bytes": 0, "decoded_records": 0, "widened": 0}
        for vbeg, vend in chunks:
            d = self._decode_chunk(vbeg, vend)
            self.last_query["decoded_records"] += int(d.n_records)
            k, idx = self.ctx.overlap_filter(d, r, beg, end, contained)
            try:
                yield d, k, idx
            finally:
                self.ctx.L.hbam_device_free(self.ctx.h, idx)
            st = int(d.status)  # never HBAM_EMORE here: _decode_chunk widens or raises
            if st != _lib.HBAM_OK:
                _raise(st, "at record %d of chunk %#x-%#x" % (int(d.n_records), vbeg, vend))

    def _query(self, ref, beg, end, contained):
        out = []
        for d, k, idx in self.query_columns(ref, beg, end, contained):
            voff, payload, off = self.ctx.gather_to_host(d, idx, k)
            for j in range(k):
                rec = BAMRecordBytes(payload[int(off[j]):int(off[j + 1])].tobytes())
                rec.voffset = int(voff[j])
                out.append(rec)
        return out
