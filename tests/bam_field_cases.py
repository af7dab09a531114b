"""Crafted BAM records for the fixed-field, key and pool decode (k_decode_fixed, k_decode_pools and
the k_scan4_* offset scans in csrc/hbam_kernels.hip; k_gather_records_tile in csrc/hbam_sort.hip).

A record is laid out from explicit pieces (Rec: the name bytes as given, the CIGAR words, the packed
SEQ bytes, QUAL, aux, the fixed fields) and the builder keeps the pieces, so every case carries its
own expectation, independent of the oracle and of helpers.oracle_pools: the pools are the pieces in
record order (SEQ as "=ACMGRSVTWYHKDBN"[nibble]), the offset columns their running sums over the
layout_ok records, the keys a plain-Python reading of BAMRecordReader.getKey (java_key).

The cases (each a function returning a Case; their structure is asserted on the CPU in
test_bam_fields_model.py, the device runs them in test_bam_fields_gpu.py):
  length_grid     every segment at every length 0..49 (name also 254, 255; n_cigar 0..13)
  prefixes        the first n records of length_grid: partial last tiles, a one-lane tile
  murmur_lengths  unplaced unmapped records with every variable-block length 0..287
  key_edges       the branches of the key: pos -1, -2, 0x7fffffff, 0x7ffffffe, flag 4, refID -1
  unit_boundary   a record of 65535 / 65537 sixteen-byte units at lane 0, 32 or 63 of its tile
  field_major     tiles that take k_decode_pools' field-major loop
  empty_tiles     tiles without units, tiles that begin with records without units
"""
import functools
import struct

import numpy as np

import chain_craft as cc
from helpers import bgzf_pack
from sam_ref import murmur_bytes

SEQ_ALPHA = "=ACMGRSVTWYHKDBN"
_ALPHA = np.frombuffer(SEQ_ALPHA.encode(), np.uint8)
N_REF = cc.N_REF
FIXED = ("block_size", "ref_id", "pos", "l_read_name", "mapq", "bin", "n_cigar", "flag", "l_seq",
         "next_ref_id", "next_pos", "tlen")
POOLS = (("names", np.uint8), ("cigars", np.uint32), ("seq", np.uint8), ("qual", np.uint8), ("aux", np.uint8))
OFFS = ("name_off", "cigar_off", "seq_off", "aux_off")


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def _i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def hash_key(var):
    """getKey0(Integer.MAX_VALUE, (int)murmurhash3(var, 0)): the int is sign-extended into the OR."""
    return _i64(0x7fffffff << 32 | (_i32(murmur_bytes(var, 0)) & (1 << 64) - 1))


def java_key(ref, pos, flag, var):
    """BAMRecordReader.getKey(SAMRecord) :66-106 for an undecoded BAM record, in Java's int and long
    arithmetic: getAlignmentStart() is pos + 1 (int), getKey(refIdx, start) is
    (long)refIdx << 32 | start - 1 with the int start - 1 sign-extended."""
    start = _i32(pos + 1)
    if not ((flag & 4) or ref < 0 or start < 0):
        return _i64(_i64(ref << 32) | (_i32(start - 1) & (1 << 64) - 1))
    return hash_key(var)


class Rec:
    """One record from its pieces.  n_cigar / l_seq: what the fixed fields claim where that is not
    what the pieces hold (the layout check then has to fail: such a record has no pool entries)."""

    def __init__(self, name=b"", cigar=(), seq=b"", l_seq=0, qual=b"", aux=b"", ref=0, pos=0, mapq=0, bin_=0,
                 flag=0, nref=-1, npos=-1, tlen=0, claim_n_cigar=None, claim_l_seq=None):
        assert len(name) <= 255 and len(seq) == (l_seq + 1) // 2 and len(qual) == l_seq
        self.name, self.cigar, self.seq, self.qual, self.aux = bytes(name), tuple(cigar), bytes(seq), bytes(qual), bytes(aux)
        self.var = self.name + struct.pack("<%dI" % len(self.cigar), *self.cigar) + self.seq + self.qual + self.aux
        self.n_cigar = len(self.cigar) if claim_n_cigar is None else claim_n_cigar
        self.l_seq = l_seq if claim_l_seq is None else claim_l_seq
        self.ref, self.pos, self.mapq, self.bin, self.flag = ref, pos, mapq, bin_, flag
        self.nref, self.npos, self.tlen = nref, npos, tlen
        self.block_size = 32 + len(self.var)
        need = len(self.name) + 4 * self.n_cigar + (self.l_seq + 1) // 2 + self.l_seq
        self.layout_ok = int(self.l_seq >= 0 and need <= len(self.var))
        if claim_n_cigar is not None or claim_l_seq is not None:
            assert not self.layout_ok, "a claim that fits is a different record, not a bad layout"
        self.bytes = struct.pack("<iiiBBHHHiiii", self.block_size, ref, pos, len(self.name), mapq, bin_, self.n_cigar,
                                 flag, self.l_seq, nref, npos, tlen) + self.var
        self.key = java_key(ref, pos, flag, self.var)

    def bases(self):
        b = np.frombuffer(self.seq, np.uint8)
        nib = np.stack([b >> 4, b & 15], 1).reshape(-1)[:len(self.qual)]
        return _ALPHA[nib]

    # 16-byte units per field, as k_decode_pools counts them (L = name, 4 n_cigar, l_seq, l_seq, aux)
    def field_lens(self):
        if not self.layout_ok:
            return (0, 0, 0, 0, 0)
        return (len(self.name), 4 * len(self.cigar), len(self.qual), len(self.qual), len(self.aux))

    def units(self):
        return tuple((n + 15) >> 4 for n in self.field_lens())


class Case:
    def __init__(self, recs, notes=None):
        self.recs = list(recs)
        self.notes = notes or {}
        head = cc.bam_header()
        self.header_len = len(head)
        self.u = head + b"".join(r.bytes for r in self.recs)
        self.data = np.frombuffer(bgzf_pack(self.u), np.uint8).copy()
        assert self.header_len < 65280
        self.v_start = self.header_len           # block 0, offset header_len
        self.v_end = len(self.data) << 16 | 0xffff

    @functools.cached_property
    def expect(self):
        rs = self.recs
        ok = [r for r in rs if r.layout_ok]
        e = dict(n=len(rs), layout_ok=np.array([r.layout_ok for r in rs], np.uint8),
                 key=np.array([r.key for r in rs], np.int64))
        for k, a in (("block_size", "block_size"), ("ref_id", "ref"), ("pos", "pos"), ("mapq", "mapq"), ("bin", "bin"),
                     ("n_cigar", "n_cigar"), ("flag", "flag"), ("l_seq", "l_seq"), ("next_ref_id", "nref"),
                     ("next_pos", "npos"), ("tlen", "tlen")):
            e[k] = np.array([getattr(r, a) for r in rs], np.int64)
        e["l_read_name"] = np.array([len(r.name) for r in rs], np.int64)
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        e["names"] = np.frombuffer(b"".join(r.name for r in ok), np.uint8)
        e["cigars"] = np.array([w for r in ok for w in r.cigar], np.uint32)
        e["seq"] = cat([r.bases() for r in ok], np.uint8)
        e["qual"] = np.frombuffer(b"".join(r.qual for r in ok), np.uint8)
        e["aux"] = np.frombuffer(b"".join(r.aux for r in ok), np.uint8)
        for off, i in zip(OFFS, (0, 1, 2, 4)):
            lens = [(len(r.name), len(r.cigar), len(r.qual), 0, len(r.aux))[i] if r.layout_ok else 0 for r in rs]
            e[off] = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)
        return e

    def payload(self, order):
        """SAMRecordWritable bytes (block_size field + record) of the records `order`, and their offsets"""
        b = [self.recs[i].bytes for i in order]
        return b"".join(b), np.concatenate([[0], np.cumsum([len(x) for x in b], dtype=np.uint64)]).astype(np.uint64)


# ---- pieces ---------------------------------------------------------------------------------------------
def _name(rng, n):
    """n name bytes, NUL-terminated as a writer would (nothing here depends on it)"""
    if n == 0:
        return b""
    return bytes(rng.integers(0x21, 0x7f, n - 1, dtype=np.uint8)) + b"\0"


def _cigar(rng, n):
    return tuple(int(x) for x in rng.integers(0, 1 << 32, n, dtype=np.uint64))


def _blob(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _rec(rng, name, n_cigar, l_seq, aux, **fixed):
    """Placed and mapped unless `fixed` says otherwise; every byte of every segment random."""
    f = dict(ref=int(rng.integers(0, N_REF)), pos=int(rng.integers(0, 1 << 30)), mapq=int(rng.integers(0, 256)),
             bin_=int(rng.integers(0, 1 << 16)), flag=int(rng.integers(0, 1 << 16)) & ~4,
             nref=int(rng.integers(-1, N_REF)), npos=int(rng.integers(-1, 1 << 30)),
             tlen=int(rng.integers(-(1 << 31), 1 << 31)))
    f.update(fixed)
    return Rec(_name(rng, name), _cigar(rng, n_cigar), _blob(rng, (l_seq + 1) // 2), l_seq, _blob(rng, l_seq),
               _blob(rng, aux), **f)


def min_rec(rng, **fixed):
    """block_size 32: no name, no CIGAR, no bases, no aux"""
    return _rec(rng, 0, 0, 0, 0, **fixed)


# ---- length_grid ------------------------------------------------------------------------------------------
GRID_SEGMENTS = ("name", "cigar", "seq", "qual", "aux")
GRID_LENGTHS = dict(name=list(range(50)) + [254, 255], cigar=list(range(14)), seq=list(range(50)),
                    qual=list(range(50)), aux=list(range(50)))


@functools.lru_cache(None)
def grid_records():
    """(records, what): what[i] = (segment, length) the record was added for.  The other segments
    take seeded lengths in 0..40 (n_cigar 0..10); fixed shuffle."""
    rng = np.random.default_rng(1301)
    recs, what = [], []
    for seg in GRID_SEGMENTS:
        for n in GRID_LENGTHS[seg]:
            ln = dict(name=int(rng.integers(0, 41)), cigar=int(rng.integers(0, 11)), seq=int(rng.integers(0, 41)),
                      aux=int(rng.integers(0, 41)))
            ln["seq" if seg == "qual" else seg] = n
            recs.append(_rec(rng, ln["name"], ln["cigar"], ln["seq"], ln["aux"]))
            what.append((seg, n))
    order = np.random.default_rng(1302).permutation(len(recs))
    return tuple(recs[i] for i in order), tuple(what[i] for i in order)


@functools.lru_cache(None)
def length_grid():
    return Case(grid_records()[0])


PREFIXES = (1, 63, 64, 65, 129)


@functools.lru_cache(None)
def prefixes(n):
    return Case(grid_records()[0][:n])


# ---- murmur_lengths ---------------------------------------------------------------------------------------
MURMUR_MAX = 16 * 17 + 15


def _split_var(rng, v):
    """(name, n_cigar, l_seq, aux) lengths that fill a variable block of v bytes exactly"""
    name = int(rng.integers(0, min(v, 40) + 1))
    v -= name
    n_cigar = int(rng.integers(0, min(v // 4, 6) + 1))
    v -= 4 * n_cigar
    l_seq = int(rng.integers(0, 2 * v // 3 + 1))
    while l_seq + (l_seq + 1) // 2 > v:
        l_seq -= 1
    return name, n_cigar, l_seq, v - l_seq - (l_seq + 1) // 2


@functools.lru_cache(None)
def murmur_lengths(last_tail):
    """Flag 4, refID -1, pos -1: the key hashes the whole variable block, whose length runs over
    0..287 (block counts 0..17 times tails 0..15).  last_tail 0 / 15: the stream's last record has
    17 blocks and that tail, so the tail loads (and, tail 0, all 16 bytes of them) lie behind it."""
    assert last_tail in (0, 15)
    rng = np.random.default_rng(1310 + last_tail)
    lens = [int(x) for x in rng.permutation(MURMUR_MAX + 1)]
    last = 16 * 17 + last_tail
    lens.remove(last)
    lens.append(last)
    recs = []
    for v in lens:
        name, n_cigar, l_seq, aux = _split_var(rng, v)
        recs.append(_rec(rng, name, n_cigar, l_seq, aux, ref=-1, pos=-1, flag=int(rng.integers(0, 1 << 16)) | 4,
                         nref=-1, npos=-1))
        assert len(recs[-1].var) == v
    return Case(recs)


# ---- key_edges --------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def key_edges():
    """notes["edges"]: {label: (record index, the key spelled out)}"""
    rng = np.random.default_rng(1320)
    grid = grid_records()[0]
    mapped = 0x63          # paired, proper pair, mate unmapped, mate reverse: bit 4 clear
    twin_pieces = dict(name=_name(rng, 11), cigar=_cigar(rng, 2), seq=_blob(rng, 9), l_seq=17, qual=_blob(rng, 17),
                       aux=_blob(rng, 23))
    edge = [
        ("pos_m1", _rec(rng, 9, 1, 21, 5, ref=1, pos=-1, flag=mapped), lambda r: -1),
        ("pos_m2", _rec(rng, 9, 1, 22, 6, ref=1, pos=-2, flag=mapped), lambda r: hash_key(r.var)),
        ("pos_max", _rec(rng, 8, 2, 23, 7, ref=2, pos=0x7fffffff, flag=mapped), lambda r: hash_key(r.var)),
        ("pos_max_m1", _rec(rng, 7, 2, 24, 8, ref=2, pos=0x7ffffffe, flag=mapped), lambda r: 2 << 32 | 0x7ffffffe),
        ("flag4_placed", _rec(rng, 6, 3, 25, 9, ref=2, pos=100, flag=mapped | 4), lambda r: hash_key(r.var)),
        ("mapped_unplaced", _rec(rng, 5, 3, 26, 10, ref=-1, pos=100, flag=mapped), lambda r: hash_key(r.var)),
        ("last_ref", _rec(rng, 4, 4, 27, 11, ref=N_REF - 1, pos=77777, flag=mapped), lambda r: (N_REF - 1) << 32 | 77777),
        ("twin_a", Rec(ref=0, pos=5, mapq=3, bin_=4681, flag=4, nref=0, npos=9, tlen=100, **twin_pieces),
         lambda r: hash_key(r.var)),
        ("twin_b", Rec(ref=-1, pos=-1, mapq=60, bin_=4680, flag=0x4d, nref=-1, npos=-1, tlen=-7, **twin_pieces),
         lambda r: hash_key(r.var)),
    ]
    recs, edges = [], {}
    for k, (label, r, want) in enumerate(edge):
        recs += grid[2 * k:2 * k + 2]
        edges[label] = (len(recs), want(r))
        recs.append(r)
    recs += grid[2 * len(edge):2 * len(edge) + 2]
    return Case(recs, dict(edges=edges))


# ---- unit_boundary ----------------------------------------------------------------------------------------
UNIT_VARIANTS = [(R, lane) for R in (65535, 65537) for lane in (0, 32, 63)]


def _big_seq_rec(rng, l_seq):
    """a 16-byte name, no CIGAR, no aux: 1 + 2 (l_seq / 16) units"""
    return _rec(rng, 16, 0, l_seq, 0)


@functools.lru_cache(None)
def unit_boundary(R, lane):
    """One tile of 64: the record of R units at `lane`, 63 length_grid records around it."""
    rng = np.random.default_rng(1330 + lane + R)
    big = _big_seq_rec(rng, 16 * ((R - 1) // 2))
    assert sum(big.units()) == R
    others = list(grid_records()[0][70:133])
    return Case(others[:lane] + [big] + others[lane:], dict(big=lane))


# ---- field_major ------------------------------------------------------------------------------------------
def _bc_aux(rng, total):
    """A B:C array whose aux bytes are `total` in all (tag, type, subtype, count, payload)"""
    return b"XBBC" + struct.pack("<I", total - 8) + _blob(rng, total - 8)


def _with_aux(rng, name, n_cigar, l_seq, aux_bytes):
    r = _rec(rng, name, n_cigar, l_seq, 0)
    return Rec(r.name, r.cigar, r.seq, l_seq, r.qual, aux_bytes, ref=r.ref, pos=r.pos, mapq=r.mapq, bin_=r.bin,
               flag=r.flag, nref=r.nref, npos=r.npos, tlen=r.tlen)


FIELD_MAJOR_VARIANTS = ("one_aux", "two_over", "three_empty")


@functools.lru_cache(None)
def field_major(which):
    """one_aux:     a tile with one record whose aux is a B:C array of 1 MiB + 11 bytes (lane 17);
    two_over:    a tile with a record over the unit limit by SEQ and QUAL alone (65537 units, no
                 field of 1 MiB; lane 5) and one over it by a 1 MiB aux (lane 40);
    three_empty: every record with an empty CIGAR and l_seq 0, the last one with no name and an aux
                 of exactly 1 MiB: 65536 units, the smallest record that leaves the record-major
                 path, and three of the tile's five fields without units.
    A normal (record-major) tile of length_grid records follows each."""
    rng = np.random.default_rng(1340 + FIELD_MAJOR_VARIANTS.index(which))
    grid = grid_records()[0]
    if which == "one_aux":
        tile = list(grid[:63])
        tile.insert(17, _with_aux(rng, 9, 2, 37, _bc_aux(rng, (1 << 20) + 11)))
    elif which == "two_over":
        tile = list(grid[145:207])
        tile.insert(5, _big_seq_rec(rng, 16 * 32768))
        tile.insert(40, _with_aux(rng, 12, 0, 30, _bc_aux(rng, (1 << 20) + 16)))
    else:
        tile = [_rec(rng, int(rng.integers(0, 41)), 0, 0, int(rng.integers(0, 41))) for _ in range(63)]
        tile.append(_with_aux(rng, 0, 0, 0, _bc_aux(rng, 1 << 20)))
    assert len(tile) == 64
    return Case(tile + list(grid[130:194]))


# ---- empty_tiles ------------------------------------------------------------------------------------------
EMPTY_VARIANTS = ("no_units", "leading_empty", "bad_layout")


def bad_layout_rec(rng, k):
    """layout_ok = 0 for one of four reasons (k mod 4); every other record unmapped, so its key
    hashes the variable block the pools skip"""
    fixed = dict(flag=4, ref=-1, pos=-1) if k & 4 else {}
    why = k % 4
    if why == 0:    # n_cigar claims more than the block holds
        r = _rec(rng, 8 + k % 5, 0, 10 + k, 3, **fixed)
        return Rec(r.name, (), r.seq, len(r.qual), r.qual, r.aux, claim_n_cigar=1000 + k, ref=r.ref, pos=r.pos,
                   flag=r.flag, mapq=r.mapq, bin_=r.bin, nref=r.nref, npos=r.npos, tlen=r.tlen)
    r = _rec(rng, 6 + k % 7, k % 3, 2 * (k % 20) + 1, 0, **fixed)  # odd l_seq, no aux
    claim = {1: -1, 2: 0x7fffffff, 3: len(r.qual) + 1}[why]         # 3: the same packed bytes, one QUAL byte more
    return Rec(r.name, r.cigar, r.seq, len(r.qual), r.qual, b"", claim_l_seq=claim, ref=r.ref, pos=r.pos,
               flag=r.flag, mapq=r.mapq, bin_=r.bin, nref=r.nref, npos=r.npos, tlen=r.tlen)


@functools.lru_cache(None)
def empty_tiles(which):
    """no_units:      64 block_size-32 records (a tile without a unit), then a normal tile;
    leading_empty: a tile whose first 10 records are block_size 32, then a normal tile;
    bad_layout:    64 records with layout_ok 0 for mixed reasons, then a normal tile."""
    rng = np.random.default_rng(1350 + EMPTY_VARIANTS.index(which))
    grid = grid_records()[0]
    if which == "no_units":
        tile = [min_rec(rng) for _ in range(64)]
    elif which == "leading_empty":
        tile = [min_rec(rng) for _ in range(10)] + list(grid[100:154])
    else:
        tile = [bad_layout_rec(rng, k) for k in range(64)]
    return Case(tile + list(grid[20:84]))


# every case and variant: (id, function, arguments)
ALL = ([("length_grid", length_grid, ())] +
       [("prefixes-%d" % n, prefixes, (n,)) for n in PREFIXES] +
       [("murmur_lengths-tail%d" % t, murmur_lengths, (t,)) for t in (0, 15)] +
       [("key_edges", key_edges, ())] +
       [("unit_boundary-%d-lane%d" % v, unit_boundary, v) for v in UNIT_VARIANTS] +
       [("field_major-%s" % w, field_major, (w,)) for w in FIELD_MAJOR_VARIANTS] +
       [("empty_tiles-%s" % w, empty_tiles, (w,)) for w in EMPTY_VARIANTS])
ALL_IDS = [a[0] for a in ALL]


def get(case_id):
    _, fn, args = ALL[ALL_IDS.index(case_id)]
    return fn(*args)
