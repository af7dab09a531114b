"""The crafted merge-correction cases (tests/merge_cases.py; what they declare and reach is asserted on
the CPU in test_merge_model.py) on the device: hbam_merge_remap and hbam_rewrite_groups driven
directly over hand-made hbam_columns, against the oracle's correct_payloads and rewrite_group_tags.
Every comparison is exact.

Not covered: guard bytes behind the rewritten records.  The library owns that allocation, so a store
just past its end stays invisible here; a store that lands on a neighbouring record is seen, since
every output byte is compared.  The input payload is the test's own tensor: the 64 spare bytes the
kernels may read behind it are there, filled with a pattern, and compared after the remap."""
import ctypes as C
import struct

import numpy as np
import pytest

import f4_records as F
import merge_cases as M

pytestmark = pytest.mark.gpu

SPARE = 64
NONE = (1 << 64) - 1
STATUS = {"NullPointerException": -16, "ClassCastException": -17, "SAMFormatException": -3}  # include/hbam.h
EINVAL = -11

REMAP = M.cached(M.remap_cases)
GROUP = M.cached(M.group_cases)
PRODUCT = M.cached(M.product_cases)


def by_id(cases, cid):
    return next(c for c in cases if c.id == cid)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t, typ):
    return C.cast(C.c_void_p(t.data_ptr()), typ)


class Split:
    """hand-made hbam_columns over device tensors: the payload (with SPARE bytes of 0xA5 behind it),
    the offsets and, for the remap, the five columns it reads and writes, derived from the bytes"""

    def __init__(self, recs, keys=None):
        import torch
        from hadoop_bam import _lib
        self.pay, self.off = F.pack(recs)
        self.n = len(recs)
        self.host = np.concatenate([self.pay, np.full(SPARE, 0xA5, np.uint8)])
        self.t = {"ubuf": _dev(self.host), "rec_off": _dev(self.off.view(np.int64))}
        d = self.d = _lib.Columns()
        d.n_records, d.status, d.ubuf_len = self.n, 0, len(self.pay)
        d.ubuf, d.rec_off = _ptr(self.t["ubuf"], _lib._u8p), _ptr(self.t["rec_off"], _lib._u64p)
        if keys is not None:
            f = fields(self.pay, self.off)
            f["key"] = np.asarray(keys, np.int64)
            for k, typ in (("ref_id", _lib._i32p), ("next_ref_id", _lib._i32p), ("key", _lib._i64p),
                           ("flag", C.POINTER(C.c_uint16)), ("pos", _lib._i32p)):
                self.t[k] = _dev(f[k])
                setattr(d, k, _ptr(self.t[k], typ))
        torch.cuda.synchronize()

    def get(self, k):
        return self.t[k].cpu().numpy()


def fields(pay, off):
    b = bytes(pay)
    col = lambda fmt, at, dt: np.array([struct.unpack_from(fmt, b, int(o) + at)[0] for o in off[:-1]], dt)
    return {"ref_id": col("<i", 4, np.int32), "pos": col("<i", 8, np.int32), "flag": col("<H", 18, np.uint16),
            "next_ref_id": col("<i", 24, np.int32)}


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: length %d, expected %d" % (what, len(got), len(want))
    d = np.flatnonzero(got != want)
    assert not len(d), "%s: %d differ, the first at %d: %s, expected %s" % (what, len(d), d[0], got[d[0]:d[0] + 8], want[d[0]:d[0] + 8])


def remap(ctx, s, ref_map):
    m = np.ascontiguousarray(ref_map if ref_map is not None else [], np.int32)
    bad = C.c_uint64(0)
    rc = ctx.L.hbam_merge_remap(ctx.h, C.byref(s.d), C.c_void_p(m.ctypes.data) if len(m) else None, len(m), C.byref(bad))
    assert rc == 0, ctx.last_error()
    return -1 if bad.value == NONE else int(bad.value)


def check_remap(ctx, o, case):
    s = Split(case.recs, case.keys)
    want_pay, want_keys, want_bad = o.correct_payloads(s.pay, s.off, case.keys, case.ref_map)
    bad = remap(ctx, s, case.ref_map)
    assert bad == want_bad == case.bad, case.id
    got = s.get("ubuf")
    if bad < 0:
        n = s.n
        same(got, np.concatenate([want_pay, s.host[len(s.pay):]]), case.id + " payload and the bytes behind it")
    else:   # the oracle stops at the refused record; the device goes on writing later ones
        n = bad
        same(got[:int(s.off[n])], want_pay[:int(s.off[n])], case.id + " payload before the refused record")
        same(got[len(s.pay):], s.host[len(s.pay):], case.id + " bytes behind the payload")
    want = fields(want_pay, s.off)
    same(s.get("ref_id")[:n], want["ref_id"][:n], case.id + " ref_id")
    same(s.get("next_ref_id")[:n], want["next_ref_id"][:n], case.id + " next_ref_id")
    same(s.get("key")[:n], want_keys[:n], case.id + " key")
    same(s.get("flag"), want["flag"], case.id + " flag")
    same(s.get("pos"), want["pos"], case.id + " pos")
    same(s.get("rec_off").view(np.uint64), s.off, case.id + " rec_off")


@pytest.mark.parametrize("cid", [c.id for c in REMAP])
def test_remap(gpu_ctx, oracle_mod, cid):
    check_remap(gpu_ctx, oracle_mod, by_id(REMAP, cid))


@pytest.mark.parametrize("name", ["up", "none", "past"])
def test_remap_refused(gpu_ctx, oracle_mod, name):
    """every refused combination on its own, behind zero to two accepted records"""
    for case in M.remap_refused(name):
        check_remap(gpu_ctx, oracle_mod, case)


def rewrite(ctx, s, table):
    buf = np.frombuffer(table, np.uint8)
    st, er = C.c_int32(99), C.c_uint64(99)
    rc = ctx.L.hbam_rewrite_groups(ctx.h, C.byref(s.d), C.c_void_p(buf.ctypes.data) if len(buf) else None, len(buf),
                                   C.byref(st), C.byref(er))
    return rc, st.value, er.value


def oracle_groups(o, pay, off, groups, inp):
    """-> (payload, offsets, (exception, record) or None): the records that stand"""
    off = np.asarray(off).astype(np.int64)
    try:
        p, f = o.rewrite_group_tags(pay, off, groups, inp)
        return p, f, None
    except o.GroupRewriteError as e:
        p, f = o.rewrite_group_tags(pay, off[:e.record + 1], groups, inp)
        return p, f, (e.kind, e.record)


def check_rewritten(ctx, s, rc, st, er, want_pay, want_off, want_err, what):
    d = s.d
    assert rc == 0, ctx.last_error()
    assert (st, er) == ((STATUS[want_err[0]], want_err[1]) if want_err else (0, NONE)), what
    n = len(want_off) - 1
    assert int(d.n_records) == n, what
    assert int(d.ubuf_len) == len(want_pay), what
    addr = lambda p: C.cast(p, C.c_void_p).value
    same(ctx.download(addr(d.rec_off), 8 * (n + 1), np.uint64), want_off.astype(np.uint64), what + " rec_off")
    same(ctx.download(addr(d.block_size), 4 * n, np.int32), np.diff(want_off).astype(np.int32) - 4, what + " block_size")
    same(ctx.download(addr(d.ubuf), len(want_pay)), want_pay, what + " records")


def check_groups(ctx, o, case):
    s = Split(case.inputs())
    before = (C.cast(s.d.ubuf, C.c_void_p).value, C.cast(s.d.rec_off, C.c_void_p).value, C.cast(s.d.block_size, C.c_void_p).value)
    want_pay, want_off, want_err = oracle_groups(o, s.pay, s.off, case.groups, case.inp)
    assert want_err == case.err, case.id
    rc, st, er = rewrite(ctx, s, case.table)
    if case.noop:  # dv is left as it was
        assert (rc, st, er) == (0, 0, NONE)
        after = (C.cast(s.d.ubuf, C.c_void_p).value, C.cast(s.d.rec_off, C.c_void_p).value, C.cast(s.d.block_size, C.c_void_p).value)
        assert after == before and (int(s.d.n_records), int(s.d.ubuf_len)) == (s.n, len(s.pay))
    else:
        check_rewritten(ctx, s, rc, st, er, want_pay, want_off, want_err, case.id)
    same(s.get("ubuf"), s.host, case.id + " input payload")  # the step reads its input, never writes it


@pytest.mark.parametrize("cid", [c.id for c in GROUP])
def test_rewrite_groups(gpu_ctx, oracle_mod, cid):
    check_groups(gpu_ctx, oracle_mod, by_id(GROUP, cid))


@pytest.mark.parametrize("cid", [c.id for c in PRODUCT])
def test_both_steps_in_product_order(gpu_ctx, oracle_mod, cid):
    """sort.correct_split's order: the remap over every record, then the group step over the records
    before the refused one"""
    o, case = oracle_mod, by_id(PRODUCT, cid)
    s = Split(case.inputs(), case.keys)
    pay, keys, want_bad = o.correct_payloads(s.pay, s.off, case.keys, case.ref_map)
    bad = remap(gpu_ctx, s, case.ref_map)
    assert bad == want_bad == case.bad
    n = s.n if bad < 0 else bad
    same(s.get("key")[:n], keys[:n], "key")
    s.d.n_records = n
    want_pay, want_off, want_err = oracle_groups(o, pay, s.off[:n + 1], case.groups.groups, case.groups.inp)
    assert want_err == case.err and bytes(want_pay) == b"".join(case.out_recs)
    rc, st, er = rewrite(gpu_ctx, s, case.table)
    check_rewritten(gpu_ctx, s, rc, st, er, want_pay, want_off, want_err, case.id)


def test_table_refusals(gpu_ctx):
    """the host-side parse of the table: cut at every length, a mode of 3, a new_len under -1 —
    HBAM_EINVAL each, and dv as it was"""
    case = by_id(GROUP, "modes-11")
    s = Split(case.inputs())
    good = M.table_bytes((1, [(b"ab", b"xyz"), (b"", None)]), (1, [(b"q", b"")]))
    tables = [(good[:k], "cut at %d" % k) for k in range(len(good))]
    tables.append((M.table_bytes((3, ()), (0, ())), "PG mode 3"))
    tables.append((M.table_bytes((0, ()), (3, ())), "RG mode 3"))
    tables.append((struct.pack("<BH", 1, 1) + struct.pack("<H", 1) + b"a" + struct.pack("<h", -2) + struct.pack("<BH", 0, 0), "new_len -2"))
    before = bytes(s.d)
    for tab, what in tables:
        rc, st, er = rewrite(gpu_ctx, s, tab)
        assert rc == EINVAL, what
        assert bytes(s.d) == before, what
    rc, st, er = rewrite(gpu_ctx, s, good)  # and the whole table is accepted
    assert (rc, st, er) == (0, 0, NONE) and int(s.d.n_records) == s.n
