"""The crafted guess windows (tests/guess_cases.py; their structure is asserted on the CPU in
test_guess_model.py) on the device: every guess must equal the oracle's (out, err) exactly, through
caller-gathered windows one case at a time (host and device buffers), the whole catalogue in one
launch in two orders (cbase / k_guess_clamp with cached and uncached windows side by side), the
whole-file call, and launches of four.  k_guess_bgzf and the BCF guesser (which shares gb_read_block
and the cache) see the same kinds of input."""
import numpy as np
import pytest

import guess_cases as GC
import guess_craft as gc

pytestmark = pytest.mark.gpu


class _Items:
    """[(case, guess)] in catalogue order, built on first use (not when the module is collected)"""
    _v = None

    def _get(self):
        if _Items._v is None:
            _Items._v = GC.guesses()
        return _Items._v

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())


ITEMS = _Items()


@pytest.fixture(scope="module")
def want(oracle_mod):
    """the oracle's (out, err) of every guess, in catalogue order; computed once"""
    return [oracle_mod.guess_bam_record_start(c.np(), g["beg"], g["end"], c.n_ref) for c, g in ITEMS]


def gather(ctx, idx):
    """the windows of the guesses ITEMS[idx], concatenated -> (windows, offsets, file_len, beg, end)"""
    parts, wl = [], []
    for i in idx:
        c, g = ITEMS[i]
        n = ctx.guess_window_len(len(c.data), g["beg"], g["end"])
        wl.append(n)
        if n:
            parts.append(c.np()[g["beg"]:g["beg"] + n])
    off = np.zeros(len(idx) + 1, np.uint64)
    off[1:] = np.cumsum(wl)
    w = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    beg = np.array([ITEMS[i][1]["beg"] for i in idx], np.int64)
    end = np.array([ITEMS[i][1]["end"] for i in idx], np.int64)
    return w, off, beg, end


def run_windows(ctx, idx, device=False):
    """guess_windows over ITEMS[idx], guesses of one file"""
    import torch
    w, off, beg, end = gather(ctx, idx)
    src = torch.from_numpy(w.copy()).cuda() if (device and len(w)) else w
    rc, out, err = ctx.guess_windows(src, off, len(ITEMS[idx[0]][0].data), beg, end, GC.N_REF)
    assert rc == 0, ctx.last_error()
    return [(int(a), int(b)) for a, b in zip(out, err)]


def same_file_groups(idx):
    """idx split into runs of guesses of one file (guess_windows checks each window's length
    against one file length)"""
    groups = {}
    for i in idx:
        groups.setdefault(id(ITEMS[i][0]), []).append(i)
    return list(groups.values())


def label(i):
    c, g = ITEMS[i]
    return "%r beg=%d end=%d" % (c, g["beg"], g["end"])


@pytest.mark.parametrize("family", GC.FAMILIES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_case_per_call(gpu_ctx, want, family, device):
    idx = [i for i, (c, _) in enumerate(ITEMS) if c.family == family]
    for grp in same_file_groups(idx):
        got = run_windows(gpu_ctx, grp, device)
        for i, r in zip(grp, got):
            assert r == want[i], label(i)


def mixed_order():
    """uncached windows first, last and between cached ones"""
    D = [gc.describe(c.data, g["beg"], g["end"])["cached"] for c, g in ITEMS]
    un = [i for i, x in enumerate(D) if not x]
    ca = [i for i, x in enumerate(D) if x]
    assert len(un) >= 8 and len(ca) >= 8
    order = [un[0]]
    rest = un[1:-1]
    for k, i in enumerate(ca):
        order.append(i)
        if k % 3 == 2 and rest:
            order.append(rest.pop())
    order += rest + [un[-1]]
    assert sorted(order) == list(range(len(ITEMS)))
    return order


FAR = 1 << 40


def whole_catalogue(ctx, order):
    """One guess_windows call over the guesses ITEMS[order], which belong to different files.  The
    call takes one file length, and a window's length is min(end - beg, cap, file_len - beg); so
    each guess's (beg, end) is shifted by FAR - len(its file), which puts every file's end at FAR and
    leaves every window as its own file cut it.  The kernels see the windows, beg and end only; the
    shift is taken out of the results again (`end` comes back as given, a record start carries
    beg + cp0 above its low 16 bits)."""
    w, off, beg, end = gather(ctx, order)
    shift = np.array([FAR - len(ITEMS[i][0].data) for i in order], np.int64)
    rc, out, err = ctx.guess_windows(w, off, FAR, beg + shift, end + shift, GC.N_REF)
    assert rc == 0, ctx.last_error()
    res = []
    for k in range(len(order)):
        o, s = int(out[k]), int(shift[k])
        o = o - s if o == int(end[k]) + s else o - (s << 16)
        res.append((o, int(err[k])))
    return res


@pytest.mark.parametrize("which", ["catalogue", "mixed"])
def test_whole_catalogue_in_one_call(gpu_ctx, want, which):
    order = list(range(len(ITEMS))) if which == "catalogue" else mixed_order()
    got = whole_catalogue(gpu_ctx, order)
    for k, i in enumerate(order):
        assert got[k] == want[i], label(i)


@pytest.mark.parametrize("family", GC.FAMILIES)
def test_whole_file_batch(gpu_ctx, want, family):
    for c in [c for c in GC.cases() if c.family == family]:
        idx = [i for i, (cc, _) in enumerate(ITEMS) if cc is c]
        beg = np.array([ITEMS[i][1]["beg"] for i in idx], np.int64)
        end = np.array([ITEMS[i][1]["end"] for i in idx], np.int64)
        rc, out, err = gpu_ctx.guess_batch(c.np(), beg, end, c.n_ref)
        assert rc == 0, gpu_ctx.last_error()
        for k, i in enumerate(idx):
            assert (int(out[k]), int(err[k])) == want[i], label(i)


def test_launches_of_four(want, monkeypatch):
    """HBAM_GUESS_BATCH=4 in a fresh context: launch boundaries fall between cached and uncached
    windows of the mixed order."""
    import torch  # noqa: F401
    from hadoop_bam import _lib
    monkeypatch.setenv("HBAM_GUESS_BATCH", "4")
    ctx = _lib.Context(0)
    order = mixed_order()
    got = whole_catalogue(ctx, order)
    for k, i in enumerate(order):
        assert got[k] == want[i], label(i)


def test_bgzf_guesser(gpu_ctx, oracle_mod):
    """k_guess_bgzf has its own scan and its IOExceptions escape: families C, D and E"""
    n = 0
    for c, g in ITEMS:
        if c.family not in "CDE":
            continue
        beg, end = g["beg"], g["end"]
        wl = gpu_ctx.guess_bgzf_window_len(len(c.data), beg, end)
        got = gpu_ctx.guess_bgzf_window(c.np()[beg:beg + wl], len(c.data), beg, end)
        assert got == oracle_mod.guess_bgzf_block_start(c.np(), beg, end), (c, beg, end)
        n += 1
    assert n >= 90


@pytest.mark.parametrize("name", GC.BCF_NAMES)
def test_bcf_guesser(gpu_ctx, oracle_mod, name):
    _, data, pairs = GC.bcf_case(name)
    a = np.frombuffer(data, np.uint8)
    h = oracle_mod.bcf_header(a)
    assert isinstance(h, dict) and h["bgzf"]
    beg = np.array([p[0] for p in pairs], np.int64)
    end = np.array([p[1] for p in pairs], np.int64)
    wl = [gpu_ctx.guess_bcf_window_len(len(a), int(b), int(e), True) for b, e in pairs]
    off = np.zeros(len(pairs) + 1, np.uint64)
    off[1:] = np.cumsum(wl)
    w = np.concatenate([a[int(b):int(b) + k] for (b, _), k in zip(pairs, wl)])
    if name == "many":
        assert all(len(gc.magic_positions(a[int(b):int(b) + k])) > 256 for (b, _), k in zip(pairs[:2], wl))
    rc, out, err = gpu_ctx.guess_bcf_windows(w, off, len(a), beg, end, h)
    assert rc == 0, gpu_ctx.last_error()
    res = set()
    for i, (b, e) in enumerate(pairs):
        ref = oracle_mod.guess_bcf_record_start(a, b, e, h)
        assert (int(out[i]), int(err[i])) == ref, (name, b, e)
        res.add(ref[0] != e and ref[1] == 0)
    assert True in res  # at least one guess of each file finds a record


def test_member_over_64k_is_refused(gpu_ctx, oracle_mod):
    """The documented deviation, pinned: a member that really holds more than 65536 bytes is legal
    for htsjdk (the oracle guesses the first record of the member before it), and the device
    reader refuses it with HBAM_EUNSUPPORTED, which escapes the guess.  (An ISIZE over 65536 on a
    stream that ends short of that is a wrong field, and agrees with the oracle: E's isize_big.)"""
    data, beg, end = GC.over_64k_case()
    a = np.frombuffer(data, np.uint8)
    assert oracle_mod.guess_bam_record_start(a, beg, end, GC.N_REF) == (0, 0)
    rc, out, err = gpu_ctx.guess_batch(a, np.array([beg], np.int64), np.array([end], np.int64), GC.N_REF)
    assert rc == 0, gpu_ctx.last_error()
    assert (int(out[0]), int(err[0])) == (end, -9)
