"""The device BGZF compressor (csrc/hbam_deflate.hip, hbam_bgzf_compress) at the level of its
tokens and on the paths the output tests never took.

Every test inflates every member with zlib and checks CRC32 and ISIZE first (parity for readers
stays on the inflated bytes).  On top of that, the tokens parsed from each device member of a
crafted block (deflate_ref.parse_member) must be exactly those of deflate_ref.tokens, the serial
restatement of the documented algorithm; what each crafted block is there for is asserted on the
restatement's tokens (deflate_enc_craft.assert_coverage), so an input that stops exercising its
case fails instead of passing vacuously.  Inputs come from fixed seeds."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import deflate_enc_craft as craft
import deflate_ref as R
from helpers import bgzf_members

pytestmark = pytest.mark.gpu

HBAM_EINVAL = -11
BATCH = 4096   # blocks per launch (DF_BATCH in hbam_capi.hip)


def _check(comp, src, bs):
    """zlib walk of a compressed stream: member count, bytes, CRC, ISIZE, and the stored-block
    bound member size <= len + 31 (18 header + 5 stored-block + 8 trailer bytes)."""
    ms = bgzf_members(comp)
    assert len(ms) == (len(src) + bs - 1) // bs
    assert b"".join(m[0] for m in ms) == bytes(src)
    for i, (u, isz, crc_ok, size) in enumerate(ms):
        assert crc_ok and isz == len(u), i
        assert len(u) == (bs if i + 1 < len(ms) else len(src) - bs * (len(ms) - 1)), i
        assert size <= len(u) + 31 and size <= 65536, (i, size, len(u))
    return ms


def _parity(gpu_ctx, block, want, label, bs=0):
    """One block through the device: its member's tokens are the restatement's."""
    comp = gpu_ctx.bgzf_compress(block, bs).tobytes()
    _check(comp, block, bs or 65280)
    m = R.parse_member(comp)
    assert m["crc_ok"] and m["isize"] == len(block) and m["data"] == block and m["nblocks"] == 1, label
    if m["btype"] == 2:
        R.check_dynamic_header(m)
        assert m["tokens"] == want, (label, _first_difference(m["tokens"], want))
    else:   # a stored block has no tokens of its own: it must be one because it does not shrink
        assert m["btype"] == 0 and m["size"] == len(block) + 31, label
    return m


def _first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return min(len(a), len(b)), len(a), len(b)


def _stream(n=300000, seed=21):
    """A mixed stream: text-like records, a small alphabet, a stretch of random bytes, zeros."""
    rng = np.random.default_rng(seed)
    text = b"".join(b"r%07d\t%d\tchr%d\t%d\t%dM\t=\t%d\tACGTTGCA%d\n" % (i, i % 4096, i % 23, i * 37, 50 + i % 70, i * 41, i % 9)
                    for i in range(2500))
    parts = [text, rng.integers(0, 4, 90000, dtype=np.uint8).tobytes(), rng.integers(0, 256, 30000, dtype=np.uint8).tobytes(),
             bytes(40000), text[::-1]]
    return (b"".join(parts) * 2)[:n]


# ---- token parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["length", "distance", "edges"])
def test_tokens_are_the_restatements(gpu_ctx, group):
    """Length ladder (every match length 3..258), distance ladder (every distance symbol at its
    base and its last distance; a repeat at 32769 is not taken) and chunk / block edges (a
    258-byte match from chunk position 255, a match ending on a chunk end and on the block's last
    byte, block lengths 1..5, 255..259, 511..513, 65279, 65280): the device's tokens are those
    of deflate_ref.tokens, token for token."""
    craft.assert_coverage()
    dynamic = 0
    for label, block, want in craft.reference()[group]:
        m = _parity(gpu_ctx, block, want, label)
        dynamic += m["btype"] == 2
        assert all(t[1] <= 32768 for t in m["tokens"] if isinstance(t, tuple)), label
    # the parity above is on dynamic blocks; only the few-byte edge blocks may be stored
    assert dynamic >= len(craft.reference()[group]) - (5 if group == "edges" else 0)


def test_last_block_of_every_short_length(gpu_ctx):
    """A stream whose last block has 1..20 bytes: both members' tokens are the restatement's."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 3, 1024 + 20, dtype=np.uint8).tobytes()
    for k in range(1, 21):
        src = base[:1024 + k]
        comp = gpu_ctx.bgzf_compress(src, 1024).tobytes()
        ms = _check(comp, src, 1024)
        assert [len(m[0]) for m in ms] == [1024, k]
        for raw, blk in zip(R.split_members(comp), (src[:1024], src[1024:])):
            m = R.parse_member(raw)
            assert m["data"] == blk
            if m["btype"] == 2:
                R.check_dynamic_header(m)
                assert m["tokens"] == R.tokens(blk), k
            else:
                assert m["btype"] == 0 and m["size"] == len(blk) + 31


def test_huffman_extremes_through_the_kernel(gpu_ctx):
    """Blocks whose tokens drive the Huffman builder to its limits: a distance tree deeper than 15
    (Fibonacci-like counts over 17 distance codes), a code-length code deeper than 7, one distinct
    distance code, and no match at all in a block that still compresses (the empty distance set is
    sent as one unused code: HDIST 1).  Each header keeps the limits, is complete (Kraft sum
    exactly 1) and sends no trailing zero length (R.check_dynamic_header, in _parity)."""
    craft.assert_coverage()
    ms = {label: _parity(gpu_ctx, block, want, label) for label, block, want in craft.reference()["huffman"]}
    assert all(m["btype"] == 2 for m in ms.values())
    m = ms["deep_distance"]
    assert max(m["dl"]) == 15 and sum(1 for x in m["dl"] if x) >= 17
    f = craft.dist_code_counts(m["tokens"])
    assert R.cost(f, m["dl"] + [0] * (30 - len(m["dl"]))) >= R.cost(f, R.package_merge(f, 15)) > R.huffman_cost(f)
    m = ms["deep_code_length"]
    clf = [m["cl_syms"].count(s) for s in range(19)]
    assert max(m["cl"]) == 7 and R.cost(clf, R.package_merge(clf, 7)) > R.huffman_cost(clf)
    m = ms["one_distance_code"]
    assert m["hdist"] == 1 and m["dl"] == [1]
    m = ms["no_match"]
    assert m["hdist"] == 1 and m["dl"] == [1] and m["hlit"] == 257
    assert not any(isinstance(t, tuple) for t in m["tokens"])


# ---- paths the suite had never run -----------------------------------------------------------------
@pytest.mark.parametrize("bs", [1024, 1025, 4099, 65279, 65280])
def test_odd_block_sizes(gpu_ctx, bs):
    """Block sizes at both ends of the accepted range and two that are no multiple of 16 (most
    blocks then start unaligned: the dword staging loop of k_lz77_tokens and the byte loop of
    k_crc_blocks).  Every member inflates; a spread of blocks is compared token for token."""
    src = _stream()
    comp = gpu_ctx.bgzf_compress(src, bs).tobytes()
    ms = _check(comp, src, bs)
    raws = R.split_members(comp)
    step = max(1, len(ms) // 12)
    picked = sorted(set(range(0, len(ms), step)) | {len(ms) - 1})
    assert any((i * bs) % 16 for i in picked) or bs % 16 == 0
    dynamic = 0
    for i in picked:
        blk = src[i * bs:(i + 1) * bs]
        m = R.parse_member(raws[i])
        if m["btype"] == 2:
            dynamic += 1
            R.check_dynamic_header(m)
            assert m["tokens"] == R.tokens(blk), (i, _first_difference(m["tokens"], R.tokens(blk)))
        else:
            assert m["btype"] == 0 and m["size"] == len(blk) + 31
    assert dynamic >= len(picked) // 2


@pytest.mark.parametrize("bs", [0, 4099])
def test_unaligned_device_source(gpu_ctx, bs):
    """A device source 1, 5, 8 and 15 bytes past a 16-byte boundary (a view into a larger tensor,
    with room behind it, so no padded copy is made) gives the members of the aligned host copy."""
    import torch
    src = _stream(150000, seed=22)
    want = gpu_ctx.bgzf_compress(src, bs).tobytes()
    _check(want, src, bs or 65280)
    big = torch.zeros(len(src) + 16 + 256, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    for off in (1, 5, 8, 15):
        view = big[off:off + len(src)]
        view.copy_(torch.from_numpy(np.frombuffer(src, np.uint8).copy()))
        assert view.data_ptr() % 16 == off
        p, n, dev, keep = gpu_ctx._ptr(view)
        assert dev == 1 and keep.data_ptr() == view.data_ptr(), "a padded copy was made"
        assert gpu_ctx.bgzf_compress(view, bs).tobytes() == want, off


def test_argument_checks(gpu_ctx):
    """block_size 1023 and 65281 are HBAM_EINVAL; n = 0 returns 0 and writes nothing;
    hbam_bgzf_bound is ceil(n / bs) * 65536."""
    L = gpu_ctx.L
    src = np.zeros(5000, np.uint8)
    dst = np.full(1 << 17, 0xA5, np.uint8)
    call = lambda n, bs: L.hbam_bgzf_compress(gpu_ctx.h, C.c_void_p(src.ctypes.data), 0, n, bs,
                                              C.c_void_p(dst.ctypes.data), 0, dst.size)
    assert call(5000, 1023) == HBAM_EINVAL and call(5000, 65281) == HBAM_EINVAL
    assert np.all(dst == 0xA5)
    assert call(0, 0) == 0 and call(0, 4096) == 0 and np.all(dst == 0xA5)
    assert call(5000, 1024) > 0 and call(5000, 65280) > 0
    for n in (0, 1, 1023, 1024, 1025, 65280, 65281, 10 ** 7 + 3):
        for bs in (0, 1024, 1025, 4099, 65280):
            b = bs or 65280
            assert int(L.hbam_bgzf_bound(n, bs)) == -(-n // b) * 65536, (n, bs)


def _batch_source():
    n = BATCH * 1024 + 3 * 1024 + 7
    rng = np.random.default_rng(41)
    return rng.integers(0, 5, n, dtype=np.uint8).tobytes()   # differs block by block


def test_past_one_batch(gpu_ctx):
    """block_size 1024 and 4096 * 1024 + 3 * 1024 + 7 bytes: the batch loop's second iteration
    (its source offset, the running output offset, the reused scratch), to a host and to a device
    destination.  4100 members that inflate to the input, and, blocks being independent, exactly
    compress(first 4096 blocks) + compress(the rest)."""
    import torch
    src = _batch_source()
    cut = BATCH * 1024
    host = gpu_ctx.bgzf_compress(src, 1024).tobytes()
    ms = _check(host, src, 1024)
    assert len(ms) == BATCH + 4 and len(ms[-1][0]) == 7
    out = torch.full((len(src) + 31 * len(ms) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    n = gpu_ctx.bgzf_compress(src, 1024, out=out)
    dev = out.cpu().numpy()
    assert dev[:n].tobytes() == host and np.all(dev[n:] == 0xA5)
    a = gpu_ctx.bgzf_compress(src[:cut], 1024).tobytes()
    b = gpu_ctx.bgzf_compress(src[cut:], 1024).tobytes()
    assert len(bgzf_members(b)) == 4
    assert host == a + b


def test_blocks_are_independent_and_the_output_is_deterministic(gpu_ctx):
    import torch
    src = _stream()
    for bs in (4099, 65280):
        whole = gpu_ctx.bgzf_compress(src, bs).tobytes()
        cut = 3 * bs
        assert whole == gpu_ctx.bgzf_compress(src[:cut], bs).tobytes() + gpu_ctx.bgzf_compress(src[cut:], bs).tobytes()
        assert whole == gpu_ctx.bgzf_compress(src, bs).tobytes()
        out = torch.empty(int(gpu_ctx.L.hbam_bgzf_bound(len(src), bs)), dtype=torch.uint8, device="cuda")
        n = gpu_ctx.bgzf_compress(src, bs, out=out)
        assert out[:n].cpu().numpy().tobytes() == whole
        d = torch.from_numpy(np.frombuffer(src, np.uint8).copy()).cuda()
        n = gpu_ctx.bgzf_compress(d, bs, out=out)
        assert out[:n].cpu().numpy().tobytes() == whole


def test_stored_and_dynamic_blocks(gpu_ctx):
    """Uniform random blocks are stored (BTYPE 0) with a member of exactly len + 31 bytes; the
    compressible inputs are dynamic (BTYPE 2)."""
    rng = np.random.default_rng(51)
    src = rng.integers(0, 256, 2 * 65280 + 1234, dtype=np.uint8).tobytes()
    for bs in (65280, 1025):
        comp = gpu_ctx.bgzf_compress(src, bs).tobytes()
        ms = _check(comp, src, bs)
        for raw, (u, _, _, size) in zip(R.split_members(comp), ms):
            assert raw[18] & 7 == 1 and size == len(u) + 31     # BFINAL 1, BTYPE 0
    for src in (_stream()[:140000], bytes(70000), b"ACGT" * 20000):
        comp = gpu_ctx.bgzf_compress(src, 0).tobytes()
        _check(comp, src, 65280)
        assert all(raw[18] & 7 == 5 for raw in R.split_members(comp))   # BFINAL 1, BTYPE 2


def _short_cap(gpu_ctx, src, bs, want):
    """A device destination one byte short of the result, 256 guard bytes behind the cap."""
    import torch
    cap = len(want) - 1
    out = torch.full((cap + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    p, n, dev, keep = gpu_ctx._ptr(src)
    r = gpu_ctx.L.hbam_bgzf_compress(gpu_ctx.h, p, dev, n, bs, C.c_void_p(out.data_ptr()), 1, cap)
    torch.cuda.synchronize()
    assert r == HBAM_EINVAL, r
    assert "dst_cap" in gpu_ctx.last_error()
    got = out.cpu().numpy()
    assert np.all(got[cap:] == 0xA5), "bytes behind dst_cap were written"
    return got[:cap]


def test_destination_too_small(gpu_ctx):
    """dst_cap one byte short: HBAM_EINVAL and nothing written behind the cap; the same when the
    cap is short only in the second batch (the first batch's members are already in place)."""
    src = _stream(100000, seed=23)
    want = gpu_ctx.bgzf_compress(src, 4099).tobytes()
    got = _short_cap(gpu_ctx, src, 4099, want)
    assert np.all(got == 0xA5)      # one batch: the check comes before anything is packed
    src = _batch_source()
    want = gpu_ctx.bgzf_compress(src, 1024).tobytes()
    first = gpu_ctx.bgzf_compress(src[:BATCH * 1024], 1024).tobytes()
    assert len(first) < len(want) - 1
    got = _short_cap(gpu_ctx, src, 1024, want)
    assert got[:len(first)].tobytes() == first and np.all(got[len(first):] == 0xA5)
    # the context is still good
    again = gpu_ctx.bgzf_compress(src[:5 * 1024], 1024).tobytes()
    assert again == want[:len(again)] and len(bgzf_members(again)) == 5


def test_bgzf_sink_flushes_whole_blocks(gpu_ctx, monkeypatch):
    """_BGZFSink with block size 4099: writes of 1, 4098, 4099, 4100 and _FLUSH_BYTES + 1 bytes,
    flush(), write_device of a device tensor, and the closing flush.  The members inflate to the
    concatenation, and every member but those a flush (or the end of a device run) ends has ISIZE
    4099.  _FLUSH_BYTES is set to a few blocks for the test: the rule under test is that crossing
    it compresses whole blocks only, whatever its value."""
    import torch
    from hadoop_bam import output
    bs = 4099
    monkeypatch.setattr(output, "_FLUSH_BYTES", 9 * bs + 123)
    rng = np.random.default_rng(61)
    sizes = [1, 4098, 4099, 4100, output._FLUSH_BYTES + 1]
    chunks = [rng.integers(0, 6, k, dtype=np.uint8).tobytes() for k in sizes]
    devbytes = rng.integers(0, 6, 3 * bs + 77, dtype=np.uint8)
    f = io.BytesIO()
    sink = output._BGZFSink(f, gpu_ctx, bs)
    for c in chunks[:4]:
        sink.write(c)
    assert f.getvalue() == b""                       # below _FLUSH_BYTES: nothing leaves yet
    sink.write(chunks[4])
    total = sum(sizes)
    first = bgzf_members(f.getvalue())
    assert len(first) == total // bs and all(m[1] == bs for m in first)
    assert len(sink.buf) == total % bs > 0
    sink.flush()
    sink.write_device(torch.from_numpy(devbytes).cuda())
    sink.flush()
    ms = bgzf_members(f.getvalue())
    assert all(m[2] and m[1] == len(m[0]) for m in ms)
    assert b"".join(m[0] for m in ms) == b"".join(chunks) + devbytes.tobytes()
    assert [m[1] for m in ms] == [bs] * (total // bs) + [total % bs] + [bs] * 3 + [77]


# ---- quality ------------------------------------------------------------------------------------
# device bytes / zlib level 1 bytes over the same 65280-byte blocks, measured on an MI355X
ZLIB1_RATIO = {"bam_stream": 0.9958, "zeros": 0.3451, "text": 0.8574}


def _quality_inputs():
    from test_output import _inputs
    ins = _inputs()
    text = b"".join(b"@SQ\tSN:contig%05d\tLN:%d\tM5:%032x\tUR:file:/ref/genome.fa\n" % (i, 1000 + i * 7919 % 100000, i * 2654435761)
                    for i in range(3000))
    return {"bam_stream": ins["bam_stream"], "zeros": ins["zeros"], "text": text}


@pytest.mark.parametrize("name", ["bam_stream", "zeros", "text"])
def test_size_against_zlib_level_1(gpu_ctx, name):
    """Total compressed size against zlib level 1 on the same 65280-byte blocks (zlib's raw stream
    plus the 26 bytes of the same framing per member).  Measured device / zlib ratios on an
    MI355X: bam_stream 0.9958 (3085080 / 3097987 bytes), zeros 0.3451 (361 / 1046), text 0.8574
    (42951 / 50092).  Asserted: the measured ratio plus 5 % of itself.  The reference is zlib;
    the margin is there so that a tuning change that trades ratio for speed has to change these
    numbers visibly.  (With the hash probe disabled the ratios are 1.2688, 0.3451 and 2.5927.)"""
    src = _quality_inputs()[name]
    comp = gpu_ctx.bgzf_compress(src, 0).tobytes()
    _check(comp, src, 65280)
    z = 0
    for i in range(0, len(src), 65280):
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        z += len(co.compress(src[i:i + 65280]) + co.flush()) + 26
    ratio = len(comp) / z
    print("device %d zlib-1 %d ratio %.4f" % (len(comp), z, ratio))
    assert ratio <= ZLIB1_RATIO[name] * 1.05, (name, len(comp), z, ratio)
