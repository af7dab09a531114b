"""The per-thread rules of the device BGZF compressor (csrc/deflate_enc.h) on the CPU.

tools/deflate_enc_host.cpp, a stand-alone program built here with the address and
undefined-behaviour sanitizers, runs the functions the kernels run, with every scratch array a heap
block of exactly the kernel's size; everything it returns is compared with tests/deflate_ref.py
(RFC 1951 tables, heap Huffman, package-merge, a header parser) and with zlib.  Nothing is loaded
into Python."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_ref as R
from conftest import ROOT

CXXFLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# sum f*len of the limited code over the package-merge optimum, worst over the vectors of
# huffman_vectors() whose limit bites, per limit, measured with the host program (see the
# docstring of test_lengths_cost_against_huffman_and_package_merge)
WORST_CLAMPED_RATIO = {15: 1.0056, 7: 1.1101}


def _build(tmp, extra=(), name="deflate_enc_host"):
    exe = os.path.join(str(tmp), name)
    subprocess.run(["g++"] + CXXFLAGS + list(extra) +
                   ["-I" + os.path.join(ROOT, "hadoop-bam_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "deflate_enc_host.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_enc")
    exe = _build(d)

    def run(payload):
        src, out = os.path.join(str(d), "in.bin"), os.path.join(str(d), "out.bin")
        with open(src, "wb") as f:
            f.write(payload)
        r = subprocess.run([exe, src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return open(out, "rb").read()
    return run


# ---- symbol codes ------------------------------------------------------------------------------
def test_len_and_dist_codes_are_the_rfc_tables(host):
    """df_len_code for every length 3..258 and df_dist_code for every distance 1..32768: symbol,
    extra-bit count and extra value are those of the RFC 1951 base / extra tables.  Exhaustive."""
    got = np.frombuffer(host(struct.pack("<I", 1)), np.uint32).reshape(-1, 3)
    assert len(got) == 256 + 32768
    want = [R.len_code(L) for L in range(3, 259)]
    assert [tuple(int(x) for x in r) for r in got[:256]] == want
    # the distance table, vectorised: code = last base <= d
    d = np.arange(1, 32769)
    code = np.searchsorted(np.array(R.DBASE), d, side="right") - 1
    assert np.array_equal(got[256:, 0], code)
    assert np.array_equal(got[256:, 1], np.array(R.DEXT)[code])
    assert np.array_equal(got[256:, 2], d - np.array(R.DBASE)[code])
    assert tuple(int(x) for x in got[256 + 32767]) == R.dist_code(32768) == (29, 13, 8191)
    assert tuple(int(x) for x in got[255]) == (285, 0, 0) and tuple(int(x) for x in got[254]) == (284, 5, 30)
    # both ends of every extra-bit range occur in the table itself
    for i in range(29):
        assert R.len_code(R.LBASE[i])[0] == 257 + i
    for i in range(30):
        assert R.dist_code(R.DBASE[i]) == (i, R.DEXT[i], 0)
        assert R.dist_code(R.DBASE[i] + (1 << R.DEXT[i]) - 1) == (i, R.DEXT[i], (1 << R.DEXT[i]) - 1)


def test_hash_and_match_are_the_restatement(host):
    """df_hash of random dwords is deflate_ref.df_hash, and df_match is the common prefix up to
    the limit, including queries that end on the buffer's last byte (a heap block of exactly the
    bytes: one byte read past it is an address-sanitizer report)."""
    rng = np.random.default_rng(5)
    w = np.concatenate([rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 1, 0xffffffff, 0x80000000], np.uint32)])
    got = np.frombuffer(host(struct.pack("<II", 4, len(w)) + w.tobytes()), np.uint32)
    assert [int(x) for x in got] == [R.df_hash(int(x)) for x in w]
    assert 0 <= int(got.max()) < 1 << R.HBITS
    buf = rng.integers(0, 2, 600, dtype=np.uint8)
    buf[300:600] = buf[0:300]
    qs = []
    for _ in range(3000):
        a, p = sorted(int(x) for x in rng.integers(0, 600, 2))
        if a == p:
            continue
        qs.append((a, p, int(rng.integers(0, min(259, 600 - p + 1)))))
    qs += [(0, 300, 258), (0, 300, 300)] + [(300 - k, 600 - k, k) for k in range(1, 20)]
    pay = struct.pack("<II", 5, len(buf)) + buf.tobytes() + struct.pack("<I", len(qs))
    pay += b"".join(struct.pack("<III", *q) for q in qs)
    got = np.frombuffer(host(pay), np.uint32)
    b = buf.tobytes()
    for (a, p, lim), g in zip(qs, got):
        k = 0
        while k < lim and b[a + k] == b[p + k]:
            k += 1
        assert int(g) == k, (a, p, lim)


# ---- Huffman lengths and codes --------------------------------------------------------------------
ALPHABETS = [(286, 15), (30, 15), (19, 7)]


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def huffman_vectors():
    """(label, n, limit, f): the committed frequency vectors of the three alphabets."""
    out = []
    for n, limit in ALPHABETS:
        rng = np.random.default_rng(1000 + n)

        def put(label, used, vals):
            f = [0] * n
            for i, v in zip(used, vals):
                f[int(i)] = int(v)
            out.append(("%s/%d" % (label, n), n, limit, f))
        put("one", [n // 2], [7])
        put("one_first", [0], [1])
        put("two", [1, n - 1], [3, 900])
        put("two_equal", [0, 1], [5, 5])
        put("all_equal", range(n), [4] * n)
        put("all_ones", range(n), [1] * n)
        # Fibonacci counts, longer than the limit allows: at least 22 used symbols for limit
        # 15, at least 12 for limit 7 (the tree of k Fibonacci counts is k - 1 deep)
        for k in ((12, 14, 19) if limit == 7 else (22, 24, 30)):
            put("fib%d" % k, range(k), _fib(k))
            put("fib%d_rev" % k, range(k), _fib(k)[::-1])
            put("fib%d_shuffled" % k, rng.permutation(n)[:k], _fib(k))
        k = min(n, 30)
        put("geometric2", rng.permutation(n)[:k], [1 << i for i in range(k)])
        put("geometric3", rng.permutation(n)[:min(n, 19)], [3 ** i for i in range(min(n, 19))])
        put("dominant", range(n), [1000000 if i == n // 3 else 1 + i % 3 for i in range(n)])
        put("fib_then_flat", range(n), (_fib(20) + [3] * n)[:n])
        for r in range(100):
            kind = r % 5
            if kind == 0:    # dense, flat
                f = rng.integers(1, 1000, n)
            elif kind == 1:  # sparse
                f = rng.integers(1, 1000, n) * (rng.random(n) < 0.08)
                f[int(rng.integers(0, n))] = 1
            elif kind == 2:  # heavy tail
                f = np.minimum((rng.pareto(0.5, n) * 3).astype(np.int64) + 1, 1 << 24)
            elif kind == 3:  # powers of two: deep trees
                f = (1 << rng.integers(0, 24, n)) * (rng.random(n) < 0.5)
                f[int(rng.integers(0, n))] = 1
            else:            # a few large, many ones
                f = np.where(rng.random(n) < 0.1, rng.integers(1000, 100000, n), 1) * (rng.random(n) < 0.7)
                f[0] = 2
            put("random%d" % r, range(n), f)
    return out


@pytest.fixture(scope="module")
def huffman_results(host):
    """Every vector through df_lengths + df_codes in one run of the host program."""
    vecs = huffman_vectors()
    pay = b"".join(struct.pack("<III", 2, n, limit) + np.array(f, np.uint32).tobytes() for _, n, limit, f in vecs)
    got, p, out = host(pay), 0, []
    for label, n, limit, f in vecs:
        lens = list(got[p:p + n])
        codes = list(struct.unpack_from("<%dH" % n, got, p + n))
        p += 3 * n
        out.append((label, n, limit, f, lens, codes))
    assert p == len(got)
    return out


def test_lengths_are_a_complete_limited_monotone_code(huffman_results):
    """Every used symbol has a length in 1..limit and every unused one 0; the Kraft sum is exactly
    1 with two or more used symbols; a more frequent symbol never has the longer code; the codes
    are the canonical assignment, bit-reversed."""
    assert len(huffman_results) >= 300
    for label, n, limit, f, lens, codes in huffman_results:
        used = [i for i in range(n) if f[i]]
        for i in range(n):
            assert (1 <= lens[i] <= limit) if f[i] else lens[i] == 0, (label, i)
        if len(used) >= 2:
            assert R.kraft(lens, limit) == 1 << limit, label
        else:
            assert [lens[i] for i in used] == [1], label
        by_f = sorted(used, key=lambda i: f[i])
        for a, b in zip(by_f, by_f[1:]):   # f[a] <= f[b]
            if f[a] < f[b]:
                assert lens[a] >= lens[b], (label, a, b)
        # a chain over the sorted order covers every pair: lengths are non-increasing in f
        want = [R.rev(c, L) for c, L in zip(R.canonical(lens), lens)]
        assert codes == want, label


def test_lengths_cost_against_huffman_and_package_merge(huffman_results):
    """sum f*len is the Huffman optimum (any optimal tree has the same cost; computed with a heap)
    whenever a limited code can reach it, i.e. whenever the package-merge optimum for the limit
    equals it.  Where the limit bites, the cost is at least the package-merge optimum and at most
    WORST_CLAMPED_RATIO[limit] + 0.01 times it: the margin is over package-merge, not over an
    earlier run of this code.

    Measured on the CPU with the host program over huffman_vectors(): the limit bites for 133 of
    the 357 vectors (69 of the 286-symbol ones, 14 of the 30, 50 of the 19).  The worst cost /
    package-merge ratios: 1.1100 at limit 7 (32221 / 29027 bits, fib19/19 and fib_then_flat/19),
    1.0056 at limit 15 with 286 symbols (random32/286), 1.0016 with 30 (fib30_shuffled/30)."""
    worst, bites = {}, 0
    deep = {n: 0 for n, _ in ALPHABETS}
    for label, n, limit, f, lens, codes in huffman_results:
        c, opt = R.cost(f, lens), R.huffman_cost(f)
        assert c >= opt, label
        if c == opt:
            continue
        pm = R.cost(f, R.package_merge(f, limit))
        assert pm > opt, "%s: cost %d above the optimum %d that limit %d allows" % (label, c, opt, limit)
        assert max(lens) == limit, label
        bites += 1
        deep[n] += 1
        assert c >= pm, label
        worst[limit] = max(worst.get(limit, (0, "")), (c / pm, label))
        assert c <= pm * (WORST_CLAMPED_RATIO[limit] + 0.01), (label, c, pm, c / pm)
    print("limit bites for %d of %d vectors; worst ratios %r" % (bites, len(huffman_results), worst))
    assert all(v > 0 for v in deep.values()), deep   # each alphabet's limit is exercised


# ---- the header writer --------------------------------------------------------------------------
def _complete(lens, free):
    """Fill free positions (the first must be 256, the end-of-block code) so that the 286 lit/len
    lengths are a complete code."""
    lens = list(lens)
    deficit = (1 << 15) - R.kraft(lens[:286], 15)
    assert deficit > 0 and free[0] == 256 and all(lens[i] == 0 for i in free)
    it = iter(free)
    for L in range(1, 16):
        while deficit >= 1 << (15 - L):
            lens[next(it)] = L
            deficit -= 1 << (15 - L)
    assert deficit == 0
    return lens


FREE = [256] + list(range(258, 286, 2))   # isolated by zeros: they start no run of their own


def _interleave(counts):
    """Values with the given counts in an order with no two neighbours equal."""
    vals = [v for v, c in sorted(counts.items(), key=lambda x: -x[1]) for _ in range(c)]
    out = [0] * len(vals)
    out[0::2] = vals[:(len(vals) + 1) // 2]
    out[1::2] = vals[(len(vals) + 1) // 2:]
    assert all(a != b for a, b in zip(out, out[1:]))
    return out


def header_cases():
    """(label, 316 lengths: 286 lit/len + 30 distance, valid for an inflater?)."""
    out = []
    one_dist = [1] + [0] * 29
    for r in range(1, 151):                      # a run of exactly r zeros between two codes
        ll = [0] * 286
        ll[0] = 2
        ll[r + 1] = 2
        out.append(("zeros%d" % r, _complete(ll, FREE) + one_dist, True))
    for r in range(1, 21):                       # a run of exactly r equal non-zero lengths
        for v in (5, 9, 15):
            ll = [0] * 286
            ll[3:3 + r] = [v] * r
            ll[0] = 1 if v > 5 else 2
            out.append(("run%d_of_%d" % (r, v), _complete(ll, FREE) + one_dist, True))
    for k in range(1, 8):                        # a run over the HLIT / HDIST boundary: HLIT 286
        ll = [0] * 286
        ll[286 - k:] = [3] * k
        free = [256] + list(range(200, 250, 2))
        for nd, dv in ((8, 3), (4, 2)):
            dl = [dv] * nd + [0] * (30 - nd)
            out.append(("cross%d_%d" % (k, nd), _complete(ll, free) + dl, True))
    ll = [0] * 286
    ll[0] = 1
    out.append(("hlit257_hdist1", _complete(ll, [256]) + one_dist, True))
    assert out[-1][1][256] == 1
    out.append(("hlit257_hdist30", _complete(ll, [256]) + [1] + [0] * 28 + [1], True))
    ll = [9] * 256 + [0] * 30
    ll[285] = 9
    out.append(("hlit286_hdist30_full", _complete(ll, [256] + list(range(283, 258, -2))) + [5] * 28 + [4] * 2, True))
    out.append(("all_fifteen_dist", _complete([0] * 286, FREE)[:286] + [1, 15] + [0] * 28, False))
    # only one code-length symbol is sent (18): no inflater takes a set without an end-of-block
    # code, but the writer must still send a complete code-length code of two codes
    out.append(("all_zero", [0] * 316, False))
    # code-length symbol counts near powers of two over a dozen symbols: the code-length code's
    # own Huffman tree is deeper than 7
    counts = {10: 128, 9: 64, 8: 32, 7: 16, 6: 8, 5: 4, 11: 2, 12: 1, 13: 1}
    seq = _interleave(counts)
    ll = [0] * 286
    ll[:len(seq)] = seq
    out.append(("cl_limit", _complete(ll, FREE) + one_dist, True))
    return out


def test_header_round_trips_and_zlib_accepts_it(host):
    """The header bits of df_rle_lengths + df_put_header for every case of header_cases(): the
    reference parser returns the same lengths; HLIT, HDIST and HCLEN are minimal; the
    code-length code is complete and within 7 bits; and with an end-of-block code appended zlib
    inflates the block (to nothing)."""
    cases = header_cases()
    got, p = host(b"".join(struct.pack("<I", 3) + bytes(lens) for _, lens, _ in cases)), 0
    seen_cl_limit = seen_one_symbol = False
    zero_runs, value_runs, crossing = set(), set(), set()
    for label, lens, valid in cases:
        hlit, hdist, hbits, tbits = struct.unpack_from("<IIII", got, p)
        raw = got[p + 16:p + 16 + (tbits + 7) // 8]
        p += 16 + (tbits + 7) // 8
        ll, dl = lens[:286], lens[286:]
        assert hlit == max(257, max(i + 1 for i in range(286) if ll[i] or i == 0)), label
        assert hdist == max(1, max(i + 1 for i in range(30) if dl[i] or i == 0)), label
        bits = R.Bits(raw)
        assert (bits.get(1), bits.get(2)) == (1, 2), label
        h = R.parse_header(bits, strict=valid)
        assert bits.pos == hbits, label
        assert (h["hlit"], h["hdist"]) == (hlit, hdist), label
        assert h["ll"] == ll[:hlit] and h["dl"] == dl[:hdist], label
        assert not any(ll[hlit:]) and not any(dl[hdist:]), label
        cl = h["cl"]
        assert h["hclen"] == 4 or cl[R.ORDER[h["hclen"] - 1]] != 0, label
        assert max(cl) <= 7 and R.kraft(cl, 7) == 1 << 7, (label, cl)
        sent = sorted(set(h["cl_syms"]))
        if len(sent) == 1:
            seen_one_symbol = True
            assert sum(1 for x in cl if x) == 2 and max(cl) == 1, (label, cl)
        clf = [h["cl_syms"].count(s) for s in range(19)]
        if R.cost(clf, cl) > R.huffman_cost(clf):
            assert max(cl) == 7 and R.cost(clf, R.package_merge(clf, 7)) > R.huffman_cost(clf), label
            seen_cl_limit = True
        sent_lens = ll[:hlit] + dl[:hdist]
        i = 0
        while i < len(sent_lens):                # the maximal runs of the sequence as sent
            j = i
            while j < len(sent_lens) and sent_lens[j] == sent_lens[i]:
                j += 1
            (value_runs if sent_lens[i] else zero_runs).add(j - i)
            if i < hlit < j and sent_lens[i]:
                crossing.add(j - i)
            i = j
        if valid:
            d = zlib.decompressobj(-15)
            assert d.decompress(raw) == b"" and d.eof and not d.unused_data, label
            blocks, data, nbits = R.parse_deflate(raw)
            assert data == b"" and nbits == tbits, label
    assert p == len(got)
    assert zero_runs >= set(range(1, 151)) and value_runs >= set(range(1, 21)), (zero_runs, value_runs)
    assert len(crossing) >= 7, crossing      # runs over the HLIT / HDIST boundary
    assert seen_cl_limit, "no case needed the code-length code's limit of 7"
    assert seen_one_symbol, "no case sent a single code-length symbol"


def test_parser_reads_a_zlib_made_dynamic_block():
    """parse_member on members whose DEFLATE stream zlib wrote (dynamic, fixed and stored
    blocks): the bytes rebuilt from its tokens are the input, which parse_member itself checks
    against zlib's inflate."""
    from helpers import bgzf_pack
    rng = np.random.default_rng(3)
    text = b"".join(b"read%d\t%d\tchr%d\t%d\n" % (i, i % 7, i % 23, i * 37) for i in range(3000))[:65280]
    for u, level, btype in ((text, 6, 2), (text, 1, 2), (bytes(65280), 9, 2), (b"abc", 6, 1),
                            (rng.integers(0, 256, 30000, dtype=np.uint8).tobytes(), 6, 0),
                            (rng.integers(0, 4, 65280, dtype=np.uint8).tobytes(), 9, 2)):
        m = R.split_members(bgzf_pack(u, level))[0]
        b = R.parse_member(m)
        assert b["btype"] == btype and b["data"] == u and b["crc_ok"] and b["isize"] == len(u)
        assert R.detokenize(b["tokens"]) == u
        if btype == 2:
            assert any(isinstance(t, tuple) for t in b["tokens"])
            assert R.kraft(b["ll"], 15) == 1 << 15


def test_restated_tokenizer_rebuilds_its_input_and_follows_its_rules():
    """deflate_ref.tokens on small inputs whose tokens can be written down by hand."""
    assert R.tokens(b"") == [] and R.tokens(b"abc") == [97, 98, 99]
    # a run: one literal, then distance 1 for the rest, the probe's 16 extended to the end
    assert R.tokens(b"a" * 20) == [97, (19, 1)]
    assert R.tokens(b"a" * 300) == [97, (258, 1), (41, 1)]
    # period 3: strict improvement keeps the first period that reaches the probe's cap
    assert R.tokens(b"abc" * 10) == [97, 98, 99, (27, 3)]
    # the last three positions have no four bytes to probe: literals
    assert R.tokens(b"abcdeabc") == [97, 98, 99, 100, 101, 97, 98, 99]
    # a length-3 match is taken at a short period only
    assert R.tokens(b"abcXabcY") == [97, 98, 99, 88, (3, 4), 89]
    # a repeat inside one 256-position chunk at a distance above 4 is not seen: heads come from
    # earlier chunks
    blk = bytes(range(100)) + bytes(range(100))
    assert R.tokens(blk) == list(blk)
    blk = bytes(range(200)) + bytes(56) + bytes(range(200))
    t = R.tokens(blk)
    assert (199, 256) in t and R.detokenize(t) == blk
    rng = np.random.default_rng(11)
    for n in (1, 5, 255, 256, 257, 1000, 5000):
        blk = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
        assert R.detokenize(R.tokens(blk)) == blk


def test_sanitizer_build_reports_a_write_past_the_rle_array(tmp_path):
    """Negative control: the same build with one indexed write one past the run-length array
    (HBAM_MODEL_SELFTEST) is reported, so the clean runs above mean something."""
    exe = _build(tmp_path, ["-DHBAM_MODEL_SELFTEST"], "deflate_enc_host_selftest")
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", 3) + bytes(header_cases()[0][1]))
    r = subprocess.run([exe, src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]


def test_crafted_blocks_exercise_their_cases():
    """The crafted blocks of deflate_enc_craft (the device tests' inputs) do, by the restatement's
    tokens, what each was built for: every match length 3..258, every distance symbol at both
    ends of its range and nothing past the window, the chunk and block edges, a distance tree
    deeper than 15, one distance code, no match at all."""
    import deflate_enc_craft as C
    C.assert_coverage()
