"""The LZ77 resolve pass (k_resolve_units, csrc/resolve_units.h) on the device against the
sequential expansion, on the crafted token blocks of tests/lz77_cases.py (test_lz77_model.py shows
on the CPU which path each case reaches and that the expansion is zlib's).

Direct: every block through Context.resolve_tokens (output offset 0 mod 16).  Through the inflater:
the same blocks as BGZF members behind a lead member, so that their output starts at every offset
mod 16 the case asks for, once with the Huffman wave pass and once with the lane pass (both write
the token form the resolve pass reads), CRC checked.  Neighbours: small members packed back to back,
every second one all literals that no pass rewrites, so a byte written outside a block shows.
Every comparison is byte-exact."""
import functools

import numpy as np
import pytest

import lz77_cases
import lz77_craft as lz

pytestmark = pytest.mark.gpu

CASES = lz77_cases.cases()
MODES = {"wave": "1000000000", "lane": "0"}


@functools.lru_cache(None)
def _members(name):
    return [lz.member(toks, literal_code) for _, toks, literal_code in CASES[name].blocks]


@pytest.fixture(scope="module")
def passes():
    """mode -> a fresh Context that runs the Huffman wave pass / the lane pass on every call"""
    import torch  # noqa: F401  (its HIP runtime opens the device before libhbam's)
    from hadoop_bam import _lib
    mp, ctx = pytest.MonkeyPatch(), {}
    try:
        for mode, limit in MODES.items():
            mp.setenv("HBAM_WAVE_MAX_BLOCKS", limit)
            ctx[mode] = _lib.Context(0)
        yield ctx
    finally:
        mp.undo()
        for c in ctx.values():
            c.close()


def _inflate_and_compare(ctx, members, what):
    data, tab = lz.table(members)
    rc, u, off, st = ctx.inflate(data, tab, check_crc=True)
    assert rc == 0, what
    assert np.all(st == 0), (what, np.nonzero(st)[0][:8], st[st != 0][:8])
    for j, (_, want) in enumerate(members):
        got = u[int(off[j]):int(off[j + 1])].tobytes()
        if got != want:
            bad = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError((what, "member", j, "of", len(members), "isize", len(want), "first bad byte", bad))


@pytest.mark.parametrize("name", list(CASES))
def test_resolve_tokens_equals_the_sequential_expansion(gpu_ctx, name):
    for bname, toks, _ in CASES[name].blocks:
        io, bm, tt, td = lz.token_block(toks)
        rc, st, out = gpu_ctx.resolve_tokens(io, bm, tt, td)
        assert rc == 0 and st == 0, (bname, rc, st)
        want = lz.expand(toks)
        if out != want:
            bad = next(i for i in range(len(want)) if out[i] != want[i])
            raise AssertionError((bname, "first bad byte", bad, "of", len(want)))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.direct_only])
def test_members_at_every_lead_inflate_to_zlibs_bytes(passes, name, mode):
    for lead in CASES[name].leads:
        _inflate_and_compare(passes[mode], lz.stream(_members(name), lead), (name, mode, "lead", lead))


@pytest.mark.parametrize("mode", list(MODES))
def test_member_cut_inside_its_last_match_resolves_the_tail(passes, mode):
    """A member whose ISIZE ends 1 or 2 bytes into its last match: the Huffman pass leaves its
    symbol loop with exit code 2, finds op == isize and reports INF_OK with the tail token set
    (inflate_tok.h, `leave:`), as zlib fills the output and stops; with the CRC of those bytes the
    member is good, so the resolve pass does run its tail path in production.  The tails case's
    blocks, the cut match written whole in the stream."""
    for lead in (0,) + CASES["tails"].leads:
        _inflate_and_compare(passes[mode], lz.stream(_members("tails"), lead), ("tails", mode, "lead", lead))


@pytest.mark.parametrize("lead", [0, 7])
def test_neighbours_are_left_alone(gpu_ctx, lead):
    """Every byte of the packed output is zlib's: a write outside [base, aend) of a match member
    lands in a literal neighbour that nobody rewrites (test_lz77_model.py: every (start, end)
    residue pair mod 16 is there, some members inside one 16-byte column)."""
    members = [lz.member(toks) for toks, _ in lz77_cases.neighbours()]
    head = [lz.member(list(range(65, 65 + lead)))] if lead else []  # every residue pair moves by lead
    _inflate_and_compare(gpu_ctx, head + members, ("neighbours", lead))
