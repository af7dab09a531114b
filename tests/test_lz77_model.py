"""The crafted token blocks of the LZ77 resolve pass on the CPU (tests/lz77_cases.py): the reference
expansion is zlib's, the model of k_resolve_units' bookkeeping (lz77_craft.model) gives the same
bytes within the kernel's capacities, and every case reaches what it is there for, at output offset
0 mod 16 and at every lead test_lz77_gpu.py uses."""
import zlib

import pytest

import lz77_cases
import lz77_craft as lz

CASES = lz77_cases.cases()


@pytest.fixture(scope="module")
def want():
    """name -> [expand(tokens)] per block, computed once"""
    return {name: [lz.expand(t) for _, t, _ in c.blocks] for name, c in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_expansion_is_zlibs(want, name):
    for (bname, toks, literal_code), u in zip(CASES[name].blocks, want[name]):
        assert len(u) == lz.size(toks) <= 65536
        body, tail = lz.split_tail(toks)
        if tail is None:
            raw = lz.deflate_literals(u) if literal_code else lz.deflate(toks)
            assert zlib.decompress(raw, -15) == u, bname
        else:  # the stream holds the whole match; ISIZE cuts it as the output limit does here
            assert zlib.decompressobj(-15).decompress(lz.deflate(toks), len(u)) == u, bname


@pytest.mark.parametrize("name", list(CASES))
def test_model_gives_the_reference_bytes_within_capacity_and_reaches_the_path(want, name):
    case = CASES[name]
    for a0 in sorted({0} | set(case.leads)):
        reports = []
        for (bname, toks, _), u in zip(case.blocks, want[name]):
            got, stretches, seen = lz.model(toks, a0)
            assert got == u, (bname, a0)
            for k, s in enumerate(stretches):
                assert s["npre"] + s["nord"] <= lz.RU_CAP, (bname, a0, k, s)
                assert s["starts"] <= lz.RS_MAXM and s["maxrel"] <= lz.REL_MAX, (bname, a0, k, s)
            reports.append((stretches, seen))
        case.check(reports, a0)


def test_cut_rules():
    """the three cutting rules of resolve_units.h on their edges: unit sizes, distances, the head"""
    assert lz.cut(100, 16, 16) == ("plain", 0, [(100, 16, 16, False)])
    assert lz.cut(100, 40, 16) == ("plain", 0, [(100, 16, 16, False), (116, 16, 16, False), (132, 8, 16, False)])
    assert lz.cut(100, 7, 7) == ("plain", 0, [(100, 7, 7, False)])
    assert lz.cut(100, 8, 7) == ("periodic", 8, [(100, 8, 7, True)])
    assert lz.cut(100, 20, 7) == ("periodic", 16, [(100, 16, 7, True), (116, 4, 21, False)])
    assert [lz.cut(0, 17, d)[2][1][2] for d in range(1, 8)] == [16, 16, 18, 16, 20, 18, 21]
    assert lz.cut(100, 30, 8) == ("mid", 8, [(100, 8, 8, False), (108, 16, 16, False), (124, 6, 16, False)])
    assert lz.cut(100, 16, 15) == ("mid", 15, [(100, 15, 15, False), (115, 1, 30, False)])
    assert len(lz.cut(0, 258, 1)[2]) == 17 and len(lz.cut(0, 258, 300)[2]) == 17


def test_neighbours_cover_every_residue_pair():
    mem = lz77_cases.neighbours()
    pairs, inside = set(), 0
    for i, (toks, pos) in enumerate(mem):
        n = lz.size(toks)
        if i % 2:
            assert 4 <= n <= 40 and toks[1] == (n - 1, 1)
            pairs.add((pos % 16, (pos + n) % 16))
            inside += pos % 16 + n <= 16
        else:
            assert 1 <= n <= 33 and all(isinstance(t, int) for t in toks)
        assert i + 1 == len(mem) or mem[i + 1][1] == pos + n
    assert len(pairs) == 256 and inside >= 8
