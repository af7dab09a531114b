"""The sparse chain build's cases (tests/sparse_chain_cases.py) on its Python model: every case has
the structure it claims (where the segment boundary falls, which candidate the walker takes, which
flag sends the call to the dense path), and whenever the model accepts, its table is the true
chain.  No GPU: test_sparse_chain_gpu.py runs the same cases through the kernels."""
import pytest

import sparse_chain_cases as S


def seg1(c):
    return c.model()["segs"][1]


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_accepted_tables_are_the_true_chain(name):
    """The induction of the stitch: with no flag raised, the model's blocks and end are what a walk
    from the start gives; and every case is a valid input (segment >= SEG_MIN, start in the window)."""
    c = S.by_name()[name]
    m = c.model()
    coff, end_pos = c.truth()
    if m["sparse"]:
        assert (m["coff"], m["end_pos"]) == (coff, end_pos)
        assert all(len(sg["pos"]) <= m["cap"] for sg in m["segs"])
        # every later segment's start lies in its window
        assert all(sg["begin"] <= sg["start"] < sg["begin"] + S.WINDOW for sg in m["segs"][1:])
    else:
        assert m["flags"] != 0 and "coff" not in m


def test_well_formed_files_need_no_fallback():
    for name in ("boundary_exact", "boundary_one", "boundary_most", "full_block_at_begin", "full_block_last_pos",
                 "one_segment_shorter", "one_segment_exact", "one_segment_almost_two", "one_segment_two",
                 "window_mid_block", "inner_start", "comp_base_to_end", "comp_base_mid_block",
                 "truncated_body", "truncated_header", "truncated_member"):
        assert S.by_name()[name].model()["flags"] == 0, name


@pytest.mark.parametrize("kind", ["exact", "one", "most"])
def test_boundary(kind):
    c = S.case_boundary(kind)
    m = c.model()
    coff, _ = c.truth()
    assert m["nseg"] >= 3
    b1 = m["segs"][1]["begin"]
    k = c.k
    if kind == "exact":
        assert b1 == coff[k] == seg1(c)["start"] and seg1(c)["cands"][0] == b1
        assert m["segs"][0]["pos"][-1] == coff[k - 1]
    elif kind == "one":
        assert coff[k + 1] - b1 == 1 and seg1(c)["start"] == coff[k + 1]
        assert m["segs"][0]["pos"][-1] == coff[k]
    else:
        assert b1 - coff[k] == 1 and seg1(c)["start"] == coff[k + 1]
        assert coff[k + 1] - b1 == (coff[k + 1] - coff[k]) - 1
        assert m["segs"][0]["pos"][-1] == coff[k]


@pytest.mark.parametrize("kind", ["at_begin", "last_pos"])
def test_full_block(kind):
    c = S.case_full_block(kind)
    coff, _ = c.truth()
    sg = seg1(c)
    assert coff[c.k + 1] - coff[c.k] == 65536
    if kind == "at_begin":
        # the block is the whole window: one candidate, at its first position
        assert sg["cands"] == [sg["begin"]] == [coff[c.k]]
    else:
        assert sg["cands"] == [sg["begin"] + S.WINDOW - 1] == [coff[c.k + 1]]
    assert c.model()["sparse"]


def test_one_segment_sizes():
    n = len(S.plain_file()[0])
    m = {k: S.case_one_segment(k) for k in ("shorter", "exact", "almost_two", "two")}
    assert m["shorter"].seg > n and m["exact"].seg == n
    assert 2 * m["almost_two"].seg - n in (1, 2)
    assert n - 2 * m["two"].seg in (0, 1)
    assert [m[k].model()["nseg"] for k in ("shorter", "exact", "almost_two", "two")] == [1, 1, 1, 2]
    # the longest one-segment walk stays under the hop cap
    assert len(m["almost_two"].model()["segs"][0]["pos"]) <= m["almost_two"].model()["cap"]


def test_fake_header_hop_lands_on_garbage():
    c = S.case_fake("garbage")
    sg = seg1(c)
    assert sg["begin"] == c.fake and sg["cands"][:2] == [c.fake, c.next_true]
    assert sg["tried"] == 2 and sg["start"] == c.next_true and c.model()["sparse"]


def test_fake_header_hop_lands_on_a_second_fake():
    c = S.case_fake("second")
    sg = seg1(c)
    assert sg["cands"][:3] == [c.fake, c.fake + 100, c.next_true]
    assert sg["tried"] == 3 and sg["start"] == c.next_true and c.model()["sparse"]


def test_fake_header_rejoins_the_chain():
    """The walker accepts the fake start (its walk is flawless); only the stitch sees it."""
    c = S.case_fake("rejoin")
    sg, m = seg1(c), c.model()
    assert sg["tried"] == 1 and sg["start"] == c.fake and sg["pos"][:2] == [c.fake, c.next_true]
    assert m["segs"][0]["exit"] == c.next_true
    assert m["flags"] == S.F_STITCH


def test_more_candidates_than_slots():
    c = S.case_fake("many")
    assert len(S.candidates(c.window, c.fake, c.fake + S.WINDOW, len(c.window))) > S.CANDS
    assert c.model()["flags"] & S.F_MANY and seg1(c)["cands"] == []


def test_empties_hit_the_hop_cap():
    c = S.case_empties()
    m = c.model()
    assert m["cap"] == 32 and m["flags"] & S.F_CAP
    coff, _ = c.truth()
    assert sum(1 for p in coff if p < m["segs"][1]["begin"]) > m["cap"]


def test_window_mid_block_and_truncations_end_where_the_walk_ends():
    c = S.case_window_mid_block()
    coff_all = S.plain_file()[1]
    assert not c.file_end and c.model()["end_pos"] == coff_all[c.k] == len(c.window) - 100
    for kind, last in (("body", -1), ("header", -1), ("member", -2)):
        t = S.case_truncated(kind)
        assert t.file_end and t.model()["end_pos"] == coff_all[last]


def test_corrupt_header_and_bad_start_fall_back():
    c = S.case_corrupt()
    coff, end_pos = c.truth()
    assert end_pos == c.bad_at and c.model()["flags"] & (S.F_DERAIL | S.F_STITCH)
    assert c.bad_at > c.model()["segs"][1]["begin"] + S.WINDOW
    b = S.case_bad_start()
    assert b.truth() == ([], b.start) and b.model()["flags"] & S.F_DERAIL


def test_comp_base_windows():
    for kind in ("to_end", "mid_block"):
        c = S.case_comp_base(kind)
        assert c.comp_base > 0 and c.start == 0 and c.v_start == c.comp_base << 16
        assert c.model()["nseg"] >= 2
    assert S.case_comp_base("to_end").file_end and not S.case_comp_base("mid_block").file_end
