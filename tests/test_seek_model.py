"""The crafted seek cases (tests/seek_cases.py) on the CPU: each file has the blocks it claims, the
host restatement of the seek takes the exit the case is named for, every exit is covered in both
formats, and the oracle reads what that exit means.  The same cases run on the device in
test_seek_gpu.py."""
import zlib

import pytest

import chain_craft as cc
import seek_cases as S
from helpers import bgzf_members


def oracle_read(case, oracle):
    if case.fmt == "bam":
        return oracle.read_split(case.data, case.v_start, case.v_end, n_ref=cc.N_REF)
    return oracle.read_bcf_split_ex(case.data, case.v_start, case.v_end, case.h)


def test_broken_member_is_a_whole_block_that_zlib_rejects():
    for m in (S.E, S.parts("bam")[0]):
        b = S.broken(m)
        assert len(b) == len(m) and b[:18] == m[:18] and b[-8:] == m[-8:]
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(b[18:-8])


@pytest.mark.parametrize("fmt", S.FMTS)
def test_files_are_a_few_blocks_and_records(fmt):
    d0, d1, h, n0, n1 = S.parts(fmt)
    mem = bgzf_members(d0 + d1 + S.E)
    assert [m[1] for m in mem] == [n0, n1, 0] and all(m[2] for m in mem)
    assert 0 < h < n0
    for c in S.cases(fmt):
        assert len(c.data) < 4096 and len(c.chain()[0]) <= 4


@pytest.mark.parametrize("fmt", S.FMTS)
def test_every_exit_is_covered(fmt):
    assert sorted(set(c.exit_no for c in S.cases(fmt))) == list(range(1, 9))
    # exit 6 in its three sub-cases: end of file with and without an offset, and a readBlock error
    six = [c for c in S.cases(fmt) if c.exit_no == 6]
    assert sorted((c.chain()[1], c.v_start & 0xffff) for c in six) == [(False, 0), (False, 0), (True, 0), (True, 3)]


@pytest.mark.parametrize("fmt", S.FMTS)
def test_cases_take_their_exit(oracle_mod, fmt):
    for c in S.cases(fmt):
        assert S.seek_exit(c) == c.exit_no, c.name
        ref = oracle_read(c, oracle_mod)
        n, status = ref["n"], ref["status"]
        if c.exit_no == 8:
            assert (n, status) == (S.N_RECORDS[c.name], 0), c.name
        elif c.name in ("file_end", "empty_last"):
            assert (n, status) == (0, 0), c.name
        elif c.exit_no in (2, 7) or c.name in ("short_tail", "empty_last_offset", "empty_last_then_short"):
            assert (n, status) == (0, oracle_mod.OR_EIO), c.name  # "Invalid file pointer", "Premature end of file"
        else:
            assert n == 0 and status < 0 and status != oracle_mod.OR_EIO, (c.name, status)
