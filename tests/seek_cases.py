"""Crafted splits for every way BlockCompressedInputStream.seek(vStart) can go at the start of a BGZF
split (bgzf_seek in csrc/hbam_capi.hip), shared by test_seek_model.py (CPU: each case has the
structure it claims) and test_seek_gpu.py (device against the oracle).  A file is a few BGZF members:
D0 (the header and four records), D1 (four more), E (an empty member, the EOF block), and the same
with a broken DEFLATE stream; a case is such a file and the virtual offset the split starts at.

The exits, numbered as in seek_exit below:
  1  no block at vStart, the file ends there, offset 0: an empty split
  2  the same with a non-zero offset: "Invalid file pointer"
  3  no block at vStart and no end of file: what readBlock throws there
  4  the block at vStart is empty and does not inflate
  5  the block the seek lands in (the one after an empty block) does not inflate
  6  the block at vStart is empty and the last of the chain: as 1, 2 or 3 for what follows it
  7  the offset lies past the block, or at its end with more blocks to come
  8  the seek succeeds"""
import functools
import struct

import chain_craft as cc

E = cc.BGZF_EOF
FMTS = ["bam", "bcf"]


def broken(member):
    """The member with BFINAL = 1, BTYPE = 3 (reserved) at the start of its DEFLATE stream."""
    return member[:18] + b"\x07" + member[19:]


class SeekCase:
    def __init__(self, name, fmt, exit_no, members, v_start, header_len, bad=None, tail=b""):
        self.name, self.fmt, self.exit_no, self.bad = name, fmt, exit_no, bad
        self.data = b"".join(members) + tail
        self.v_start = v_start(self) if callable(v_start) else v_start
        self.v_end = len(self.data) << 16 | 0xffff
        self.h = dict(cc.BCF_H, header_len=header_len, bgzf=True)

    def chain(self):
        """(isize, clen) of the blocks a reader finds from vStart's file offset on, and whether the
        chain ends at the end of the file."""
        d, p, out = self.data, self.v_start >> 16, []
        while p + 18 <= len(d) and d[p:p + 4] == b"\x1f\x8b\x08\x04" and d[p + 12:p + 16] == b"BC\x02\x00":
            bs = struct.unpack_from("<H", d, p + 16)[0] + 1
            if bs < 26 or p + bs > len(d):
                break
            out.append((struct.unpack_from("<I", d, p + bs - 4)[0], bs))
            p += bs
        return out, p == len(d)


def seek_exit(case):
    """The exit of bgzf_seek the case takes, from the file's bytes (case.bad: the index in the
    chain of the block that does not inflate)."""
    blocks, at_eof = case.chain()
    off = case.v_start & 0xffff
    if not blocks:
        return 3 if not at_eof else 2 if off else 1
    sblk = 1 if blocks[0][0] == 0 else 0
    if case.bad == 0 and sblk == 1:
        return 4
    if case.bad is not None and case.bad == sblk:
        return 5
    if sblk >= len(blocks):
        return 6
    p = (case.v_start >> 16) + sum(b[1] for b in blocks[:sblk + 1])  # the file position after the seek block
    eof = p == len(case.data) or len(case.data) - p == 28
    if off > blocks[sblk][0] or (off == blocks[sblk][0] and not eof):
        return 7
    return 8


@functools.lru_cache(None)
def parts(fmt):
    """(D0, D1, header length, D0's inflated size, D1's inflated size)"""
    s = cc.BamStream() if fmt == "bam" else cc.BcfStream()
    s.add_trues(8)
    u, c = s.bytes(), s.starts[4]
    return cc.bgzf_member(u[:c]), cc.bgzf_member(u[c:]), s.header_len, c, len(u) - c


JUNK = b"\x00" + b"garbage-bytes" * 3  # 40 bytes that are no BGZF header
N_RECORDS = {"first_block": 8, "after_empty": 8, "block_end_eof": 0}  # the exit-8 cases' record counts


@functools.lru_cache(None)
def cases(fmt):
    d0, d1, h, n0, n1 = parts(fmt)
    plain = [d0, d1, E]
    at_e = (len(d0) + len(d1)) << 16  # vStart at the EOF block
    end = len(b"".join(plain)) << 16

    def mk(name, exit_no, members, v_start, **kw):
        return SeekCase(name, fmt, exit_no, members, v_start, h, **kw)

    return [
        mk("file_end", 1, plain, end),
        mk("file_end_offset", 2, plain, end | 5),
        mk("inside_a_block", 3, plain, (len(d0) + 3) << 16),
        mk("short_tail", 3, plain, end - (10 << 16)),  # ten bytes left: "Premature end of file"
        mk("broken_empty_first", 4, [broken(E), d0, d1, E], h, bad=0),
        mk("broken_after_empty", 5, [E, broken(d0), d1, E], h, bad=1),
        mk("broken_first", 5, [broken(d0), d1, E], h, bad=0),
        mk("empty_last", 6, plain, at_e),
        mk("empty_last_offset", 6, plain, at_e | 3),
        mk("empty_last_then_junk", 6, plain, at_e, tail=JUNK),
        mk("empty_last_then_short", 6, plain, at_e, tail=JUNK[:10]),
        mk("past_block", 7, plain, n0 + 1),
        mk("block_end", 7, plain, n0),
        mk("block_end_eof", 8, plain, len(d0) << 16 | n1),
        mk("after_empty", 8, [E] + plain, h),
        mk("first_block", 8, plain, h),
    ]


def ids(fmt):
    return [c.name for c in cases(fmt)]
