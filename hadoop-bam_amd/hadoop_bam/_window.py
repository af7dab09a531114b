"""The window policy of the line-oriented split readers (text VCF, SAM text, FASTQ, QSEQ)."""
from . import _lib


def read_growing_window(ss, base, start, length, tail0, call):
    """The device call over the window of FileSplit [start, start + length) of SeekableFile `ss`:
    file bytes [base, start + length + tail), the tail growing x4 from tail0 while the call answers
    HBAM_EMORE and the file goes on (length None: the whole rest of the file at once).
    call(window, base) -> the host columns dict or the device struct, whichever carries `status`;
    it raises for its own return code.  -> (that result, window)."""
    tail = tail0
    while True:
        stop = ss.length if length is None else max(base, min(ss.length, start + length + tail))
        window = ss.read_at(base, stop - base)
        res = call(window, base)
        status = res["status"] if isinstance(res, dict) else int(res.status)
        if status != _lib.HBAM_EMORE or stop == ss.length:
            return res, window
        tail *= 4
