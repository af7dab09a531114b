"""The tests' restatement of the reference's FASTQ and QSEQ writers (host Python, no device).

fastq_write is FastqRecordWriter.write with makeId (FastqOutputFormat.java:94-147) and the Sanger ->
Illumina branch of SequencedFragment.convertQuality (SequencedFragment.java:234-247); qseq_write is
QseqRecordWriter.write (QseqOutputFormat.java:100-159).  Both append to a bytearray the way the Java
writes to its stream, statement by statement, so what the stream holds when an exception leaves
write() is what the bytearray holds.  Fragments are seqfrag_ref's dicts (new_fragment): strings as
bytes (str is accepted and encoded), None for a null field.  render() runs one of them over a list
of records and returns what hbam_frag_render reports.

Where the device documents an input as not restated (a byte >= 0x80 in a QSEQ sequence or quality:
the reference decodes the Text to a String and encodes the result) qseq_write raises Unsupported.
"""
OK, EUNSUPPORTED, ERUNTIME, ESEQFORMAT = 0, -9, -15, -18


class RuntimeException(Exception):
    code = ERUNTIME


class FormatException(RuntimeException):
    code = ESEQFORMAT


class Unsupported(Exception):
    code = EUNSUPPORTED


CONF_KEY = {"fastq": "hbam.fastq-output.base-quality-encoding", "qseq": "hbam.qseq-output.base-quality-encoding"}
CONF_DEFAULT = {"fastq": "sanger", "qseq": "illumina"}


def set_conf(conf, fmt):
    """setConf of either writer -> True for Illumina output."""
    setting = conf.get(CONF_KEY[fmt], CONF_DEFAULT[fmt])
    if setting == "illumina":
        return True
    if setting == "sanger":
        return False
    raise RuntimeException("Invalid property value '%s' for %s.  Valid values are 'illumina' or 'sanger'"
                           % (setting, CONF_KEY[fmt]))


def _b(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def _str(v):
    """x == null ? "" : x (a String) or x.toString() (an Integer)."""
    if v is None:
        return b""
    if isinstance(v, bool):
        raise TypeError(v)
    return b"%d" % v if isinstance(v, int) else _b(v)


def make_id(f):
    sb = bytearray()
    sb += _str(f["instrument"]) + b":"
    sb += _str(f["run"]) + b":"
    sb += _str(f["flowcell"]) + b":"
    sb += _str(f["lane"]) + b":"
    sb += _str(f["tile"]) + b":"
    sb += _str(f["xpos"]) + b":"
    sb += _str(f["ypos"])
    sb += b" "
    sb += _str(f["read"]) + b":"
    sb += b"N" if f["filter_passed"] is None or f["filter_passed"] else b"Y"
    sb += b":"
    sb += (b"0" if f["control"] is None else _str(f["control"])) + b":"
    sb += _str(f["index"])
    return bytes(sb)


def _signed(b):
    return b - 256 if b >= 128 else b


def fastq_write(out, key, f, illumina):
    out += b"@"
    out += _b(key) if key is not None else make_id(f)
    out += b"\n"
    out += _b(f["seq"])
    out += b"\n+\n"
    if not illumina:
        out += _b(f["qual"])
    else:
        buf = bytearray(_b(f["qual"]))
        for i in range(len(buf)):  # convertQuality, Sanger -> Illumina
            if _signed(buf[i]) < 33 or _signed(buf[i]) > 33 + 93:
                raise FormatException("base quality score out of range for Sanger format (found %d)"
                                      % (_signed(buf[i]) - 33))
            buf[i] = (buf[i] + 31) & 0xff
        out += buf
    out += b"\n"


def qseq_write(out, key, f, illumina):
    seq, qual = _b(f["seq"]), _b(f["qual"])
    if any(b >= 0x80 for b in seq) or any(b >= 0x80 for b in qual):
        raise Unsupported("a byte >= 0x80 in the sequence or the quality")
    sb = bytearray()
    for k in ("instrument", "run", "lane", "tile", "xpos", "ypos"):
        sb += _str(f[k]) + b"\t"
    index = b"0" if f["index"] is None or len(_b(f["index"])) == 0 else _b(f["index"]).replace(b"N", b".")
    sb += index + b"\t"
    sb += _str(f["read"]) + b"\t"
    sb += seq.replace(b"N", b".") + b"\t"
    start = len(sb)
    sb += qual
    if illumina:
        for i in range(start, len(sb)):
            v = sb[i] + 31
            if v > 126:
                raise RuntimeException("output quality score over allowed range.  Maybe you meant to write in "
                                       "Sanger format?")
            sb[i] = v
    sb += b"\t"
    sb += b"1" if f["filter_passed"] is None or f["filter_passed"] else b"0"
    out += sb
    out += b"\n"


def render(records, fmt, illumina, use_key=False):
    """The writer over `records` in order -> what hbam_frag_render reports: text (the complete
    records), line_off, n, status, err_record and partial (the bytes of the failing record the stream
    already holds)."""
    write = fastq_write if fmt == "fastq" else qseq_write
    out = bytearray()
    off = [0]
    res = {"status": OK, "err_record": 0, "partial": b""}
    for k, f in enumerate(records):
        try:
            write(out, f["key"] if (use_key and fmt == "fastq") else None, f, illumina)
        except (RuntimeException, Unsupported) as e:
            res.update(status=e.code, err_record=k, partial=bytes(out[off[-1]:]))
            del out[off[-1]:]
            break
        off.append(len(out))
    res.update(text=bytes(out), line_off=off, n=len(off) - 1)
    return res
