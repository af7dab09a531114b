"""Plain-Python restatement of the SAM text WRITE path, for the tests only (the product never imports
it and it does not import the product's renderer), written from the rules of include/hbam.h and not
from the device code: a record's status, its line as htsjdk's SAMTextWriter.writeAlignment writes
it with floats in Java's Float.toString layout (JDK 19+), and the predicate that says which records
the device hands to the host.  It reuses sam_ref.fields and sam_ref.decode_aux.  htsjdk is not in
the reference tree: the rules are restated from memory (DESIGN.md lists them), so parity is between
two restatements."""
import struct

import numpy as np

import sam_ref

HBAM_OK, HBAM_EFORMAT, HBAM_EREFID = 0, -3, -6
_WIDTH = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def bits_of(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def java_float(bits):
    """Float.toString of the float32 with these bits (JDK 19+): the shortest digits that read back
    as the same float32, at least two of them (one: the value rounded to two); plain decimal for
    1e-3 <= |v| < 1e7, else d.dddE[-]x; at least one digit after the point."""
    v = np.frombuffer(struct.pack("<I", bits & 0xffffffff), np.float32)[0]
    if np.isnan(v):
        return "NaN"
    sign = "-" if bits >> 31 else ""
    if np.isinf(v):
        return sign + "Infinity"
    if bits & 0x7fffffff == 0:
        return sign + "0.0"
    mant, exp = np.format_float_scientific(np.abs(v), unique=True, trim="-").split("e")
    digits, e = mant.replace(".", ""), int(exp)
    if len(digits) == 1:  # float -> double is exact, and '%e' of a double rounds its exact value
        mant, exp = ("%.1e" % float(np.abs(v))).split("e")
        digits, e = mant.replace(".", ""), int(exp)
    digits = digits.rstrip("0") or "0"
    if -3 <= e < 7:
        if e >= 0:
            whole, frac = digits[:e + 1].ljust(e + 1, "0"), digits[e + 1:]
        else:
            whole, frac = "0", "0" * (-e - 1) + digits
        return sign + whole + "." + (frac or "0")
    return sign + digits[0] + "." + (digits[1:] or "0") + "E%d" % e


def float_on_device(bits):
    """The device's float domain: 0.0, -0.0 and the integer values below 10^7 in magnitude."""
    v = float(np.frombuffer(struct.pack("<I", bits), np.float32)[0])
    return v == v and abs(v) < 1e7 and v == int(v)


def _walk_tags(rec, p):
    """-> [(type, subtype, values offset, count)] of the aux bytes rec[p:], or None when malformed."""
    end, out = len(rec), []
    while p < end:
        if end - p < 3:
            return None
        t = chr(rec[p + 2])
        p += 3
        if t in _WIDTH:
            if end - p < _WIDTH[t]:
                return None
            out.append((t, None, p, 1))
            p += _WIDTH[t]
        elif t in "ZH":
            z = rec.find(b"\0", p)
            if z < 0:
                return None
            out.append((t, None, p, z - p))
            p = z + 1
        elif t == "B":
            if end - p < 5:
                return None
            sub, cnt = chr(rec[p]), struct.unpack_from("<i", rec, p + 1)[0]
            if sub not in "cCsSiIf" or cnt < 0 or _WIDTH[sub] * cnt > end - p - 5:
                return None
            out.append((t, sub, p + 5, cnt))
            p += 5 + _WIDTH[sub] * cnt
        else:
            return None
    return out


def status(slot, n_ref):
    """The status of the record in its rec_off slot (bytes): the checks in the header's order."""
    if len(slot) < 36:
        return HBAM_EFORMAT
    bs = struct.unpack_from("<i", slot, 0)[0]
    if bs < 32 or 4 + bs > len(slot):
        return HBAM_EFORMAT
    rec = bytes(slot[:4 + bs])
    ref, _, lrn, _, _, ncig, _, lseq, nref = struct.unpack_from("<iiBBHHHii", rec, 4)
    if lrn == 0 or lseq < 0:
        return HBAM_EFORMAT
    if bs < 32 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq:
        return HBAM_EFORMAT
    if not (-1 <= ref < n_ref and -1 <= nref < n_ref):
        return HBAM_EREFID
    if any(w & 15 > 8 for w in struct.unpack_from("<%dI" % ncig, rec, 36 + lrn)):
        return HBAM_EREFID
    q = 36 + lrn + 4 * ncig + (lseq + 1) // 2
    if _walk_tags(rec, q + lseq) is None:
        return HBAM_EFORMAT
    if lseq and rec[q] != 0xff and max(rec[q:q + lseq]) > 93:
        return HBAM_EREFID
    return HBAM_OK


def deferred(rec):
    """A valid record the device hands to the host: an H tag, or a float outside float_on_device."""
    for _, kind, v in sam_ref.decode_aux(sam_ref.fields(rec)["aux"]):
        if kind == "H":
            return True
        if kind == "f" and not float_on_device(v):
            return True
        if kind == "Bf" and not all(float_on_device(x) for x in v):
            return True
    return False


def line(rec, names):
    """A valid record's SAM line with its '\\n'."""
    f = sam_ref.fields(rec)
    rname = names[f["ref"]] if f["ref"] >= 0 else b"*"
    if f["nref"] >= 0 and f["nref"] == f["ref"]:
        rnext = b"="
    else:
        rnext = names[f["nref"]] if f["nref"] >= 0 else b"*"
    cigar = b"".join(b"%d%c" % (w >> 4, sam_ref.CIGAR_OPS[w & 15]) for w in f["cigar"]) or b"*"
    ls = f["l_seq"]
    if ls == 0:
        seq = qual = b"*"
    else:
        packed = np.frombuffer(f["seq"], np.uint8)
        nib = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:ls]  # high nibble first
        seq = np.frombuffer(sam_ref.SEQ_TABLE, np.uint8)[nib].tobytes()
        q = np.frombuffer(f["qual"], np.uint8)
        qual = b"*" if q[0] == 0xff else (q.astype(np.uint16) + 33).astype(np.uint8).tobytes()
    cols = [f["name"], b"%d" % f["flag"], rname, b"%d" % sam_ref._i32(f["pos"] + 1), b"%d" % f["mapq"], cigar,
            rnext, b"%d" % sam_ref._i32(f["npos"] + 1), b"%d" % f["tlen"], seq, qual]
    for tag, kind, v in sam_ref.decode_aux(f["aux"]):
        if kind == "i":
            cols.append(tag + b":i:%d" % v)
        elif kind == "f":
            cols.append(tag + b":f:" + java_float(v).encode())
        elif kind in "AZH":
            cols.append(tag + b":" + kind.encode() + b":" + v)
        else:
            vals = [java_float(x).encode() if kind == "Bf" else b"%d" % x for x in v]
            cols.append(tag + b":B:" + b",".join([kind[1:].encode()] + vals))
    return b"\t".join(cols) + b"\n"


def render(records, names, n_ref=None):
    """What hbam_sam_render returns for these records (the bytes of each one's rec_off slot), from
    the rules: n, status, the device text (a deferred
    record's line empty), line_off, the deferred positions, and `full`, every line rendered (what
    a writer puts out once the deferred lines are spliced in).  The first failing record ends it."""
    n_ref = len(names) if n_ref is None else n_ref
    out = dict(n=0, status=HBAM_OK, lines=[], full=[], deferred=[])
    for k, rec in enumerate(records):
        st = status(rec, n_ref)
        if st != HBAM_OK:
            out["status"] = st
            break
        bs = struct.unpack_from("<i", rec, 0)[0]
        rec = bytes(rec[:4 + bs])
        ln = line(rec, names)
        d = deferred(rec)
        if d:
            out["deferred"].append(k)
        out["lines"].append(b"" if d else ln)
        out["full"].append(ln)
        out["n"] += 1
    out["text"] = b"".join(out["lines"])
    lo = np.zeros(out["n"] + 1, np.uint64)
    lo[1:] = np.cumsum([len(x) for x in out["lines"]])
    out["line_off"] = lo
    return out
