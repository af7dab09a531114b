"""ctypes binding of libhbam.so (include/hbam.h).

The product path is the HIP library only: if libhbam.so is missing or cannot create a
device context, calls raise HbamUnavailable — there is no CPU fallback.
"""
import ctypes as C
import sys
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # hadoop-bam_amd/
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.path.join(PKG_ROOT, "libhbam.so")

HBAM_OK = 0
HBAM_EIO = -1
HBAM_ETRUNC = -2
HBAM_EFORMAT = -3
HBAM_ERUNTIMEIO = -4
HBAM_EEOF = -5
HBAM_EREFID = -6
HBAM_EDATA = -7
HBAM_ENOMEM = -8
HBAM_EUNSUPPORTED = -9
HBAM_EDEVICE = -10
HBAM_EINVAL = -11
HBAM_EMORE = -12
HBAM_EINDEX = -13
HBAM_ETRIBBLE = -14
HBAM_ERUNTIME = -15
HBAM_ENULL = -16
HBAM_ECLASSCAST = -17
HBAM_ESEQFORMAT = -18
HBAM_ENUMBER = -19
HBAM_QUAL_SANGER, HBAM_QUAL_ILLUMINA = 0, 1

CODE_NAMES = {
    HBAM_OK: "OK", HBAM_EIO: "IOException", HBAM_ETRUNC: "FileTruncatedException",
    HBAM_EFORMAT: "SAMFormatException", HBAM_ERUNTIMEIO: "RuntimeIOException",
    HBAM_EEOF: "RuntimeEOFException", HBAM_EREFID: "IllegalArgumentException",
    HBAM_EDATA: "RuntimeException(DataFormatException)", HBAM_ENOMEM: "OutOfMemory",
    HBAM_EUNSUPPORTED: "Unsupported", HBAM_EDEVICE: "DeviceError", HBAM_EINVAL: "InvalidArgument",
    HBAM_EMORE: "NeedMoreData", HBAM_EINDEX: "IndexOutOfBoundsException",
    HBAM_ETRIBBLE: "TribbleException", HBAM_ERUNTIME: "RuntimeException",
    HBAM_ENULL: "NullPointerException", HBAM_ECLASSCAST: "ClassCastException",
    HBAM_ESEQFORMAT: "FormatException", HBAM_ENUMBER: "NumberFormatException",
}

# every entry point include/hbam.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "hbam_create", "hbam_destroy", "hbam_last_error", "hbam_stream", "hbam_get_timing",
    "hbam_upload", "hbam_device_free", "hbam_parse_header", "hbam_scan_blocks", "hbam_inflate",
    "hbam_decode_split", "hbam_columns_to_host", "hbam_free_host_columns",
    "hbam_release_columns", "hbam_guess_bam_record_start", "hbam_guess_batch",
    "hbam_guess_bgzf_block_start", "hbam_probabilistic_splits",
    "hbam_sort_keys", "hbam_gather_records", "hbam_permute", "hbam_splitting_index",
    "hbam_bgzf_block_index", "hbam_resolve_tokens", "hbam_split_open", "hbam_split_next",
    "hbam_split_stats", "hbam_split_close", "hbam_device_alloc", "hbam_sort_split",
    "hbam_sort_partition", "hbam_sort_received", "hbam_bgzf_bound", "hbam_bgzf_compress",
    "hbam_summarize_ranges", "hbam_name_order", "hbam_fixmate", "hbam_download",
    "hbam_guess_window_len", "hbam_guess_windows", "hbam_guess_bgzf_window_len",
    "hbam_guess_bgzf_window", "hbam_probabilistic_splits_windows", "hbam_merge_remap",
    "hbam_host_register", "hbam_host_unregister", "hbam_bcf_parse_header", "hbam_guess_bcf_window_len",
    "hbam_guess_bcf_windows", "hbam_bcf_decode_split", "hbam_comm_unique_id", "hbam_comm_init",
    "hbam_comm_destroy", "hbam_comm_split_points", "hbam_sort_exchange", "hbam_split_open_reader",
    "hbam_split_read_bytes", "hbam_rewrite_groups", "hbam_records_to_host", "hbam_split_records_to_host",
    "hbam_bai_bound", "hbam_bai_build", "hbam_overlap_filter",
    "hbam_vcf_decode_split", "hbam_vcf_columns_to_host", "hbam_vcf_release", "hbam_vcf_gather_lines",
    "hbam_sam_decode_split", "hbam_sam_render",
    "hbam_fastq_decode_split", "hbam_qseq_decode_split", "hbam_frag_columns_to_host", "hbam_frag_release",
    "hbam_frag_render",
    "hbam_bcf_header_text", "hbam_vcf_render",
    "hbam_fasta_sections", "hbam_fasta_decode_split", "hbam_fasta_columns_to_host", "hbam_fasta_release",
    "hbam_chain_table",
    "hbam_summarize_reduce", "hbam_summary_keys", "hbam_summary_gather_lines", "hbam_device_copy",
]

# hbam_read_fn: int64_t read(void* user, uint64_t offset, uint64_t len, uint8_t* dst)
READ_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)


class HbamUnavailable(RuntimeError):
    pass


class Opts(C.Structure):
    _fields_ = [("check_crc", C.c_int32), ("validate_refs", C.c_int32),
                ("reserved", C.c_int32 * 14)]


class Header(C.Structure):
    _fields_ = [("l_text", C.c_int32), ("n_ref", C.c_int32), ("header_ulen", C.c_uint64),
                ("first_voffset", C.c_uint64)]


class Block(C.Structure):
    _fields_ = [("coff", C.c_uint64), ("clen", C.c_uint32), ("isize", C.c_uint32),
                ("crc", C.c_uint32), ("pad", C.c_uint32)]


class ChainInfo(C.Structure):
    _fields_ = [("n_blocks", C.c_uint64), ("end_pos", C.c_uint64), ("end_code", C.c_int32),
                ("sparse", C.c_int32), ("fallback_flags", C.c_uint32), ("pad", C.c_uint32),
                ("sparse_calls", C.c_uint64), ("dense_calls", C.c_uint64)]


class Timing(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("scan_ms", "inflate_ms", "crc_ms", "walk_ms",
                                          "decode_ms", "pools_ms", "total_ms",
                                          "huffman_ms", "resolve_ms")] + \
               [(n, C.c_uint64) for n in ("n_blocks", "comp_bytes", "ubuf_bytes", "n_records",
                                          "pool_bytes")] + [("exchange_ms", C.c_double)]


class SortedRunC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("payload_bytes", C.c_uint64), ("key", C.c_void_p),
                ("voffset", C.c_void_p), ("block_size", C.c_void_p), ("offsets", C.c_void_p),
                ("payload", C.c_void_p)]


class RangesC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32), ("key", C.c_void_p),
                ("beg", C.c_void_p), ("end", C.c_void_p), ("rev", C.c_void_p), ("record", C.c_void_p)]


class FixmateRunC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("payload_bytes", C.c_uint64), ("n_groups", C.c_uint64),
                ("status", C.c_int32), ("pad", C.c_int32), ("src", C.c_void_p), ("mate", C.c_void_p),
                ("offsets", C.c_void_p), ("payload", C.c_void_p)]


class SummaryC(C.Structure):
    _fields_ = [("n_streams", C.c_uint64), ("n_lines", C.c_uint64), ("text_len", C.c_uint64),
                ("n_segments", C.c_uint64), ("first", C.c_void_p), ("rid", C.c_void_p), ("beg", C.c_void_p),
                ("end", C.c_void_p), ("count", C.c_void_p), ("text", C.c_void_p), ("text_off", C.c_void_p)]


class SummaryLinesC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32), ("text", C.c_void_p),
                ("start", C.c_void_p), ("len", C.c_void_p), ("key", C.c_void_p)]


class BcfHeaderC(C.Structure):
    _fields_ = [("n_contig", C.c_int32), ("n_sample", C.c_int32), ("n_dict", C.c_int32),
                ("bgzf", C.c_int32), ("header_len", C.c_uint64), ("first_voffset", C.c_uint64)]


_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


class Columns(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("status", C.c_int32), ("pad0", C.c_int32),
        ("err_record", C.c_uint64), ("voffset", _u64p), ("key", _i64p), ("rec_off", _u64p),
        ("ubuf", _u8p), ("ubuf_len", C.c_uint64), ("block_size", _i32p), ("ref_id", _i32p),
        ("pos", _i32p), ("l_read_name", _u8p), ("mapq", _u8p), ("bin", _u16p),
        ("n_cigar", _u16p), ("flag", _u16p), ("l_seq", _i32p), ("next_ref_id", _i32p),
        ("next_pos", _i32p), ("tlen", _i32p), ("layout_ok", _u8p), ("name_off", _u64p),
        ("names", _u8p), ("cigar_off", _u64p), ("cigars", _u32p), ("seq_off", _u64p),
        ("seq", _u8p), ("qual", _u8p), ("aux_off", _u64p), ("aux", _u8p),
    ]


class BcfColumnsC(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("status", C.c_int32), ("pad0", C.c_int32),
        ("err_record", C.c_uint64), ("rel", C.c_void_p), ("rec_off", C.c_void_p), ("data", C.c_void_p),
        ("data_len", C.c_uint64), ("key", C.c_void_p), ("l_shared", C.c_void_p), ("l_indiv", C.c_void_p),
        ("chrom", C.c_void_p), ("pos", C.c_void_p), ("rlen", C.c_void_p), ("qual", C.c_void_p),
        ("n_allele_info", C.c_void_p), ("n_fmt_sample", C.c_void_p),
    ]


BCF_FIELDS = [("rel", np.int64), ("rec_off", np.uint64), ("key", np.int64), ("l_shared", np.int32),
              ("l_indiv", np.int32), ("chrom", np.int32), ("pos", np.int32), ("rlen", np.int32),
              ("qual", np.uint32), ("n_allele_info", np.int32), ("n_fmt_sample", np.int32)]


class VcfContigC(C.Structure):
    _fields_ = [("name_off", C.c_uint32), ("name_len", C.c_uint32), ("ordinal", C.c_int32)]


class VcfColumnsC(C.Structure):
    _fields_ = [
        ("n", C.c_uint64), ("status", C.c_int32), ("host", C.c_int32), ("line_off", C.c_void_p),
        ("line_len", C.c_void_p), ("tab", C.c_void_p), ("chrom", C.c_void_p), ("pos", C.c_void_p),
        ("ref_len", C.c_void_p), ("key", C.c_void_p), ("text", C.c_void_p), ("text_base", C.c_uint64),
        ("text_len", C.c_uint64),
    ]


class SamTextC(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32), ("err_record", C.c_uint64),
        ("text_len", C.c_uint64), ("text", C.c_void_p), ("line_off", C.c_void_p), ("n_deferred", C.c_uint64),
        ("deferred", C.c_void_p),
    ]


class VcfMetaC(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("contig_names", "contig_off", "dict_names", "dict_off", "dict_rank",
                                          "dict_flags", "dict_number")]


# hbam_vcf_meta.dict_flags / dict_number (include/hbam.h)
HBAM_VCF_HAS_INFO, HBAM_VCF_INFO_FLAG, HBAM_VCF_HAS_FORMAT, HBAM_VCF_KIND_SHIFT = 1, 2, 4, 4
HBAM_VCF_KINDS = {"GT": 1, "DP": 2, "GQ": 3, "AD": 4, "PL": 5, "FT": 6}
HBAM_VCF_NUMBER = {".": -1, "A": -2, "R": -3, "G": -4}
HBAM_VCF_MAX_INFO, HBAM_VCF_MAX_FILTER, HBAM_VCF_MAX_FORMAT, HBAM_VCF_MAX_PLOIDY = 64, 64, 16, 16
HBAM_VCF_WAVE_SAMPLES = 64


class FragColumnsC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("status", C.c_int32), ("host", C.c_int32), ("err_pos", C.c_uint64),
                ("first_pos", C.c_uint64), ("end_pos", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("rec_off", "pos_after", "present", "run", "lane", "tile", "xpos", "ypos",
                                          "read", "filter_passed", "control", "instrument", "flowcell", "index",
                                          "key_off", "seq_off", "qual_off", "key", "seq", "qual")] + \
               [("key_len", C.c_uint64), ("seq_len", C.c_uint64), ("qual_len", C.c_uint64),
                ("text_base", C.c_uint64)]


class FastaColumnsC(C.Structure):
    _fields_ = [("n", C.c_uint64), ("status", C.c_int32), ("host", C.c_int32), ("err_pos", C.c_uint64),
                ("first_pos", C.c_uint64), ("end_pos", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("rec_off", "pos_after", "position", "line_len", "key_off", "seq_off",
                                          "key", "seq")] + \
               [("key_len", C.c_uint64), ("seq_len", C.c_uint64), ("index_off", C.c_uint32),
                ("index_len", C.c_uint32), ("text_base", C.c_uint64)]


FASTA_FIELDS = [("rec_off", np.uint64), ("pos_after", np.uint64), ("position", np.int32), ("line_len", np.uint32)]


class FragTextC(C.Structure):
    _fields_ = [
        ("n_records", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32), ("err_record", C.c_uint64),
        ("text_len", C.c_uint64), ("partial_len", C.c_uint64), ("text", C.c_void_p), ("line_off", C.c_void_p),
    ]


HBAM_FRAG_FASTQ, HBAM_FRAG_QSEQ = 0, 1
HBAM_FRAG_USE_KEY, HBAM_FRAG_INDEX_DOTS = 1, 2

# SequencedFragment's *_Present bits, in hbam_frag_columns.present's order
FRAG_PRESENT = {"instrument": 0x001, "run": 0x002, "flowcell": 0x004, "lane": 0x008, "tile": 0x010,
                "xpos": 0x020, "ypos": 0x040, "read": 0x080, "filter_passed": 0x100, "control": 0x200,
                "index": 0x400}
FRAG_FIELDS = [("rec_off", np.uint64), ("pos_after", np.uint64), ("present", np.uint32), ("run", np.int32),
               ("lane", np.int32), ("tile", np.int32), ("xpos", np.int32), ("ypos", np.int32),
               ("read", np.int32), ("filter_passed", np.int32), ("control", np.int32)]


VCF_FIELDS = [("line_off", np.uint64), ("line_len", np.uint32), ("chrom", np.int32), ("pos", np.int32),
              ("ref_len", np.int32), ("key", np.int64)]


FIXED = [("voffset", np.uint64), ("key", np.int64), ("rec_off", np.uint64),
         ("block_size", np.int32), ("ref_id", np.int32), ("pos", np.int32),
         ("l_read_name", np.uint8), ("mapq", np.uint8), ("bin", np.uint16),
         ("n_cigar", np.uint16), ("flag", np.uint16), ("l_seq", np.int32),
         ("next_ref_id", np.int32), ("next_pos", np.int32), ("tlen", np.int32),
         ("layout_ok", np.uint8)]

_LIB = None


def load(path=None):
    """Load libhbam.so (raises HbamUnavailable if it is not built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = path or os.environ.get("HBAM_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise HbamUnavailable("libhbam.so not built (run __graft_entry__.build())")
    L = C.CDLL(path)
    vp = C.c_void_p
    sig = {
        "hbam_create": (vp, [C.c_int, C.POINTER(Opts)]),
        "hbam_destroy": (None, [vp]),
        "hbam_last_error": (C.c_char_p, [vp]),
        "hbam_stream": (vp, [vp]),
        "hbam_get_timing": (C.c_int, [vp, C.POINTER(Timing)]),
        "hbam_upload": (C.c_int, [vp, vp, C.c_uint64, C.POINTER(vp)]),
        "hbam_device_free": (C.c_int, [vp, vp]),
        "hbam_download": (C.c_int, [vp, vp, C.c_uint64, vp]),
        "hbam_parse_header": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.POINTER(Header)]),
        "hbam_scan_blocks": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64,
                                       C.POINTER(Block), C.c_uint64, C.POINTER(C.c_uint64)]),
        "hbam_chain_table": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                       C.POINTER(Block), C.c_uint64, C.POINTER(ChainInfo)]),
        "hbam_inflate": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.POINTER(Block), C.c_uint64,
                                   C.c_int, vp, C.c_uint64, vp, vp]),
        "hbam_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                        C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(Columns)]),
        "hbam_columns_to_host": (C.c_int, [vp, C.POINTER(Columns), C.POINTER(Columns)]),
        "hbam_free_host_columns": (None, [C.POINTER(Columns)]),
        "hbam_records_to_host": (C.c_int, [vp, C.POINTER(Columns), C.POINTER(Columns)]),
        "hbam_split_records_to_host": (C.c_int, [vp, C.POINTER(Columns), C.POINTER(Columns)]),
        "hbam_release_columns": (None, [vp, C.POINTER(Columns)]),
        "hbam_guess_bam_record_start": (C.c_int64, [vp, vp, C.c_int, C.c_uint64, C.c_int64,
                                                    C.c_int64, C.c_int32, _i32p]),
        "hbam_guess_batch": (C.c_int, [vp, vp, C.c_int, C.c_uint64, vp, vp, C.c_uint64,
                                       C.c_int32, vp, vp]),
        "hbam_guess_bgzf_block_start": (C.c_int64, [vp, vp, C.c_int, C.c_uint64, C.c_int64,
                                                    C.c_int64, _i32p]),
        "hbam_probabilistic_splits": (C.c_int64, [vp, vp, C.c_int, C.c_uint64, vp, vp,
                                                  C.c_uint64, vp, vp]),
        "hbam_guess_window_len": (C.c_uint64, [C.c_uint64, C.c_int64, C.c_int64]),
        "hbam_guess_bgzf_window_len": (C.c_uint64, [C.c_uint64, C.c_int64, C.c_int64]),
        "hbam_guess_windows": (C.c_int, [vp, vp, C.c_int, vp, C.c_uint64, vp, vp, C.c_uint64,
                                         C.c_int32, vp, vp]),
        "hbam_guess_bgzf_window": (C.c_int64, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int64,
                                               C.c_int64, _i32p]),
        "hbam_probabilistic_splits_windows": (C.c_int64, [vp, vp, C.c_uint64, vp, C.c_int, vp,
                                                          C.c_uint64, vp, vp, C.c_uint64, vp, vp]),
        "hbam_sort_keys": (C.c_int, [vp, vp, C.c_uint64, vp, vp]),
        "hbam_gather_records": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp,
                                          C.POINTER(C.c_uint64)]),
        "hbam_permute": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint64, vp]),
        "hbam_splitting_index": (C.c_int64, [vp, C.POINTER(Columns), C.c_int32, C.c_uint64, vp,
                                             C.c_uint64]),
        "hbam_bgzf_block_index": (C.c_int64, [vp, vp, C.c_int, C.c_uint64, C.c_int32, vp,
                                              C.c_uint64]),
        "hbam_resolve_tokens": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, _i32p]),
        "hbam_split_open": (vp, [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint64]),
        "hbam_split_next": (C.c_int, [vp, C.POINTER(Columns)]),
        "hbam_split_open_reader": (vp, [vp, READ_FN, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32,
                                        C.c_uint64]),
        "hbam_split_read_bytes": (C.c_uint64, [vp]),
        "hbam_rewrite_groups": (C.c_int, [vp, C.POINTER(Columns), vp, C.c_uint64, _i32p, C.POINTER(C.c_uint64)]),
        "hbam_split_stats": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                       C.POINTER(C.c_uint64)]),
        "hbam_split_close": (None, [vp]),
        "hbam_device_alloc": (C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
        "hbam_sort_split": (C.c_int, [vp, C.POINTER(Columns), C.POINTER(SortedRunC)]),
        "hbam_sort_partition": (C.c_int, [vp, C.POINTER(SortedRunC), vp, C.c_uint32, vp, vp]),
        "hbam_sort_received": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(SortedRunC)]),
        "hbam_merge_remap": (C.c_int, [vp, C.POINTER(Columns), vp, C.c_int32, C.POINTER(C.c_uint64)]),
        "hbam_host_register": (C.c_int, [vp, vp, C.c_uint64]),
        "hbam_host_unregister": (C.c_int, [vp, vp]),
        "hbam_bgzf_bound": (C.c_uint64, [C.c_uint64, C.c_uint32]),
        "hbam_bcf_parse_header": (C.c_int, [vp, vp, C.c_uint64, C.POINTER(BcfHeaderC)]),
        "hbam_guess_bcf_window_len": (C.c_uint64, [C.c_uint64, C.c_int64, C.c_int64, C.c_int]),
        "hbam_guess_bcf_windows": (C.c_int, [vp, vp, C.c_int, vp, C.c_uint64, vp, vp, C.c_uint64,
                                             C.POINTER(BcfHeaderC), vp, vp]),
        "hbam_bcf_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.POINTER(BcfHeaderC), C.c_uint64, C.c_uint64,
                                            C.POINTER(BcfColumnsC)]),
        "hbam_summarize_ranges": (C.c_int, [vp, C.POINTER(Columns), C.POINTER(RangesC)]),
        "hbam_summarize_reduce": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int,
                                            C.POINTER(SummaryC)]),
        "hbam_device_copy": (C.c_int, [vp, vp, vp, C.c_uint64]),
        "hbam_summary_keys": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.POINTER(SummaryLinesC)]),
        "hbam_summary_gather_lines": (C.c_int, [vp, C.POINTER(SummaryLinesC), vp, C.c_uint64, vp, C.c_uint64, vp,
                                                C.POINTER(C.c_uint64)]),
        "hbam_name_order": (C.c_int, [vp, vp, vp, C.c_uint64, vp]),
        "hbam_fixmate": (C.c_int, [vp, vp, vp, C.c_uint64, C.POINTER(FixmateRunC)]),
        "hbam_bgzf_compress": (C.c_int64, [vp, vp, C.c_int, C.c_uint64, C.c_uint32, vp, C.c_int,
                                           C.c_uint64]),
        "hbam_comm_unique_id": (C.c_int, [vp]),
        "hbam_comm_init": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.POINTER(vp)]),
        "hbam_comm_destroy": (None, [vp]),
        "hbam_comm_split_points": (C.c_int, [vp, vp, C.POINTER(SortedRunC), C.c_uint32, vp]),
        "hbam_sort_exchange": (C.c_int, [vp, vp, C.POINTER(SortedRunC), vp, C.POINTER(SortedRunC)]),
        "hbam_bai_bound": (C.c_uint64, [C.c_uint64, C.c_int32]),
        "hbam_bai_build": (C.c_int64, [vp, C.POINTER(Columns), C.c_int32, C.c_uint64, vp, C.c_uint64,
                                       C.POINTER(C.c_uint64)]),
        "hbam_overlap_filter": (C.c_int64, [vp, C.POINTER(Columns), C.c_int32, C.c_int64, C.c_int64,
                                            C.c_int32, vp]),
        "hbam_vcf_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, C.c_int32,
                                            C.POINTER(VcfColumnsC)]),
        "hbam_vcf_columns_to_host": (C.c_int, [vp, C.POINTER(VcfColumnsC), C.POINTER(VcfColumnsC)]),
        "hbam_vcf_release": (None, [vp, C.POINTER(VcfColumnsC)]),
        "hbam_vcf_gather_lines": (C.c_int, [vp, C.POINTER(VcfColumnsC), vp, C.c_uint64, vp, C.c_uint64, vp,
                                            C.POINTER(C.c_uint64)]),
        "hbam_sam_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, C.c_int32,
                                            C.POINTER(Columns)]),
        "hbam_sam_render": (C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_int, vp, vp, C.c_int32, C.POINTER(SamTextC)]),
        "hbam_bcf_header_text": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
        "hbam_vcf_render": (C.c_int, [vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_int, C.POINTER(BcfHeaderC),
                                      C.POINTER(VcfMetaC), C.POINTER(SamTextC)]),
        "hbam_fastq_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                              C.c_uint64, C.c_int32, C.c_int32, C.POINTER(FragColumnsC)]),
        "hbam_qseq_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                             C.c_uint64, C.c_int32, C.c_int32, C.POINTER(FragColumnsC)]),
        "hbam_frag_columns_to_host": (C.c_int, [vp, C.POINTER(FragColumnsC), C.POINTER(FragColumnsC)]),
        "hbam_frag_release": (None, [vp, C.POINTER(FragColumnsC)]),
        "hbam_frag_render": (C.c_int, [vp, C.POINTER(FragColumnsC), vp, C.c_int, C.c_uint64, vp, C.c_uint64,
                                       C.c_int32, C.c_int32, C.c_uint32, C.POINTER(FragTextC)]),
        "hbam_fasta_sections": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_uint64,
                                          C.POINTER(C.c_uint64)]),
        "hbam_fasta_decode_split": (C.c_int, [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                              C.c_uint64, C.POINTER(FastaColumnsC)]),
        "hbam_fasta_columns_to_host": (C.c_int, [vp, C.POINTER(FastaColumnsC), C.POINTER(FastaColumnsC)]),
        "hbam_fasta_release": (None, [vp, C.POINTER(FastaColumnsC)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name, None)
        if f is None:  # an older build (A/B runs): only what it exports is bound
            continue
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


def bgzf_blocks(data, start=0):
    """Host walk of the BGZF chain of `data` (bytes / numpy / memmap) from file offset `start`:
    yields (coff, clen, isize, crc) per block, one Python iteration and 26 bytes read each, and
    stops at the end of the data or at a block the readers would not accept (gzip magic, the BC
    subfield, BSIZE inside the data: [htsjdk] BlockCompressedInputStream.readBlock's checks)."""
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
    n, p = len(a), int(start)
    while p + 18 <= n:
        h = a[p:p + 18].tobytes()
        if h[:4] != b"\x1f\x8b\x08\x04" or h[10:16] != b"\x06\x00BC\x02\x00":
            return
        clen = (h[16] | h[17] << 8) + 1
        if clen < 26 or p + clen > n:
            return
        crc, isize = (int(x) for x in np.frombuffer(a[p + clen - 8:p + clen].tobytes(), "<u4"))
        yield p, clen, isize, crc
        p += clen


def host_columns_to_numpy(h):
    """Copy a host hbam_columns into a dict of numpy arrays."""
    n = int(h.n_records)
    out = {"n": n, "status": int(h.status), "err_record": int(h.err_record)}
    for name, dt in FIXED:
        p = getattr(h, name)
        out[name] = np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)
    for name in ("name_off", "cigar_off", "seq_off", "aux_off"):
        p = getattr(h, name)
        out[name] = np.ctypeslib.as_array(p, shape=(n + 1,)).copy() if p else np.zeros(1, np.uint64)
    ul = int(h.ubuf_len)
    out["ubuf"] = np.ctypeslib.as_array(h.ubuf, shape=(ul,)).copy() if (ul and h.ubuf) else np.zeros(0, np.uint8)
    pools = [("names", np.uint8, "name_off"), ("cigars", np.uint32, "cigar_off"),
             ("seq", np.uint8, "seq_off"), ("qual", np.uint8, "seq_off"),
             ("aux", np.uint8, "aux_off")]
    for name, dt, off in pools:
        m = int(out[off][-1]) if n else 0
        p = getattr(h, name)
        out[name] = np.ctypeslib.as_array(p, shape=(m,)).astype(dt).copy() if m else np.zeros(0, dt)
    return out


def _host_array(ptr, count, dt):
    """A copy of `count` elements of dtype `dt` at a host pointer of any ctypes pointer type."""
    if not count:
        return np.zeros(0, dt)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)),
                                 shape=(count * np.dtype(dt).itemsize,)).view(dt).copy()


class DeviceBuffer:
    """Device bytes the library allocated (Context.upload: freed by free()) or owns (a view of a
    call's output, valid until the context's next call of that kind): ptr, nbytes, and 64 readable
    bytes behind them.  Accepted wherever a call takes bytes / numpy / a device tensor."""

    def __init__(self, ctx, ptr, nbytes, owned):
        self.ctx, self.ptr, self.nbytes, self.owned = ctx, int(ptr or 0), int(nbytes), owned

    def free(self):
        if self.owned and self.ptr and self.ctx.h:
            self.ctx.L.hbam_device_free(self.ctx.h, C.c_void_p(self.ptr))
        self.ptr, self.owned = 0, False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One device context (hbam_ctx): a HIP stream plus device work buffers."""

    def __init__(self, device=0, check_crc=False, validate_refs=True):
        self.L = load()
        # PyTorch-ROCm ships its own HIP runtime; when both live in one process, torch's must
        # open the device first (the other order leaves torch with "No HIP GPUs").
        if "torch" in sys.modules:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        o = Opts()
        o.check_crc = int(check_crc)
        o.validate_refs = int(validate_refs)
        self.h = self.L.hbam_create(device, C.byref(o))
        if not self.h:
            raise HbamUnavailable("hbam_create failed: no HIP device %d" % device)

    def close(self):
        if getattr(self, "h", None):
            self.L.hbam_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self.L.hbam_last_error(self.h).decode(errors="replace")

    def timing(self):
        t = Timing()
        self.L.hbam_get_timing(self.h, C.byref(t))
        return {n: getattr(t, n) for n, _ in Timing._fields_}

    @staticmethod
    def _ptr(data, output=False):
        """(pointer, length, on_device, keepalive) for bytes / numpy / torch cuda tensor.  An
        output buffer (the library writes into it) is never replaced by a padded copy."""
        if isinstance(data, DeviceBuffer):
            return C.c_void_p(data.ptr), data.nbytes, 1, data
        if hasattr(data, "data_ptr") and hasattr(data, "is_cuda"):
            if data.is_cuda:
                # libhbam reads the raw pointer on its own stream: the bytes must be one dense
                # run, and whatever torch is still producing into them (a torch.cat, a .to(dev),
                # an all_to_all) must be finished first
                if not data.is_contiguous():
                    raise ValueError("device input must be contiguous")
                import torch
                nbytes = data.numel() * data.element_size()
                # the kernels read whole 16-byte quads and fixed windows past the last byte: 64
                # readable bytes must follow (include/hbam.h); a view that ends at (or near) the end
                # of its allocation is copied into a padded buffer first
                room = data.untyped_storage().nbytes() - data.storage_offset() * data.element_size()
                if room < nbytes + 64 and not output:
                    pad = torch.zeros(nbytes + 64, dtype=torch.uint8, device=data.device)
                    pad[:nbytes].copy_(data.reshape(-1).view(torch.uint8))
                    data = pad
                torch.cuda.current_stream(data.device).synchronize()
                return C.c_void_p(data.data_ptr()), nbytes, 1, data
            a = data.numpy()
        elif isinstance(data, np.ndarray):
            a = np.ascontiguousarray(data, dtype=np.uint8)
        else:
            a = np.frombuffer(bytes(data), dtype=np.uint8)
        if a.size == 0:
            a = np.zeros(1, np.uint8)
            return C.c_void_p(a.ctypes.data), 0, 0, a
        return C.c_void_p(a.ctypes.data), a.size, 0, a

    def upload(self, data):
        """hbam_upload: a device copy of `data` (bytes / numpy) -> DeviceBuffer; free() it."""
        p, n, dev, keep = self._ptr(data)
        d = C.c_void_p()
        rc = self.L.hbam_upload(self.h, p, n, C.byref(d))
        if rc:
            raise RuntimeError("hbam_upload failed (%d): %s" % (rc, self.last_error()))
        return DeviceBuffer(self, d.value, n, True)

    def bgzf_compress(self, data, block_size=0, out=None):
        """BlockCompressedOutputStream over `data` (bytes / numpy / torch tensor, host or device)
        with the device deflate (hbam_bgzf_compress): the BGZF members, no terminator.  Returns
        a numpy uint8 array, or writes into the device tensor `out` and returns its length."""
        p, n, dev, keep = self._ptr(data)
        bound = int(self.L.hbam_bgzf_bound(n, block_size))
        if out is not None:
            q, cap, odev, okeep = self._ptr(out, output=True)
            r = self.L.hbam_bgzf_compress(self.h, p, dev, n, block_size, q, odev, cap)
            if r < 0:
                raise RuntimeError("hbam_bgzf_compress failed (%d): %s" % (r, self.last_error()))
            return int(r)
        buf = np.empty(max(bound, 1), np.uint8)
        r = self.L.hbam_bgzf_compress(self.h, p, dev, n, block_size, C.c_void_p(buf.ctypes.data), 0, bound)
        if r < 0:
            raise RuntimeError("hbam_bgzf_compress failed (%d): %s" % (r, self.last_error()))
        return buf[:r]

    def parse_header(self, data):
        p, n, dev, keep = self._ptr(data)
        h = Header()
        rc = self.L.hbam_parse_header(self.h, p, dev, n, C.byref(h))
        if rc:
            return rc
        return dict(l_text=h.l_text, n_ref=h.n_ref, header_ulen=h.header_ulen,
                    first_voffset=h.first_voffset)

    def scan_blocks(self, data, base_off=0):
        p, n, dev, keep = self._ptr(data)
        cap = n // 18 + 2
        arr = (Block * cap)()
        nb = C.c_uint64(0)
        rc = self.L.hbam_scan_blocks(self.h, p, dev, n, base_off, arr, cap, C.byref(nb))
        k = int(nb.value)
        out = dict(coff=np.array([arr[i].coff for i in range(k)], np.uint64),
                   clen=np.array([arr[i].clen for i in range(k)], np.uint32),
                   isize=np.array([arr[i].isize for i in range(k)], np.uint32),
                   crc=np.array([arr[i].crc for i in range(k)], np.uint32))
        return rc, out

    def chain_table(self, data, start=0, window_is_file_end=True):
        """hbam_chain_table: the block table of the chain from `start` of the window `data`, as
        the decoders build it -> dict(coff, clen, isize, crc, nb, end_pos, end_code, sparse,
        fallback_flags, sparse_calls, dense_calls)."""
        p, n, dev, keep = self._ptr(data)
        info = ChainInfo()
        cap = n // 18 + 2
        if cap > 1 << 20:  # a large window: count first (a second chain build) instead of n / 18 rows
            rc = self.L.hbam_chain_table(self.h, p, dev, n, int(start), int(bool(window_is_file_end)),
                                         None, 0, C.byref(info))
            if rc:
                raise RuntimeError("hbam_chain_table failed (%d): %s" % (rc, self.last_error()))
            cap = int(info.n_blocks) + 1
        arr = np.zeros(cap, np.dtype([("coff", "<u8"), ("clen", "<u4"), ("isize", "<u4"),
                                      ("crc", "<u4"), ("pad", "<u4")]))
        rc = self.L.hbam_chain_table(self.h, p, dev, n, int(start), int(bool(window_is_file_end)),
                                     C.cast(C.c_void_p(arr.ctypes.data), C.POINTER(Block)), cap,
                                     C.byref(info))
        if rc:
            raise RuntimeError("hbam_chain_table failed (%d): %s" % (rc, self.last_error()))
        k = int(info.n_blocks)
        out = {f: arr[f][:k].copy() for f in ("coff", "clen", "isize", "crc")}
        out.update(nb=k, end_pos=int(info.end_pos), end_code=int(info.end_code), sparse=int(info.sparse),
                   fallback_flags=int(info.fallback_flags), sparse_calls=int(info.sparse_calls),
                   dense_calls=int(info.dense_calls))
        return out

    def chain_counters(self):
        """(sparse, dense) chain builds of this context so far, by every entry point."""
        info = ChainInfo()
        self.L.hbam_chain_table(self.h, None, 0, 0, 0, 1, None, 0, C.byref(info))
        return int(info.sparse_calls), int(info.dense_calls)

    def inflate(self, data, blocks, check_crc=True):
        p, n, dev, keep = self._ptr(data)
        k = len(blocks["coff"])
        arr = (Block * max(k, 1))()
        for i in range(k):
            arr[i].coff = int(blocks["coff"][i])
            arr[i].clen = int(blocks["clen"][i])
            arr[i].isize = int(blocks["isize"][i])
            arr[i].crc = int(blocks["crc"][i])
        total = int(np.sum(blocks["isize"], dtype=np.uint64)) if k else 0
        out = np.zeros(max(total, 1), np.uint8)
        off = np.zeros(k + 1, np.uint64)
        st = np.zeros(max(k, 1), np.int32)
        rc = self.L.hbam_inflate(self.h, p, dev, n, arr, k, int(check_crc),
                                 out.ctypes.data, out.size, off.ctypes.data, st.ctypes.data)
        return rc, out[:total], off, st[:k]

    def decode_split(self, data, v_start, v_end, n_ref=-1, comp_base=0, file_len=None):
        """BAMRecordReader over one FileVirtualSplit; returns host numpy columns."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = comp_base + n
        d = Columns()
        rc = self.L.hbam_decode_split(self.h, p, dev, comp_base, n, file_len, v_start, v_end,
                                      n_ref, C.byref(d))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        h = Columns()
        rc = self.L.hbam_columns_to_host(self.h, C.byref(d), C.byref(h))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        out = host_columns_to_numpy(h)
        self.L.hbam_free_host_columns(C.byref(h))
        out["rc"] = 0
        out["timing"] = self.timing()
        return out

    def split_stream(self, data, v_start, v_end, n_ref, window_bytes=1 << 30, host=True):
        """Streamed BAMRecordReader over a host-resident file (hbam_split_open/next): yields
        the host columns of each window in order; the last one carries the split's status.
        host=False yields each window's device Columns struct instead (valid until the next
        window is requested); host="records" the records-only copy (records_to_host: views, valid
        until the next window is requested)."""
        a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray)
                                 else data, dtype=np.uint8)
        keep = a if a.size else np.zeros(1, np.uint8)
        s = self.L.hbam_split_open(self.h, C.c_void_p(keep.ctypes.data), a.size, v_start, v_end,
                                   int(n_ref), int(window_bytes))
        if not s:
            raise HbamUnavailable("hbam_split_open failed: %s" % self.last_error())
        return self._stream(s, host, keep)

    def split_stream_reader(self, read, file_len, v_start, v_end, n_ref, window_bytes=1 << 30, host=True):
        """Split-local streamed BAMRecordReader (hbam_split_open_reader): read(offset, length) ->
        bytes is a positioned read of the file (os.pread, FSDataInputStream.read(long, ...)); only
        the blocks the split needs are requested.  Yields as split_stream."""
        def cb(user, off, n, dst):
            b = read(int(off), int(n))
            if not b:
                return -1
            if len(b) > n:  # never past the n bytes of staging the library asked to fill
                b = b[:n]
            C.memmove(dst, bytes(b), len(b))
            return len(b)
        fn = READ_FN(cb)
        s = self.L.hbam_split_open_reader(self.h, fn, None, int(file_len), v_start, v_end, int(n_ref),
                                          int(window_bytes))
        if not s:
            raise HbamUnavailable("hbam_split_open_reader failed: %s" % self.last_error())
        return self._stream(s, host, fn)

    def _stream(self, s, host, keep):
        try:
            while True:
                d = Columns()
                rc = self.L.hbam_split_next(s, C.byref(d))
                if rc < 0:
                    raise RuntimeError("hbam_split_next failed (%d): %s" % (rc, self.last_error()))
                if rc == 0:
                    return
                if not host:
                    yield d
                    continue
                if host == "records":
                    yield self.records_to_host(d, stream=s)
                    continue
                h = Columns()
                rc = self.L.hbam_columns_to_host(self.h, C.byref(d), C.byref(h))
                if rc:
                    raise RuntimeError("hbam_columns_to_host failed (%d): %s" % (rc, self.last_error()))
                out = host_columns_to_numpy(h)
                self.L.hbam_free_host_columns(C.byref(h))
                yield out
        finally:
            self.last_stream_stats = self._split_stats(s)
            self.L.hbam_split_close(s)
            del keep

    def records_to_host(self, d, stream=None):
        """hbam_records_to_host: what the drop-in reader hands out (key, voffset, rec_off, block_size
        and the records' bytes), as numpy VIEWS of the context's pinned staging — valid until the
        next call on this context; with `stream` (a split stream handle) hbam_split_records_to_host,
        views of that stream's own staging, valid until its next window or close whatever other
        readers of the context do.  d2h_bytes = what crossed PCIe."""
        h = Columns()
        if stream is not None:
            rc = self.L.hbam_split_records_to_host(stream, C.byref(d), C.byref(h))
        else:
            rc = self.L.hbam_records_to_host(self.h, C.byref(d), C.byref(h))
        if rc:
            raise RuntimeError("hbam_records_to_host failed (%d): %s" % (rc, self.last_error()))
        n = int(h.n_records)
        out = {"n": n, "status": int(h.status), "err_record": int(h.err_record)}
        for name, dt in (("voffset", np.uint64), ("key", np.int64), ("rec_off", np.uint64),
                         ("block_size", np.int32)):
            p = getattr(h, name)
            out[name] = np.ctypeslib.as_array(p, shape=(n,)).view(dt) if n else np.zeros(0, dt)
        ul = int(h.ubuf_len)
        out["ubuf"] = np.ctypeslib.as_array(h.ubuf, shape=(ul,)) if (ul and h.ubuf) else np.zeros(0, np.uint8)
        out["d2h_bytes"] = 28 * n + ul
        return out

    def _split_stats(self, s):
        b, w = C.c_uint64(0), C.c_uint64(0)
        ms = C.c_double(0)
        self.L.hbam_split_stats(s, C.byref(b), C.byref(ms), C.byref(w))
        return {"h2d_bytes": int(b.value), "h2d_ms": float(ms.value), "windows": int(w.value),
                "read_bytes": int(self.L.hbam_split_read_bytes(s))}

    def download(self, ptr, nbytes, dtype=np.uint8):
        """hbam_download: `nbytes` of device memory at address `ptr` -> numpy array of dtype."""
        a = np.empty(max(int(nbytes), 1), np.uint8)
        if nbytes:
            rc = self.L.hbam_download(self.h, C.c_void_p(int(ptr)), int(nbytes), C.c_void_p(a.ctypes.data))
            if rc:
                raise RuntimeError("hbam_download failed (%d): %s" % (rc, self.last_error()))
        return a[:int(nbytes)].view(dtype)

    def columns_slice(self, d, i0, i1):
        """Host copy of records [i0, i1) of device columns `d` (an hbam_decode_split /
        hbam_split_next result): the fixed columns and each record's SAMRecordWritable bytes."""
        n = max(0, int(i1) - int(i0))
        out = {"n": n}
        for name, dt in FIXED:
            sz = np.dtype(dt).itemsize
            p = C.cast(getattr(d, name), C.c_void_p).value
            out[name] = self.download(p + int(i0) * sz, n * sz, dt).copy() if n else np.zeros(0, dt)
        ub = C.cast(d.ubuf, C.c_void_p).value
        out["records"] = [self.download(ub + int(o), 4 + int(b)).tobytes()
                          for o, b in zip(out["rec_off"], out["block_size"])]
        return out

    def decode_split_device(self, data, v_start, v_end, n_ref, comp_base=0, file_len=None):
        """Device-resident decode (bench path): returns the hbam_columns struct."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = comp_base + n
        d = Columns()
        rc = self.L.hbam_decode_split(self.h, p, dev, comp_base, n, file_len, v_start, v_end,
                                      n_ref, C.byref(d))
        return rc, d

    def guess_batch(self, data, beg, end, n_ref):
        p, n, dev, keep = self._ptr(data)
        beg = np.ascontiguousarray(beg, np.int64)
        end = np.ascontiguousarray(end, np.int64)
        k = len(beg)
        out = np.zeros(max(k, 1), np.int64)
        err = np.zeros(max(k, 1), np.int32)
        rc = self.L.hbam_guess_batch(self.h, p, dev, n, beg.ctypes.data, end.ctypes.data, k,
                                     n_ref, out.ctypes.data, err.ctypes.data)
        return rc, out[:k], err[:k]

    def guess_window_len(self, file_len, beg, end):
        return int(self.L.hbam_guess_window_len(int(file_len), int(beg), int(end)))

    def guess_bgzf_window_len(self, file_len, beg, end):
        return int(self.L.hbam_guess_bgzf_window_len(int(file_len), int(beg), int(end)))

    def guess_windows(self, windows, win_off, file_len, beg, end, n_ref):
        """hbam_guess_windows: windows = the k guess windows concatenated (win_off: k+1)."""
        p, n, dev, keep = self._ptr(windows)
        beg = np.ascontiguousarray(beg, np.int64)
        end = np.ascontiguousarray(end, np.int64)
        win_off = np.ascontiguousarray(win_off, np.uint64)
        k = len(beg)
        out = np.zeros(max(k, 1), np.int64)
        err = np.zeros(max(k, 1), np.int32)
        rc = self.L.hbam_guess_windows(self.h, p, dev, win_off.ctypes.data, int(file_len), beg.ctypes.data,
                                       end.ctypes.data, k, n_ref, out.ctypes.data, err.ctypes.data)
        return rc, out[:k], err[:k]

    def guess_bgzf_window(self, window, file_len, beg, end):
        p, n, dev, keep = self._ptr(window)
        e = C.c_int32(0)
        r = self.L.hbam_guess_bgzf_window(self.h, p, dev, n, int(file_len), int(beg), int(end), C.byref(e))
        return r, e.value

    def probabilistic_splits_windows(self, head, windows, win_off, file_len, beg, end):
        hp, hn, hdev, hkeep = self._ptr(head)
        if hdev:
            raise ValueError("the header prefix is a host buffer")
        p, n, dev, keep = self._ptr(windows)
        beg = np.ascontiguousarray(beg, np.uint64)
        end = np.ascontiguousarray(end, np.uint64)
        win_off = np.ascontiguousarray(win_off, np.uint64)
        k = len(beg)
        vs = np.zeros(max(k, 1), np.uint64)
        ve = np.zeros(max(k, 1), np.uint64)
        r = self.L.hbam_probabilistic_splits_windows(self.h, hp, hn, p, dev, win_off.ctypes.data, int(file_len),
                                                     beg.ctypes.data, end.ctypes.data, k, vs.ctypes.data,
                                                     ve.ctypes.data)
        if r < 0:
            return r, None, None
        return r, vs[:r], ve[:r]

    def guess_bgzf_block_start(self, data, beg, end):
        p, n, dev, keep = self._ptr(data)
        e = C.c_int32(0)
        r = self.L.hbam_guess_bgzf_block_start(self.h, p, dev, n, beg, end, C.byref(e))
        return r, e.value

    def probabilistic_splits(self, data, beg, end):
        p, n, dev, keep = self._ptr(data)
        beg = np.ascontiguousarray(beg, np.uint64)
        end = np.ascontiguousarray(end, np.uint64)
        k = len(beg)
        vs = np.zeros(max(k, 1), np.uint64)
        ve = np.zeros(max(k, 1), np.uint64)
        r = self.L.hbam_probabilistic_splits(self.h, p, dev, n, beg.ctypes.data, end.ctypes.data,
                                             k, vs.ctypes.data, ve.ctypes.data)
        if r < 0:
            return r, None, None
        return r, vs[:r], ve[:r]

    def splitting_index(self, data, granularity=4096):
        """SplittingBAMIndexer over a whole BAM file on the device -> uint64 entries."""
        p, n, dev, keep = self._ptr(data)
        h = self.parse_header(data)
        if not isinstance(h, dict):
            return h, None
        d = Columns()
        rc = self.L.hbam_decode_split(self.h, p, dev, 0, n, n, h["first_voffset"],
                                      (n << 16) | 0xffff, h["n_ref"], C.byref(d))
        if rc:
            return rc, None
        cap = int(d.n_records) // granularity + 2
        out = np.zeros(cap, np.uint64)
        r = self.L.hbam_splitting_index(self.h, C.byref(d), granularity, n, out.ctypes.data, cap)
        if r < 0:
            return int(r), None
        return 0, out[:r]

    def bai_build(self, dcols, n_ref, end_voffset):
        """hbam_bai_build over the device columns of a whole-file decode -> (rc, .bai bytes or None,
        err_record): rc < 0 is the exception the indexer raises at record err_record."""
        cap = int(self.L.hbam_bai_bound(int(dcols.n_records), int(n_ref)))
        out = np.empty(cap, np.uint8)
        err = C.c_uint64(0)
        r = self.L.hbam_bai_build(self.h, C.byref(dcols), int(n_ref), int(end_voffset), out.ctypes.data, cap,
                                  C.byref(err))
        if r < 0:
            return int(r), None, int(err.value)
        return 0, out[:r].tobytes(), None

    def bai_index(self, data):
        """The Index plugin's work for one BAM held in host memory (bytes / numpy / memmap): header,
        whole-file device decode, hbam_bai_build -> (rc, .bai bytes or None, err_record)."""
        p, n, dev, keep = self._ptr(data)
        k = min(n, 1 << 20)
        while True:  # the header from a growing prefix (usually one or two BGZF blocks)
            h = self.parse_header(data[:k])
            if isinstance(h, dict) or k >= n:
                break
            k = min(n, 4 * k)
        if not isinstance(h, dict):
            return h, None, None
        ev = self.end_voffset(data, h["first_voffset"])
        d = Columns()
        rc = self.L.hbam_decode_split(self.h, p, dev, 0, n, n, h["first_voffset"], (n << 16) | 0xffff,
                                      h["n_ref"], C.byref(d))
        if rc:
            return rc, None, None
        return self.bai_build(d, h["n_ref"], ev)

    @staticmethod
    def end_voffset(data, first_voffset):
        """getFilePointer() after the last record a reader gets from a BAM whose first record is at
        first_voffset: the read ends at the first empty BGZF block after the first record's block
        (the 28-byte terminator, or an empty block in mid-file), else at the end of the file; the
        stream has then consumed the block before it and points at that block's start.  A host
        walk of the block headers (bgzf_blocks: host time the device timing of hbam_bai_build does
        not include; DESIGN.md gives one measurement).  The walk stops at a block the decode would
        not accept; the decode then raises and no index is built."""
        first = int(first_voffset) >> 16
        for coff, _, isize, _ in bgzf_blocks(data, first):
            if isize == 0 and coff > first:
                return coff << 16
        return len(data) << 16

    def overlap_filter(self, dcols, ref_id, beg=0, end=0, contained=False):
        """hbam_overlap_filter over device columns -> (count, device buffer handle of the kept record
        indices, ascending u32); the caller frees the handle with device_free."""
        n = int(dcols.n_records)
        buf = C.c_void_p()
        rc = self.L.hbam_device_alloc(self.h, 4 * max(n, 1), C.byref(buf))
        if rc:
            raise RuntimeError("hbam_device_alloc failed (%d): %s" % (rc, self.last_error()))
        k = self.L.hbam_overlap_filter(self.h, C.byref(dcols), int(ref_id), int(beg), int(end),
                                       int(bool(contained)), buf)
        if k < 0:
            self.L.hbam_device_free(self.h, buf)
            raise RuntimeError("hbam_overlap_filter failed (%d): %s" % (k, self.last_error()))
        return int(k), buf

    def gather_to_host(self, dcols, idx, k):
        """Host copy of records idx[0..k) (device u32 indices, e.g. overlap_filter's) of device
        columns: (voffset u64[k], payload u8 = the records' block_size + bytes packed in that
        order, offsets u64[k+1]).  Only the k records cross to the host (hbam_gather_records,
        hbam_permute, hbam_download)."""
        if k == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(1, np.uint64)
        vp = C.c_void_p
        bufs = []

        def alloc(nbytes):
            b = vp()
            rc = self.L.hbam_device_alloc(self.h, int(nbytes), C.byref(b))
            if rc:
                raise RuntimeError("hbam_device_alloc failed (%d): %s" % (rc, self.last_error()))
            bufs.append(b)
            return b
        try:
            ubuf, rec_off = C.cast(dcols.ubuf, vp), C.cast(dcols.rec_off, vp)
            bs, vo = C.cast(dcols.block_size, vp), C.cast(dcols.voffset, vp)
            off = alloc(8 * (k + 1))
            tot = C.c_uint64(0)
            rc = self.L.hbam_gather_records(self.h, ubuf, rec_off, bs, idx, k, None, 0, off, C.byref(tot))
            if not rc:
                pay = alloc(max(int(tot.value), 1))
                rc = self.L.hbam_gather_records(self.h, ubuf, rec_off, bs, idx, k, pay, tot.value, off,
                                                C.byref(tot))
            if not rc:
                dvo = alloc(8 * k)
                rc = self.L.hbam_permute(self.h, vo, 8, idx, k, dvo)
            if rc:
                raise RuntimeError("gathering %d records failed (%d): %s" % (k, rc, self.last_error()))
            return (self._d2h(dvo.value, k, np.uint64), self._d2h(pay.value, int(tot.value), np.uint8),
                    self._d2h(off.value, k + 1, np.uint64))
        finally:
            for b in bufs:
                self.L.hbam_device_free(self.h, b)

    def overlap_indices(self, dcols, ref_id, beg=0, end=0, contained=False):
        """hbam_overlap_filter -> the kept record indices on the host (uint32, ascending)."""
        k, buf = self.overlap_filter(dcols, ref_id, beg, end, contained)
        try:
            return self._d2h(buf.value, k, np.uint32)
        finally:
            self.L.hbam_device_free(self.h, buf)

    def resolve_tokens(self, tokens, bitmap, tail_token=0, tail_dist=0):
        """Diagnostic: run the LZ77 pass on one token block -> (rc, status, resolved bytes)."""
        io = np.ascontiguousarray(np.frombuffer(bytes(tokens), np.uint8)).copy()
        bm = np.ascontiguousarray(bitmap, np.uint32)
        st = C.c_int32(0)
        rc = self.L.hbam_resolve_tokens(self.h, io.ctypes.data, len(io), bm.ctypes.data,
                                        tail_token, tail_dist, C.byref(st))
        return rc, st.value, io.tobytes()

    def bgzf_block_index(self, data, granularity=1):
        """BGZFBlockIndexer.index (util/BGZFBlockIndexer.java:97-181) on the device ->
        (rc, uint64 entries)."""
        p, n, dev, keep = self._ptr(data)
        cap = n // 28 // max(int(granularity), 1) + 2  # a BGZF block is at least 28 bytes
        out = np.zeros(cap, np.uint64)
        r = self.L.hbam_bgzf_block_index(self.h, p, dev, n, int(granularity), out.ctypes.data, cap)
        if r < 0:
            return int(r), None
        return 0, out[:r]

    @staticmethod
    def _devptr(x):
        """A device pointer given as an int, None, a ctypes pointer or a torch tensor -> c_void_p."""
        if hasattr(x, "data_ptr"):
            import torch
            torch.cuda.current_stream(x.device).synchronize()
            return C.c_void_p(x.data_ptr())
        return C.c_void_p(x) if isinstance(x, (int, type(None))) else C.cast(x, C.c_void_p)

    def _text_result(self, rc, t):
        """A render's (rc, SamTextC) -> the dict of sam_render and vcf_render."""
        if rc:
            return {"rc": rc, "error": self.last_error()}
        k = int(t.n_records)
        return {"rc": 0, "n": k, "status": int(t.status), "err_record": int(t.err_record),
                "text": self._d2h(t.text, int(t.text_len), np.uint8).tobytes(),
                "line_off": self._d2h(t.line_off, k + 1, np.uint64),
                "deferred": self._d2h(t.deferred, int(t.n_deferred), np.uint32), "timing": self.timing()}

    # ---- read-name / CIGAR keyed consumers --------------------------------
    def _d2h(self, ptr, n, dtype):
        """Copy n elements of a device array (context-owned) to a numpy array."""
        out = np.empty(n, dtype)
        if n:
            rc = self.L.hbam_download(self.h, C.c_void_p(ptr), out.nbytes, C.c_void_p(out.ctypes.data))
            if rc:
                raise RuntimeError("hbam_download failed (%d): %s" % (rc, self.last_error()))
        return out

    def summarize_ranges(self, dcols):
        """SummarizeRecordReader's ranges over device columns (hbam_summarize_ranges) -> dict of
        numpy arrays + status."""
        r = RangesC()
        rc = self.L.hbam_summarize_ranges(self.h, C.byref(dcols), C.byref(r))
        if rc:
            raise RuntimeError("hbam_summarize_ranges failed (%d): %s" % (rc, self.last_error()))
        n = int(r.n)
        return dict(key=self._d2h(r.key, n, np.int64), beg=self._d2h(r.beg, n, np.int32),
                    end=self._d2h(r.end, n, np.int32), rev=self._d2h(r.rev, n, np.uint8),
                    record=self._d2h(r.record, n, np.uint32), status=int(r.status))

    def name_order(self, ubuf_ptr, rec_off_ptr, n, perm_ptr):
        rc = self.L.hbam_name_order(self.h, C.c_void_p(ubuf_ptr), C.c_void_p(rec_off_ptr), n,
                                    C.c_void_p(perm_ptr))
        if rc:
            raise RuntimeError("hbam_name_order failed (%d): %s" % (rc, self.last_error()))

    def fixmate(self, ubuf_ptr, rec_off_ptr, n):
        """FixMateReducer over the name shuffle of n device records -> host dict(payload,
        offsets, src, mate, n_groups, status)."""
        r = FixmateRunC()
        rc = self.L.hbam_fixmate(self.h, C.c_void_p(ubuf_ptr), C.c_void_p(rec_off_ptr), n, C.byref(r))
        if rc:
            raise RuntimeError("hbam_fixmate failed (%d): %s" % (rc, self.last_error()))
        k = int(r.n)
        return dict(payload=self._d2h(r.payload, int(r.payload_bytes), np.uint8),
                    offsets=self._d2h(r.offsets, k + 1, np.uint64) if k else np.zeros(1, np.uint64),
                    src=self._d2h(r.src, k, np.uint32), mate=self._d2h(r.mate, k, np.uint32),
                    n_groups=int(r.n_groups), status=int(r.status))

    # ---- the summarize plugin's reduce side and SummarySort ------------------------------------
    def device_alloc(self, nbytes):
        """hbam_device_alloc -> DeviceBuffer (freed by free())."""
        b = C.c_void_p()
        rc = self.L.hbam_device_alloc(self.h, int(nbytes), C.byref(b))
        if rc:
            raise RuntimeError("hbam_device_alloc failed (%d): %s" % (rc, self.last_error()))
        return DeviceBuffer(self, b.value, nbytes, True)

    def device_copy(self, dst_ptr, src_ptr, nbytes):
        rc = self.L.hbam_device_copy(self.h, C.c_void_p(dst_ptr), C.c_void_p(src_ptr), int(nbytes))
        if rc:
            raise RuntimeError("hbam_device_copy failed (%d): %s" % (rc, self.last_error()))

    def summarize_reduce_device(self, key_ptr, beg_ptr, end_ptr, rev_ptr, n, levels, sort_output=False):
        """hbam_summarize_reduce over n device-resident ranges -> SummaryC (device memory owned by
        the context until the next call)."""
        lv = np.ascontiguousarray(levels, np.int32)
        s = SummaryC()
        rc = self.L.hbam_summarize_reduce(self.h, C.c_void_p(key_ptr), C.c_void_p(beg_ptr), C.c_void_p(end_ptr),
                                          C.c_void_p(rev_ptr), int(n), C.c_void_p(lv.ctypes.data), len(lv),
                                          int(bool(sort_output)), C.byref(s))
        if rc:
            raise RuntimeError("hbam_summarize_reduce failed (%d): %s" % (rc, self.last_error()))
        return s

    def summary_to_host(self, s):
        k, m = int(s.n_streams), int(s.n_lines)
        return dict(first=self._d2h(s.first, k + 1, np.uint64), rid=self._d2h(s.rid, m, np.int32),
                    beg=self._d2h(s.beg, m, np.int32), end=self._d2h(s.end, m, np.int32),
                    count=self._d2h(s.count, m, np.int32),
                    text=self._d2h(s.text, int(s.text_len), np.uint8).tobytes(),
                    text_off=self._d2h(s.text_off, k + 1, np.uint64), n_segments=int(s.n_segments))

    def summarize_reduce(self, key, beg, end, rev, levels, sort_output=False):
        """hbam_summarize_reduce over host arrays (uploaded) -> host dict(first, rid, beg, end,
        count, text, text_off, n_segments, timing)."""
        arrs = [np.ascontiguousarray(key, np.int64), np.ascontiguousarray(beg, np.int32),
                np.ascontiguousarray(end, np.int32), np.ascontiguousarray(rev, np.uint8)]
        n = len(arrs[0])
        bufs = [self.upload(a.view(np.uint8)) for a in arrs]
        try:
            s = self.summarize_reduce_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, levels,
                                             sort_output)
            t = self.timing()
            out = self.summary_to_host(s)
            out["timing"] = t
            return out
        finally:
            for b in bufs:
                b.free()

    def summary_keys_device(self, text):
        """hbam_summary_keys -> SummaryLinesC (device memory owned by the context); `text` must stay
        alive while the result is used when it is device-resident."""
        p, n, dev, keep = self._ptr(text)
        s = SummaryLinesC()
        rc = self.L.hbam_summary_keys(self.h, p, dev, n, C.byref(s))
        if rc:
            raise RuntimeError("hbam_summary_keys failed (%d): %s" % (rc, self.last_error()))
        return s

    def summary_gather_lines(self, lines, perm=None, n=None):
        """hbam_summary_gather_lines: lines perm[0..n) (a device pointer, or None for the identity),
        each followed by a newline -> a DeviceBuffer of the text (free() it)."""
        n = int(lines.n) if n is None else int(n)
        off = self.device_alloc(8 * (n + 1))
        try:
            tot = C.c_uint64(0)
            rc = self.L.hbam_summary_gather_lines(self.h, C.byref(lines), perm, n, None, 0, C.c_void_p(off.ptr),
                                                  C.byref(tot))
            if rc:
                raise RuntimeError("hbam_summary_gather_lines failed (%d): %s" % (rc, self.last_error()))
            out = self.device_alloc(max(int(tot.value), 1))
            out.nbytes = int(tot.value)
            rc = self.L.hbam_summary_gather_lines(self.h, C.byref(lines), perm, n, C.c_void_p(out.ptr), tot.value,
                                                  C.c_void_p(off.ptr), C.byref(tot))
            if rc:
                out.free()
                raise RuntimeError("hbam_summary_gather_lines failed (%d): %s" % (rc, self.last_error()))
            return out
        finally:
            off.free()

    def summary_keys(self, text, sort=False):
        """hbam_summary_keys over `text` -> host dict(n, status, start, len, key, lines): `lines`
        = the n lines gathered in file order, or (sort) in the stable order of their keys."""
        dtext = self.upload(text) if not isinstance(text, DeviceBuffer) else text
        try:
            s = self.summary_keys_device(dtext)
            n = int(s.n)
            out = dict(n=n, status=int(s.status), start=self._d2h(s.start, n, np.uint32),
                       len=self._d2h(s.len, n, np.uint32), key=self._d2h(s.key, n, np.int64))
            perm = None
            pbuf = None
            if sort and n:
                pbuf = self.device_alloc(4 * n)
                rc = self.L.hbam_sort_keys(self.h, C.c_void_p(s.key), n, None, C.c_void_p(pbuf.ptr))
                if rc:
                    raise RuntimeError("hbam_sort_keys failed (%d): %s" % (rc, self.last_error()))
                perm = C.c_void_p(pbuf.ptr)
            try:
                g = self.summary_gather_lines(s, perm, n)
                out["lines"] = self._d2h(g.ptr, g.nbytes, np.uint8).tobytes()
                g.free()
            finally:
                if pbuf is not None:
                    pbuf.free()
            return out
        finally:
            if dtext is not text:
                dtext.free()

    # ---- BCF over BGZF --------------------------------------------------------
    def bcf_parse_header(self, file_prefix):
        """BCF2Codec.readHeader over the file's first bytes -> dict, or an error code."""
        a = np.ascontiguousarray(np.frombuffer(bytes(file_prefix), np.uint8))
        h = BcfHeaderC()
        rc = self.L.hbam_bcf_parse_header(self.h, C.c_void_p(a.ctypes.data), a.size, C.byref(h))
        if rc:
            return rc
        return dict(n_contig=h.n_contig, n_sample=h.n_sample, n_dict=h.n_dict, bgzf=bool(h.bgzf),
                    header_len=h.header_len, first_voffset=h.first_voffset)

    @staticmethod
    def _bcf_hdr(h):
        c = BcfHeaderC()
        c.n_contig, c.n_sample, c.n_dict = h["n_contig"], h["n_sample"], h["n_dict"]
        c.bgzf = int(bool(h["bgzf"]))
        c.header_len = int(h["header_len"])
        c.first_voffset = int(h.get("first_voffset", 0))
        return c

    def guess_bcf_window_len(self, file_len, beg, end, bgzf):
        return int(self.L.hbam_guess_bcf_window_len(int(file_len), int(beg), int(end), int(bool(bgzf))))

    def guess_bcf_windows(self, windows, win_off, file_len, beg, end, h):
        """hbam_guess_bcf_windows: BCFSplitGuesser over the k windows -> (rc, out, err)."""
        p, n, dev, keep = self._ptr(windows)
        beg = np.ascontiguousarray(beg, np.int64)
        end = np.ascontiguousarray(end, np.int64)
        win_off = np.ascontiguousarray(win_off, np.uint64)
        k = len(beg)
        out = np.zeros(max(k, 1), np.int64)
        err = np.zeros(max(k, 1), np.int32)
        hc = self._bcf_hdr(h)
        rc = self.L.hbam_guess_bcf_windows(self.h, p, dev, win_off.ctypes.data, int(file_len), beg.ctypes.data,
                                           end.ctypes.data, k, C.byref(hc), out.ctypes.data, err.ctypes.data)
        return rc, out[:k], err[:k]

    def bcf_decode_split(self, data, h, start, end_or_len, comp_base=0, file_len=None, keep_data=False):
        """BCFRecordReader over one split (hbam_bcf_decode_split) -> host numpy columns."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = comp_base + n
        d = BcfColumnsC()
        hc = self._bcf_hdr(h)
        rc = self.L.hbam_bcf_decode_split(self.h, p, dev, int(comp_base), n, int(file_len), C.byref(hc),
                                          int(start), int(end_or_len), C.byref(d))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        k = int(d.n_records)
        out = {"rc": 0, "n": k, "status": int(d.status), "err_record": int(d.err_record)}
        for name, dt in BCF_FIELDS:
            out[name] = self._d2h(getattr(d, name), k, dt)
        if keep_data:
            out["data"] = self._d2h(d.data, int(d.data_len), np.uint8)
        out["timing"] = self.timing()
        return out

    # ---- text VCF (hbam_vcf.hip) ------------------------------------------------------------------
    @staticmethod
    def vcf_contig_table(contigs):
        """The contig dictionary as hbam_vcf_decode_split takes it: (VcfContigC array, size, names
        bytes).  `contigs` = the ##contig IDs in header order (bytes); a later duplicate overwrites
        the earlier one's ordinal.  Open addressing, linear probing, FNV-1a, a power of two of at
        least twice the distinct IDs."""
        d = {}
        for i, name in enumerate(contigs):
            d[bytes(name)] = i
        size = 2
        while size < 2 * len(d):
            size *= 2
        tab = (VcfContigC * size)()
        for e in tab:
            e.ordinal = -1
        names = bytearray()
        for name, ordinal in d.items():
            h = 2166136261
            for b in name:
                h = ((h ^ b) * 16777619) & 0xffffffff
            h &= size - 1
            while tab[h].ordinal >= 0:
                h = (h + 1) & (size - 1)
            tab[h].name_off, tab[h].name_len, tab[h].ordinal = len(names), len(name), ordinal
            names += name
        return tab, size, bytes(names)

    def vcf_decode_split_device(self, data, start, length, data_start, table, text_base=0, file_len=None,
                                keep_text=False):
        """hbam_vcf_decode_split -> (rc, device VcfColumnsC); `table` = vcf_contig_table(...)."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = text_base + n
        tab, size, names = table
        nm = np.frombuffer(names, np.uint8) if names else np.zeros(1, np.uint8)
        d = VcfColumnsC()
        rc = self.L.hbam_vcf_decode_split(self.h, p, dev, int(text_base), n, int(file_len), int(start), int(length),
                                          int(data_start), C.cast(tab, C.c_void_p), size,
                                          C.c_void_p(nm.ctypes.data), len(names), int(bool(keep_text)), C.byref(d))
        return rc, d

    def vcf_decode_split(self, data, start, length, data_start, table, text_base=0, file_len=None):
        """VCFRecordReader over one split (hbam_vcf_decode_split + hbam_vcf_columns_to_host) -> host
        numpy columns."""
        rc, d = self.vcf_decode_split_device(data, start, length, data_start, table, text_base, file_len)
        if rc:
            return {"rc": rc, "error": self.last_error()}
        h = VcfColumnsC()
        rc = self.L.hbam_vcf_columns_to_host(self.h, C.byref(d), C.byref(h))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        k = int(h.n)
        out = {"rc": 0, "n": k, "status": int(h.status)}
        for name, dt in VCF_FIELDS:
            out[name] = _host_array(getattr(h, name), k, dt)
        out["tab"] = _host_array(h.tab, 8 * k, np.uint32).reshape(k, 8)
        self.L.hbam_vcf_release(self.h, C.byref(h))
        out["timing"] = self.timing()
        return out

    # ---- FASTQ / QSEQ (hbam_fastq.hip) ------------------------------------------------------------
    def frag_decode_split_device(self, fmt, data, start, length, encoding=HBAM_QUAL_SANGER, filter_failed_qc=False,
                                 text_base=0, file_len=None):
        """hbam_fastq_decode_split (fmt "fastq") / hbam_qseq_decode_split ("qseq") -> (rc, device
        FragColumnsC).  length None = the reference's unbounded end (a compressed file)."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = text_base + n
        fn = {"fastq": self.L.hbam_fastq_decode_split, "qseq": self.L.hbam_qseq_decode_split}[fmt]
        d = FragColumnsC()
        rc = fn(self.h, p, dev, int(text_base), n, int(file_len), int(start),
                0xffffffffffffffff if length is None else int(length), int(encoding), int(bool(filter_failed_qc)),
                C.byref(d))
        return rc, d

    def frag_decode_split(self, fmt, data, start, length, encoding=HBAM_QUAL_SANGER, filter_failed_qc=False,
                          text_base=0, file_len=None):
        """FastqRecordReader / QseqRecordReader over one split -> host numpy columns: n, status, err_pos,
        first_pos, end_pos, FRAG_FIELDS, instrument / flowcell / index as (n, 2) offset-length pairs
        into the window, and the pools key / seq / qual with their n + 1 offsets."""
        rc, d = self.frag_decode_split_device(fmt, data, start, length, encoding, filter_failed_qc, text_base,
                                              file_len)
        if rc:
            return {"rc": rc, "error": self.last_error()}
        h = FragColumnsC()
        rc = self.L.hbam_frag_columns_to_host(self.h, C.byref(d), C.byref(h))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        k = int(h.n)
        out = {"rc": 0, "n": k, "status": int(h.status), "err_pos": int(h.err_pos), "first_pos": int(h.first_pos),
               "end_pos": int(h.end_pos)}
        for name, dt in FRAG_FIELDS:
            out[name] = _host_array(getattr(h, name), k, dt)
        for name in ("instrument", "flowcell", "index"):
            out[name] = _host_array(getattr(h, name), 2 * k, np.uint32).reshape(k, 2)
        for name in ("key", "seq", "qual"):
            out[name + "_off"] = _host_array(getattr(h, name + "_off"), k + 1, np.uint64)
            out[name] = _host_array(getattr(h, name), int(getattr(h, name + "_len")), np.uint8)
        self.L.hbam_frag_release(self.h, C.byref(h))
        out["timing"] = self.timing()
        return out

    # ---- FASTA (hbam_fasta.hip) --------------------------------------------------------------------
    def fasta_sections(self, data, text_base=0):
        """hbam_fasta_sections over one window -> {"rc", "offsets"}: the file offsets of every '>'
        (uint64, ascending).  The size query and the call that fills the array."""
        p, n, dev, keep = self._ptr(data)
        cnt = C.c_uint64(0)
        rc = self.L.hbam_fasta_sections(self.h, p, dev, int(text_base), n, None, 0, C.byref(cnt))
        if rc not in (HBAM_OK, HBAM_EMORE):
            return {"rc": rc, "error": self.last_error()}
        out = np.zeros(int(cnt.value), np.uint64)
        if rc == HBAM_EMORE:
            rc = self.L.hbam_fasta_sections(self.h, p, dev, int(text_base), n, C.c_void_p(out.ctypes.data), len(out),
                                            C.byref(cnt))
            if rc:
                return {"rc": rc, "error": self.last_error()}
        return {"rc": 0, "offsets": out, "timing": self.timing()}

    def fasta_decode_split_device(self, data, start, length, text_base=0, file_len=None):
        """hbam_fasta_decode_split -> (rc, device FastaColumnsC)."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = text_base + n
        d = FastaColumnsC()
        rc = self.L.hbam_fasta_decode_split(self.h, p, dev, int(text_base), n, int(file_len), int(start), int(length),
                                            C.byref(d))
        return rc, d

    def fasta_decode_split(self, data, start, length, text_base=0, file_len=None):
        """FastaRecordReader over one split -> host numpy columns: n, status, err_pos, first_pos,
        end_pos, FASTA_FIELDS, index_off / index_len (the indexSequence inside the window) and the
        pools key / seq with their n + 1 offsets."""
        rc, d = self.fasta_decode_split_device(data, start, length, text_base, file_len)
        if rc:
            return {"rc": rc, "error": self.last_error()}
        h = FastaColumnsC()
        rc = self.L.hbam_fasta_columns_to_host(self.h, C.byref(d), C.byref(h))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        k = int(h.n)
        out = {"rc": 0, "n": k, "status": int(h.status), "err_pos": int(h.err_pos), "first_pos": int(h.first_pos),
               "end_pos": int(h.end_pos), "index_off": int(h.index_off), "index_len": int(h.index_len)}
        for name, dt in FASTA_FIELDS:
            out[name] = _host_array(getattr(h, name), k, dt)
        for name in ("key", "seq"):
            out[name + "_off"] = _host_array(getattr(h, name + "_off"), k + 1, np.uint64)
            out[name] = _host_array(getattr(h, name), int(getattr(h, name + "_len")), np.uint8)
        self.L.hbam_fasta_release(self.h, C.byref(h))
        out["timing"] = self.timing()
        return out

    # ---- FASTQ / QSEQ output (hbam_fragtext.hip) ---------------------------------------------------
    @staticmethod
    def _frag_host_columns(cols):
        """Host columns (frag_decode_split's dict form) as a FragColumnsC with host = 1 -> (struct,
        the arrays it points into)."""
        n = int(cols["n"])
        h, keep = FragColumnsC(), []
        h.n, h.host = n, 1

        def put(name, dt, count):
            a = np.ascontiguousarray(cols[name], dt).reshape(-1)
            if a.size != count:
                raise ValueError("column %s holds %d elements, not %d" % (name, a.size, count))
            keep.append(a)
            setattr(h, name, a.ctypes.data if a.size else None)
            return a
        put("present", np.uint32, n)
        for name in ("run", "lane", "tile", "xpos", "ypos", "read", "filter_passed", "control"):
            put(name, np.int32, n)
        for name in ("instrument", "flowcell", "index"):
            put(name, np.uint32, 2 * n)
        for name in ("key", "seq", "qual"):
            put(name + "_off", np.uint64, n + 1)
            a = np.ascontiguousarray(cols[name], np.uint8).reshape(-1)
            keep.append(a)
            setattr(h, name, a.ctypes.data if a.size else None)
            setattr(h, name + "_len", a.size)
        return h, keep

    def frag_render_device(self, cols, window, n=None, fmt=HBAM_FRAG_FASTQ, encoding=HBAM_QUAL_SANGER, flags=0,
                           perm=None):
        """hbam_frag_render -> (rc, device FragTextC).  cols: a device FragColumnsC (what
        frag_decode_split_device left on this context) or host columns as a dict of numpy arrays
        (frag_decode_split's form); window: the bytes the instrument / flowcell / index pairs point
        into (bytes / numpy / a torch tensor, host or device); perm: a device pointer (int, ctypes
        pointer or torch tensor) to n u32 record indices, device columns only."""
        keep = None
        if isinstance(cols, dict):
            cols, keep = self._frag_host_columns(cols)
        if n is None:
            n = int(cols.n)
        wp, wn, wdev, wkeep = self._ptr(window)
        t = FragTextC()
        rc = self.L.hbam_frag_render(self.h, C.byref(cols), wp, wdev, wn, self._devptr(perm), int(n), int(fmt),
                                     int(encoding), int(flags), C.byref(t))
        del keep, wkeep
        return rc, t

    def frag_render(self, cols, window, n=None, fmt=HBAM_FRAG_FASTQ, encoding=HBAM_QUAL_SANGER, flags=0, perm=None):
        """hbam_frag_render and a host copy of what it wrote -> dict: n, status, err_record, text
        (bytes: the complete records), partial (bytes: what the reference's stream already holds of
        the failing record), line_off (uint64[n + 1]), timing."""
        rc, t = self.frag_render_device(cols, window, n, fmt, encoding, flags, perm)
        if rc:
            return {"rc": rc, "error": self.last_error()}
        k, tl, pl = int(t.n_records), int(t.text_len), int(t.partial_len)
        both = self._d2h(t.text, tl + pl, np.uint8).tobytes()
        return {"rc": 0, "n": k, "status": int(t.status), "err_record": int(t.err_record), "text": both[:tl],
                "partial": both[tl:], "line_off": self._d2h(t.line_off, k + 1, np.uint64), "timing": self.timing()}

    # ---- SAM text (hbam_sam.hip) ------------------------------------------------------------------
    def sam_decode_split_device(self, data, start, length, data_start, table, n_ref, text_base=0, file_len=None):
        """hbam_sam_decode_split -> (rc, device Columns), as decode_split_device; `table` =
        vcf_contig_table(the @SQ SN names in header order)."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = text_base + n
        tab, size, names = table
        nm = np.frombuffer(names, np.uint8) if names else np.zeros(1, np.uint8)
        d = Columns()
        rc = self.L.hbam_sam_decode_split(self.h, p, dev, int(text_base), n, int(file_len), int(start), int(length),
                                          int(data_start), C.cast(tab, C.c_void_p), size,
                                          C.c_void_p(nm.ctypes.data), len(names), int(n_ref), C.byref(d))
        return rc, d

    def sam_decode_split(self, data, start, length, data_start, table, n_ref, text_base=0, file_len=None):
        """SAMRecordReader over one FileSplit of SAM text; returns host numpy columns, as decode_split
        (voffset = the plain file offset of each line)."""
        rc, d = self.sam_decode_split_device(data, start, length, data_start, table, n_ref, text_base, file_len)
        if rc:
            return {"rc": rc, "error": self.last_error()}
        h = Columns()
        rc = self.L.hbam_columns_to_host(self.h, C.byref(d), C.byref(h))
        if rc:
            return {"rc": rc, "error": self.last_error()}
        out = host_columns_to_numpy(h)
        self.L.hbam_free_host_columns(C.byref(h))
        out["rc"] = 0
        out["timing"] = self.timing()
        return out

    # ---- SAM text output (hbam_samtext.hip) --------------------------------------------------------
    def sam_render_device(self, ubuf, rec_off, n, names, perm=None, on_device=True):
        """hbam_sam_render -> (rc, device SamTextC).  on_device: ubuf / rec_off / perm are device
        pointers (ints or ctypes pointers: a decode's columns, a sorted run, hbam_overlap_filter's
        list); else ubuf is host bytes and rec_off a host uint64 array of n + 1 offsets.  names = the
        dictionary names (bytes) in order."""
        names = [bytes(x) for x in names]
        noff = np.zeros(len(names) + 1, np.uint32)
        noff[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        nm = np.frombuffer(b"".join(names) or b"\0", np.uint8)
        t = SamTextC()
        vp = C.c_void_p
        if on_device:
            args = [self._devptr(x) for x in (ubuf, rec_off, perm)]
            keep = None
        else:
            if perm is not None:
                raise ValueError("perm needs device arguments")
            ro = np.ascontiguousarray(rec_off, np.uint64)
            if len(ro) != n + 1:
                raise ValueError("rec_off must hold n + 1 offsets")
            ub = np.frombuffer(bytes(ubuf), np.uint8) if not isinstance(ubuf, np.ndarray) else np.ascontiguousarray(ubuf)
            if n and int(ro[n]) > ub.size:
                raise ValueError("rec_off runs past the record bytes")
            keep = (ro, ub)
            args = [vp(ub.ctypes.data if ub.size else 0), vp(ro.ctypes.data), vp(None)]
        rc = self.L.hbam_sam_render(self.h, args[0], args[1], args[2], int(n), int(bool(on_device)),
                                    vp(nm.ctypes.data), vp(noff.ctypes.data), len(names), C.byref(t))
        del keep
        return rc, t

    def sam_render(self, ubuf, rec_off, n, names, perm=None, on_device=True):
        """hbam_sam_render and a host copy of what it wrote -> dict: n, status, err_record, text
        (bytes; a deferred line is empty), line_off (uint64[n + 1]), deferred (uint32, ascending
        output positions), timing."""
        return self._text_result(*self.sam_render_device(ubuf, rec_off, n, names, perm, on_device))

    # ---- VCF text output (hbam_vcftext.hip) --------------------------------------------------------
    def bcf_header_text(self, file_prefix):
        """hbam_bcf_header_text: the VCF header text of a BCF file (BGZF or plain) from its first bytes
        -> bytes, or an error code (HBAM_EMORE: the header runs past the prefix)."""
        a = np.ascontiguousarray(np.frombuffer(bytes(file_prefix), np.uint8))
        n = C.c_uint64(0)
        rc = self.L.hbam_bcf_header_text(self.h, C.c_void_p(a.ctypes.data), a.size, None, 0, C.byref(n))
        if rc:
            return rc
        out = np.zeros(max(int(n.value), 1), np.uint8)
        rc = self.L.hbam_bcf_header_text(self.h, C.c_void_p(a.ctypes.data), a.size, C.c_void_p(out.ctypes.data),
                                         int(n.value), C.byref(n))
        if rc:
            return rc
        return out[:int(n.value)].tobytes()

    def bcf_decode_split_device(self, data, h, start, end_or_len, comp_base=0, file_len=None):
        """hbam_bcf_decode_split -> (rc, device BcfColumnsC): nothing is copied; the arrays are the
        context's until its next decode."""
        p, n, dev, keep = self._ptr(data)
        if file_len is None:
            file_len = comp_base + n
        d = BcfColumnsC()
        hc = self._bcf_hdr(h)
        rc = self.L.hbam_bcf_decode_split(self.h, p, dev, int(comp_base), n, int(file_len), C.byref(hc),
                                          int(start), int(end_or_len), C.byref(d))
        del keep
        return rc, d

    def vcf_render_device(self, data, data_len, rec_off, n, h, meta, perm=None, on_device=True):
        """hbam_vcf_render -> (rc, device SamTextC).  on_device: data / rec_off / perm are device
        pointers (a BCF decode's columns, hbam_sort_keys' permutation); else data is host bytes and
        rec_off a host uint64 array of n offsets.  h = the header counts (bcf_parse_header's dict),
        meta = the dict of host arrays VCFHeader.meta() builds."""
        vp = C.c_void_p
        m = VcfMetaC()
        keep = [np.ascontiguousarray(meta[k]) for k in ("contig_names", "contig_off", "dict_names", "dict_off",
                                                        "dict_rank", "dict_flags", "dict_number")]
        for (name, _), a in zip(VcfMetaC._fields_, keep):
            setattr(m, name, a.ctypes.data)
        hc = self._bcf_hdr(dict(h, bgzf=0, header_len=0))
        t = SamTextC()
        if on_device:
            args = [self._devptr(x) for x in (data, rec_off, perm)]
        else:
            if perm is not None:
                raise ValueError("perm needs device arguments")
            ro = np.ascontiguousarray(rec_off, np.uint64)
            if len(ro) < n:
                raise ValueError("rec_off must hold n offsets")
            ub = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
            data_len = ub.size
            keep += [ro, ub]
            args = [vp(ub.ctypes.data if ub.size else 0), vp(ro.ctypes.data), vp(None)]
        rc = self.L.hbam_vcf_render(self.h, args[0], int(data_len), args[1], args[2], int(n), int(bool(on_device)),
                                    C.byref(hc), C.byref(m), C.byref(t))
        del keep
        return rc, t

    def vcf_render(self, data, data_len, rec_off, n, h, meta, perm=None, on_device=True):
        """hbam_vcf_render and a host copy of what it wrote -> dict: n, status, err_record, text
        (bytes; a deferred line is empty), line_off (uint64[n + 1]), deferred (uint32, ascending
        output positions), timing."""
        return self._text_result(*self.vcf_render_device(data, data_len, rec_off, n, h, meta, perm, on_device))

    def vcf_gather_lines(self, dcols, perm=None, n=None):
        """hbam_vcf_gather_lines over the device columns of a keep_text decode: lines perm[0..n)
        (a device pointer, or None for the identity), each followed by a newline -> host bytes."""
        n = int(dcols.n) if n is None else int(n)
        if n == 0:
            return b""
        vp = C.c_void_p
        bufs = []

        def alloc(nbytes):
            b = vp()
            rc = self.L.hbam_device_alloc(self.h, int(nbytes), C.byref(b))
            if rc:
                raise RuntimeError("hbam_device_alloc failed (%d): %s" % (rc, self.last_error()))
            bufs.append(b)
            return b
        try:
            off = alloc(8 * (n + 1))
            tot = C.c_uint64(0)
            rc = self.L.hbam_vcf_gather_lines(self.h, C.byref(dcols), perm, n, None, 0, off, C.byref(tot))
            if not rc:
                pay = alloc(max(int(tot.value), 1))
                rc = self.L.hbam_vcf_gather_lines(self.h, C.byref(dcols), perm, n, pay, tot.value, off, C.byref(tot))
            if rc:
                raise RuntimeError("hbam_vcf_gather_lines failed (%d): %s" % (rc, self.last_error()))
            return self._d2h(pay.value, int(tot.value), np.uint8).tobytes()
        finally:
            for b in bufs:
                self.L.hbam_device_free(self.h, b)
