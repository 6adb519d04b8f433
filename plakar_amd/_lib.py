"""ctypes binding of libplakar_cdc.so (the C ABI declared in include/plakar_cdc.h).

The product path always goes through this library: there is no CPU chunker in
the package.  If the shared library is missing, import fails loudly with the
command that builds it.
"""
import ctypes
import numbers
import os
import sys
import warnings

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLAKAR_CDC_LIB selects an alternative build of the same library (kernel
# variants for A/B measurements, tools/ab.sh); default: the in-tree build.
LIB_PATH = os.environ.get("PLAKAR_CDC_LIB") or os.path.join(_HERE, "_lib", "libplakar_cdc.so")

CDC_OK = 0
CDC_EOF = 1
CDC_NEED_DATA = 2
CDC_E_INVALID = -1
CDC_E_UNSUPPORTED = -2
CDC_E_NOSPACE = -3
CDC_E_DEVICE = -4
CDC_E_NOMEM = -5
CDC_E_NORMAL_SIZE = -6
CDC_E_MIN_SIZE = -7
CDC_E_MAX_SIZE = -8
CDC_E_IO = -9
CDC_E_NOT_INIT = -10
CDC_E_NO_DEVICE = -11
CDC_E_AUTH = -12
CDC_E_CORRUPT = -13
CDC_E_MISMATCH = -14
CDC_E_NOTFOUND = -15

# the compression selector of cdc_encode_device, cdc_decode_device, cdc_check_device and the
# backup and restore options' `compress`
CDC_COMPRESS_NONE = 0
CDC_COMPRESS_LZ4 = 1
CDC_COMPRESS_GZIP = 2

# the compression level (compression.Configuration.Level, compression/compression.go:12-51): which
# match search Encode, the gzip stream, the zip pieces and the archive and backup sessions run
CDC_LEVEL_FAST = 0  # matches inside their 8-KiB segment
CDC_LEVEL_WIDE = 1  # matches from up to 32 KiB before the segment
_LEVEL_BEST = 9     # CDC_LEVEL_BEST: the same window, four candidates per bucket and a lazy parse: the smallest


def __getattr__(name):
    # CDC_LEVEL_BEST is an attribute of the module without being in dir(): 9 is no
    # status code, and a sweep over the module's CDC_* names (every status has a
    # cdc_strerror text) takes each name's value for one.
    if name == "CDC_LEVEL_BEST":
        return _LEVEL_BEST
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def level_code(level):
    """The C level for 0 / 1 / 9 (CDC_LEVEL_FAST / CDC_LEVEL_WIDE / CDC_LEVEL_BEST); ValueError otherwise."""
    if (isinstance(level, bool) or not isinstance(level, numbers.Integral)
            or level not in (CDC_LEVEL_FAST, CDC_LEVEL_WIDE, _LEVEL_BEST)):
        raise ValueError(f"unsupported level {level!r} (0: fast, 1: wide, 9: best)")
    return int(level)


def compress_code(compression):
    """The selector for a repository's compression name ("LZ4", "GZIP" or None)."""
    try:
        return {None: CDC_COMPRESS_NONE, "LZ4": CDC_COMPRESS_LZ4, "GZIP": CDC_COMPRESS_GZIP}[compression]
    except (KeyError, TypeError):
        raise ValueError(f"unsupported compression {compression!r} (LZ4 and GZIP are implemented)") from None


class cdc_opts(ctypes.Structure):
    _fields_ = [("min_size", ctypes.c_uint32), ("normal_size", ctypes.c_uint32),
                ("max_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class cdc_cut(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class cdc_buf(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class cdc_result(ctypes.Structure):
    _fields_ = [("ncuts", ctypes.c_uint64), ("consumed", ctypes.c_uint64),
                ("status", ctypes.c_int64), ("needed", ctypes.c_uint64)]


class cdc_backup_opts(ctypes.Structure):
    _fields_ = [("chunking", cdc_opts), ("packfile_max", ctypes.c_uint32), ("compress", ctypes.c_int),
                ("key", ctypes.c_void_p), ("packers", ctypes.c_int), ("readers", ctypes.c_int),
                ("batch_bytes", ctypes.c_uint64), ("known", ctypes.c_void_p), ("nknown", ctypes.c_uint64),
                ("timestamp", ctypes.c_int64)]


class cdc_backup_file(ctypes.Structure):
    _fields_ = [("index", ctypes.c_int), ("status", ctypes.c_int), ("checksum", ctypes.c_uint8 * 32),
                ("size", ctypes.c_uint64), ("nchunks", ctypes.c_uint64), ("cuts", ctypes.POINTER(cdc_cut)),
                ("digests", ctypes.POINTER(ctypes.c_uint8)), ("hists", ctypes.POINTER(ctypes.c_uint32)),
                ("is_new", ctypes.POINTER(ctypes.c_uint8)), ("entropy", ctypes.POINTER(ctypes.c_double)),
                ("object_entropy", ctypes.c_double), ("piece", ctypes.c_uint32), ("pieces", ctypes.c_uint32),
                ("data", ctypes.POINTER(ctypes.c_uint8)), ("data_offset", ctypes.c_uint64),
                ("data_len", ctypes.c_uint64)]


class cdc_backup_stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("files", "bytes", "chunks", "new_blobs", "new_bytes", "encoded_bytes",
                                               "packfiles", "packed_bytes", "batches")] + \
               [(n, ctypes.c_double) for n in ("read_s", "objhash_s", "h2d_s", "chunk_s", "digest_s", "d2h_s",
                                               "encode_s", "device_s", "callback_s", "read_wait_s", "pack_s", "wall_s")] + \
               [(n, ctypes.c_uint64) for n in ("failed_files", "pieces", "slot_arena_bytes")] + \
               [("hw_queues", ctypes.c_int32), ("streams_serialised", ctypes.c_int32)] + \
               [(n, ctypes.c_double) for n in ("fill_s", "drain_s", "chain_s")] + [("chain_bytes", ctypes.c_uint64)]


class cdc_packfile_footer(ctypes.Structure):
    _fields_ = [("version", ctypes.c_uint32), ("count", ctypes.c_uint32), ("timestamp", ctypes.c_int64),
                ("index_offset", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("index_checksum", ctypes.c_uint8 * 32)]


class cdc_packfile_row(ctypes.Structure):
    _fields_ = [("checksum", ctypes.c_uint8 * 32), ("offset", ctypes.c_uint32), ("length", ctypes.c_uint32),
                ("type", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3)]


# CDC_PACKFILE_* of the header, without the prefix (a module name that starts with CDC_ is a status code)
PACKFILE_PLAIN, PACKFILE_STORED, PACKFILE_ROWS = 0, 1, 2


def packfile_form_code(form):
    """The C form for "plain" / "stored" (the packfile forms a writer makes); ValueError otherwise."""
    try:
        return {"plain": PACKFILE_PLAIN, "stored": PACKFILE_STORED}[form]
    except (KeyError, TypeError):
        raise ValueError(f"unsupported packfile form {form!r} (\"plain\" or \"stored\")") from None


class cdc_packfile_src(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_void_p), ("len", ctypes.c_uint64), ("path", ctypes.c_char_p),
                ("form", ctypes.c_int), ("rows", ctypes.POINTER(cdc_packfile_row)), ("nrows", ctypes.c_uint64)]


# CDC_STATE_* of the header, without the prefix
STATE_PLAIN, STATE_STORED = 0, 1


def state_form_code(form):
    """The C form for "plain" / "stored" (a state's serialised bytes, or what PutState stores); ValueError otherwise."""
    try:
        return {"plain": STATE_PLAIN, "stored": STATE_STORED}[form]
    except (KeyError, TypeError):
        raise ValueError(f"unsupported state form {form!r} (\"plain\" or \"stored\")") from None


class cdc_state_src(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_void_p), ("len", ctypes.c_uint64), ("id", ctypes.c_uint8 * 32),
                ("form", ctypes.c_int)]


class cdc_state_row(ctypes.Structure):
    _fields_ = [("checksum", ctypes.c_uint8 * 32), ("packfile", ctypes.c_uint8 * 32), ("offset", ctypes.c_uint32),
                ("length", ctypes.c_uint32), ("type", ctypes.c_uint8), ("found", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 6)]


STATE_ROW_DTYPE_FIELDS = [("checksum", "V32"), ("packfile", "V32"), ("offset", "<u4"), ("length", "<u4"),
                          ("type", "u1"), ("found", "u1"), ("reserved", "V6")]


class cdc_state_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("states", ctypes.c_uint64),
                ("rejected", ctypes.c_uint64), ("rows", ctypes.c_uint64 * 9), ("deleted_snapshots", ctypes.c_uint64),
                ("capacity", ctypes.c_uint64), ("records", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64),
                ("decode_s", ctypes.c_double), ("index_s", ctypes.c_double), ("insert_s", ctypes.c_double)]


# CDC_SWEEP_* of the header, without the prefix
SWEEP_KEEP, SWEEP_DROP, SWEEP_REPACK = 0, 1, 2


class cdc_sweep_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("keep_types", ctypes.c_uint32), ("repack_permille", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class cdc_sweep_pack(ctypes.Structure):
    _fields_ = [("packfile", ctypes.c_uint8 * 32), ("extent", ctypes.c_uint64), ("live_bytes", ctypes.c_uint64),
                ("live_rows", ctypes.c_uint64), ("first_record", ctypes.c_uint64), ("row_first", ctypes.c_uint64),
                ("row_count", ctypes.c_uint64), ("verdict", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


SWEEP_PACK_DTYPE_FIELDS = [("packfile", "V32"), ("extent", "<u8"), ("live_bytes", "<u8"), ("live_rows", "<u8"),
                           ("first_record", "<u8"), ("row_first", "<u8"), ("row_count", "<u8"), ("verdict", "<i4"),
                           ("reserved", "<u4")]


class cdc_sweep_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] + \
               [(name, ctypes.c_uint64) for name in ("records", "live", "dead", "losers", "packs", "keep", "drop", "repack",
                                                     "kept_rows", "repack_rows", "live_bytes", "reclaimable_bytes")] + \
               [(name, ctypes.c_double) for name in ("packs_s", "sweep_s", "verdict_s", "compact_s", "download_s")]


class cdc_codec(ctypes.Structure):
    _fields_ = [("compress", ctypes.c_int), ("key", ctypes.c_char_p)]


class cdc_sync_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("src", cdc_codec), ("dst", cdc_codec), ("verify", ctypes.c_int),
                ("level", ctypes.c_int), ("packfile_max", ctypes.c_uint32), ("batch_bytes", ctypes.c_uint64),
                ("readers", ctypes.c_int), ("packers", ctypes.c_int), ("timestamp", ctypes.c_int64),
                ("known", ctypes.c_void_p), ("nknown", ctypes.c_uint64)]


class cdc_sync_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("path", ctypes.c_int32)] + \
               [(n, ctypes.c_uint64) for n in ("blobs", "skipped", "failed", "bytes_in", "bytes_out", "batches",
                                               "packfiles", "packed_bytes")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "transcode_s", "d2h_s", "pack_s", "callback_s",
                                               "device_wait_s", "wall_s")]


class cdc_restore_opts(ctypes.Structure):
    _fields_ = [("compress", ctypes.c_int), ("key", ctypes.c_void_p), ("verify", ctypes.c_int),
                ("writers", ctypes.c_int), ("batch_bytes", ctypes.c_uint64)]


class cdc_restore_file(ctypes.Structure):
    _fields_ = [("path", ctypes.c_char_p), ("nchunks", ctypes.c_uint64), ("checksums", ctypes.c_void_p),
                ("lengths", ctypes.c_void_p)]


class cdc_restore_result(ctypes.Structure):
    _fields_ = [("index", ctypes.c_int), ("status", ctypes.c_int), ("size", ctypes.c_uint64),
                ("piece", ctypes.c_uint32), ("pieces", ctypes.c_uint32), ("data", ctypes.POINTER(ctypes.c_uint8)),
                ("data_offset", ctypes.c_uint64), ("data_len", ctypes.c_uint64)]


class cdc_restore_stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("files", "failed_files", "bytes", "segments", "distinct_blobs",
                                               "decoded_blobs", "encoded_bytes", "decoded_bytes", "batches", "batches_identity",
                                               "pieces")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "d2h_s",
                                               "write_s", "wall_s")]


class cdc_read_range(ctypes.Structure):
    _fields_ = [("file", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("offset", ctypes.c_uint64),
                ("length", ctypes.c_uint64)]


class cdc_read_result(ctypes.Structure):
    _fields_ = [("index", ctypes.c_int), ("status", ctypes.c_int), ("piece", ctypes.c_uint32),
                ("pieces", ctypes.c_uint32), ("data", ctypes.POINTER(ctypes.c_uint8)),
                ("data_offset", ctypes.c_uint64), ("data_len", ctypes.c_uint64), ("length", ctypes.c_uint64)]


class cdc_read_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("ranges", "failed_ranges", "bytes", "segments", "batches",
                                               "distinct_blobs", "whole_blobs", "prefix_blobs", "verified_blobs",
                                               "encoded_bytes", "decoded_bytes", "skipped_bytes")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "d2h_s",
                                               "wall_s")]


class cdc_check_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("compress", ctypes.c_int), ("key", ctypes.c_void_p),
                ("fast", ctypes.c_int), ("threads", ctypes.c_int), ("batch_bytes", ctypes.c_uint64),
                ("host_min_len", ctypes.c_uint64)]


class cdc_check_file(ctypes.Structure):
    _fields_ = [("nchunks", ctypes.c_uint64), ("checksums", ctypes.c_void_p), ("lengths", ctypes.c_void_p),
                ("object_checksum", ctypes.c_void_p)]


class cdc_check_result(ctypes.Structure):
    _fields_ = [("index", ctypes.c_int), ("status", ctypes.c_int), ("bad_chunk", ctypes.c_int64),
                ("hashed", ctypes.c_int), ("checksum", ctypes.c_uint8 * 32), ("size", ctypes.c_uint64)]


class cdc_check_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("files", "failed_files", "bytes", "segments", "distinct_blobs",
                                               "decoded_blobs", "encoded_bytes", "decoded_bytes", "batches", "pieces",
                                               "device_objects", "device_bytes", "host_objects", "host_bytes",
                                               "seam_bytes")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "decode_s", "verify_s", "digest_s", "d2h_s", "hash_s",
                                               "wall_s")]


class cdc_line_rec(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("hash", ctypes.c_uint64 * 2)]


class cdc_diff_op(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("tag", "group", "i1", "i2", "j1", "j2")]


class cdc_emit_rec(ctypes.Structure):
    _fields_ = [("src_off", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("len", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class cdc_diff_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("compress", ctypes.c_int), ("key", ctypes.c_void_p),
                ("context", ctypes.c_int), ("threads", ctypes.c_int), ("batch_bytes", ctypes.c_uint64),
                ("max_lines", ctypes.c_uint64), ("hash_bits", ctypes.c_int)]


class cdc_diff_pair(ctypes.Structure):
    _fields_ = [("a", cdc_check_file), ("b", cdc_check_file), ("from_name", ctypes.c_char_p),
                ("to_name", ctypes.c_char_p)]


class cdc_diff_result(ctypes.Structure):
    _fields_ = [("index", ctypes.c_int), ("status", ctypes.c_int), ("bad_side", ctypes.c_int),
                ("identical", ctypes.c_int), ("bad_chunk", ctypes.c_int64), ("a_lines", ctypes.c_uint64),
                ("b_lines", ctypes.c_uint64), ("hunks", ctypes.c_uint64), ("text", ctypes.POINTER(ctypes.c_uint8)),
                ("text_len", ctypes.c_uint64)]


class cdc_diff_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("pairs", "failed_pairs", "identical_pairs", "skipped_pairs", "bytes",
                                               "segments", "distinct_blobs", "decoded_blobs", "encoded_bytes",
                                               "decoded_bytes", "batches", "lines", "distinct_lines", "verify_rounds",
                                               "hunks", "out_bytes")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "table_s",
                                               "ids_s", "match_s", "emit_s", "d2h_s", "wall_s")]


# CDC_DIFF_* and CDC_EMIT_* of the header, without the prefix: a module name that starts with CDC_ is a status code
DIFF_EQUAL, DIFF_REPLACE, DIFF_DELETE, DIFF_INSERT = 0, 1, 2, 3
EMIT_PREFIX, EMIT_LITERAL, EMIT_NEWLINE = 0x100, 0x200, 0x400
GREP_IGNORE_CASE = 1


class cdc_grep_hit(ctypes.Structure):
    _fields_ = [("text", ctypes.c_uint32), ("line", ctypes.c_uint32), ("off", ctypes.c_uint64),
                ("len", ctypes.c_uint32), ("col", ctypes.c_uint32), ("mask", ctypes.c_uint32),
                ("nocc", ctypes.c_uint32)]


class cdc_grep_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("compress", ctypes.c_int), ("key", ctypes.c_void_p),
                ("threads", ctypes.c_int), ("batch_bytes", ctypes.c_uint64), ("max_lines", ctypes.c_uint64)]


class cdc_grep_query(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("patterns", ctypes.c_void_p),
                ("pattern_len", ctypes.c_void_p), ("npatterns", ctypes.c_uint32), ("limit", ctypes.c_uint64),
                ("want_text", ctypes.c_int), ("max_line_bytes", ctypes.c_uint32)]


class cdc_grep_result(ctypes.Structure):
    _fields_ = [("index", ctypes.c_int), ("status", ctypes.c_int), ("bad_chunk", ctypes.c_int64),
                ("binary", ctypes.c_int), ("size", ctypes.c_uint64), ("lines", ctypes.c_uint64),
                ("matched", ctypes.c_uint64), ("hits", ctypes.POINTER(cdc_grep_hit)), ("nhits", ctypes.c_uint64),
                ("text", ctypes.POINTER(ctypes.c_uint8)), ("text_len", ctypes.c_uint64)]


class cdc_grep_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("files", "failed_files", "bytes", "segments", "distinct_blobs",
                                               "decoded_blobs", "encoded_bytes", "decoded_bytes", "batches", "lines",
                                               "matched_lines", "hits", "occurrences", "out_bytes")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "table_s",
                                               "scan_s", "compact_s", "emit_s", "d2h_s", "wall_s")]


class cdc_archive_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("compress", ctypes.c_int), ("key", ctypes.c_void_p),
                ("verify", ctypes.c_int), ("writers", ctypes.c_int), ("batch_bytes", ctypes.c_uint64),
                ("format", ctypes.c_int)]


class cdc_archive_entry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("type", ctypes.c_int), ("mode", ctypes.c_uint32),
                ("mtime", ctypes.c_int64), ("nchunks", ctypes.c_uint64), ("checksums", ctypes.c_void_p),
                ("lengths", ctypes.c_void_p)]


class cdc_archive_stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("failed_entry", ctypes.c_int32)] + \
               [(n, ctypes.c_uint64) for n in ("entries", "skipped_entries", "stream_bytes", "output_bytes", "segments",
                                               "decoded_blobs", "encoded_bytes", "decoded_bytes", "batches")] + \
               [(n, ctypes.c_double) for n in ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "deflate_s",
                                               "d2h_s", "write_s", "wall_s")]


class cdc_zip_piece(ctypes.Structure):
    _fields_ = [("src_off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("first", ctypes.c_uint32),
                ("last", ctypes.c_uint32), ("hdr_off", ctypes.c_uint32), ("hdr_len", ctypes.c_uint32),
                ("crc_reg", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("csize_before", ctypes.c_uint64),
                ("usize_before", ctypes.c_uint64)]


class cdc_zip_piece_out(ctypes.Structure):
    _fields_ = [("out_off", ctypes.c_uint64), ("out_len", ctypes.c_uint64), ("deflate_len", ctypes.c_uint64),
                ("crc_reg", ctypes.c_uint32), ("zip64", ctypes.c_uint32)]


CDC_ARCHIVE_TAR, CDC_ARCHIVE_TARGZ = 0, 1
CDC_ARCHIVE_FILE, CDC_ARCHIVE_DIR = 0, 1
ARCHIVE_DATA_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64)
ARCHIVE_ENTRY_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)
RESTORE_FILE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(cdc_restore_result))
READ_RANGE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(cdc_read_result))
CHECK_FILE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(cdc_check_result))
DIFF_PAIR_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(cdc_diff_result))
GREP_FILE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(cdc_grep_result))
BACKUP_FILE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(cdc_backup_file))
BACKUP_PACK_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64)
SYNC_BLOB_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint8, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int)

CUT_DTYPE_FIELDS = [("offset", "<u8"), ("length", "<u4"), ("reserved", "<u4")]
READ_FN = ctypes.CFUNCTYPE(ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)

_P = ctypes.POINTER
_u8p = _P(ctypes.c_uint8)

# name -> (restype, argtypes); every symbol here is declared in include/plakar_cdc.h
SIGNATURES = {
    "cdc_abi_version": (ctypes.c_int, []),
    "cdc_init": (ctypes.c_int, [ctypes.c_uint32, _P(ctypes.c_uint64), ctypes.c_uint64,
                                ctypes.c_uint64, ctypes.c_int]),
    "cdc_shutdown": (None, []),
    "cdc_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "cdc_device_count": (ctypes.c_int, []),
    "cdc_default_gear": (None, [_P(ctypes.c_uint64)]),
    "cdc_default_mask_s": (ctypes.c_uint64, []),
    "cdc_default_mask_l": (ctypes.c_uint64, []),
    "cdc_validate": (ctypes.c_int, [ctypes.c_char_p, _P(cdc_opts)]),
    "cdc_default_opts": (None, [_P(cdc_opts)]),
    "cdc_chunk": (ctypes.c_int, [_P(cdc_buf), ctypes.c_int, _P(cdc_opts), _P(cdc_cut),
                                 ctypes.c_uint64, _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "cdc_device_workspace_size": (ctypes.c_int, [ctypes.c_uint64, _P(cdc_opts),
                                                 _P(ctypes.c_uint64)]),
    "cdc_chunk_device_async": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.c_int, _P(cdc_opts), ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p]),
    "cdc_device_batch_workspace_size": (ctypes.c_int, [_P(ctypes.c_uint64), ctypes.c_int,
                                                       _P(cdc_opts), _P(ctypes.c_uint64)]),
    "cdc_chunk_device_batch_async": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_void_p),
                                                    _P(ctypes.c_uint64), ctypes.c_int,
                                                    ctypes.c_int, _P(cdc_opts),
                                                    _P(ctypes.c_void_p), _P(ctypes.c_uint64),
                                                    _P(ctypes.c_void_p), ctypes.c_void_p,
                                                    ctypes.c_uint64, ctypes.c_void_p]),
    "cdc_stream_new": (ctypes.c_int, [ctypes.c_char_p, _P(cdc_opts), ctypes.c_uint64,
                                      ctypes.c_int, _P(ctypes.c_void_p)]),
    "cdc_stream_buffer": (ctypes.c_int, [ctypes.c_void_p, _P(_u8p), _P(ctypes.c_uint64)]),
    "cdc_stream_commit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]),
    "cdc_stream_next": (ctypes.c_int, [ctypes.c_void_p, _P(_u8p), _P(ctypes.c_uint64)]),
    "cdc_stream_free": (None, [ctypes.c_void_p]),
    "cdc_chunker_new": (ctypes.c_int, [ctypes.c_char_p, READ_FN, ctypes.c_void_p, _P(cdc_opts),
                                       _P(ctypes.c_void_p)]),
    "cdc_chunker_next": (ctypes.c_int, [ctypes.c_void_p, _P(_u8p), _P(ctypes.c_uint64)]),
    "cdc_chunker_free": (None, [ctypes.c_void_p]),
    "cdc_chunk_digests_device_async": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                                      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "cdc_chunk_digests_device_batch_async": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_void_p),
                                                            _P(ctypes.c_uint64), ctypes.c_int,
                                                            _P(ctypes.c_void_p), _P(ctypes.c_uint64),
                                                            _P(ctypes.c_void_p), _P(ctypes.c_void_p),
                                                            _P(ctypes.c_void_p), ctypes.c_void_p]),
    "cdc_chunk_digests_hybrid": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_void_p), _P(ctypes.c_uint64), ctypes.c_int,
                                                _P(ctypes.c_void_p), _P(ctypes.c_uint64), _P(ctypes.c_void_p),
                                                _P(ctypes.c_void_p), _P(ctypes.c_void_p), ctypes.c_int,
                                                ctypes.c_uint64, ctypes.c_void_p, _P(ctypes.c_uint64),
                                                _P(ctypes.c_uint64)]),
    "cdc_batch_new": (ctypes.c_int, [ctypes.c_uint64, _P(ctypes.c_void_p)]),
    "cdc_batch_reserve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, _P(_P(ctypes.c_uint8))]),
    "cdc_batch_add_fd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]),
    "cdc_batch_add_files": (ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_char_p), ctypes.c_int, ctypes.c_int,
                                           _P(ctypes.c_uint64)]),
    "cdc_batch_count": (ctypes.c_int, [ctypes.c_void_p]),
    "cdc_batch_get": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _P(_P(ctypes.c_uint8)), _P(ctypes.c_uint64)]),
    "cdc_batch_chunk_files": (ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_char_p), ctypes.c_int, ctypes.c_int,
                                             _P(cdc_opts), _P(cdc_cut), ctypes.c_uint64, _P(ctypes.c_uint64),
                                             _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "cdc_batch_chunk": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_opts), _P(cdc_cut), ctypes.c_uint64,
                                       _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "cdc_batch_reset": (None, [ctypes.c_void_p]),
    "cdc_batch_free": (None, [ctypes.c_void_p]),
    "cdc_packer_new": (ctypes.c_int, [ctypes.c_uint32, _P(ctypes.c_void_p)]),
    "cdc_packer_add_blob": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, _P(ctypes.c_uint8), ctypes.c_void_p,
                                           ctypes.c_uint64]),
    "cdc_packer_add_chunks": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, _P(cdc_cut), ctypes.c_uint64,
                                               ctypes.c_void_p, ctypes.c_void_p]),
    "cdc_packer_size": (ctypes.c_uint64, [ctypes.c_void_p]),
    "cdc_packer_count": (ctypes.c_uint32, [ctypes.c_void_p]),
    "cdc_packer_serialize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64,
                                            _P(ctypes.c_uint64)]),
    "cdc_packer_serialize_part": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                 ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_packer_reset": (None, [ctypes.c_void_p]),
    "cdc_packer_free": (None, [ctypes.c_void_p]),
    "cdc_collector_new": (ctypes.c_int, [_P(cdc_opts), ctypes.c_uint64, ctypes.c_uint32, _P(ctypes.c_void_p)]),
    "cdc_collector_chunk": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _P(cdc_cut),
                                           ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_collector_stats": (ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "cdc_collector_free": (None, [ctypes.c_void_p]),
    "cdc_encode_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                         ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p,
                                         ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64), ctypes.c_void_p]),
    "cdc_encode_device_level": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                               ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p,
                                               ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64), ctypes.c_int,
                                               ctypes.c_void_p]),
    "cdc_encode_bound": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int]),
    "cdc_gzip_stream_new": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_void_p)]),
    "cdc_gzip_stream_bound": (ctypes.c_uint64, [ctypes.c_uint64]),
    "cdc_gzip_stream_piece": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64), ctypes.c_void_p]),
    "cdc_gzip_stream_free": (None, [ctypes.c_void_p]),
    "cdc_gzip_stream_set_level": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "cdc_zip_pieces_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, _P(cdc_zip_piece),
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_uint64, _P(cdc_zip_piece_out), _P(ctypes.c_uint64),
                                             ctypes.c_void_p]),
    "cdc_zip_pieces_device_level": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, _P(cdc_zip_piece),
                                                   ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.c_uint64, _P(cdc_zip_piece_out), _P(ctypes.c_uint64),
                                                   ctypes.c_int, ctypes.c_void_p]),
    "cdc_decode_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                         ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p,
                                         ctypes.c_uint64, _P(ctypes.c_uint64), _P(ctypes.c_int32), ctypes.c_void_p]),
    "cdc_decode_prefix_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64),
                                                _P(ctypes.c_uint64), _P(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_int,
                                                ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64),
                                                _P(ctypes.c_int32), ctypes.c_void_p]),
    "cdc_check_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                        ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p,
                                        ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64), _P(ctypes.c_int32),
                                        ctypes.c_void_p]),
    "cdc_transcode_size": (ctypes.c_int64, [ctypes.c_uint64, ctypes.c_int, ctypes.c_int]),
    "cdc_transcode_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                            ctypes.c_uint32, _P(cdc_codec), _P(cdc_codec), ctypes.c_char_p,
                                            ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64),
                                            _P(ctypes.c_int32), ctypes.c_void_p]),
    "cdc_transcode_device_level": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, _P(ctypes.c_uint64),
                                                  _P(ctypes.c_uint64), ctypes.c_uint32, _P(cdc_codec), _P(cdc_codec),
                                                  ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64,
                                                  _P(ctypes.c_uint64), _P(ctypes.c_int32), ctypes.c_int,
                                                  ctypes.c_void_p]),
    "cdc_packfile_index": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, _P(cdc_packfile_footer),
                                          _P(cdc_packfile_row), ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_packfile_index_stored": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                 ctypes.c_char_p, _P(cdc_packfile_footer), _P(cdc_packfile_row),
                                                 ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_packer_stored_bound": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "cdc_packer_serialize_stored": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64,
                                                   _P(ctypes.c_uint64)]),
    "cdc_assemble_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64),
                                           _P(ctypes.c_uint64), _P(ctypes.c_uint64), ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "cdc_debug_set_assemble_policy": (ctypes.c_int, [ctypes.c_int]),
    "cdc_restore_default_opts": (None, [_P(cdc_restore_opts)]),
    "cdc_restore_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_restore_opts), _P(ctypes.c_void_p)]),
    "cdc_restore_add_packfile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "cdc_restore_add_packfile_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "cdc_restore_add_packfiles": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_packfile_src), ctypes.c_uint32,
                                   _P(ctypes.c_int32)]),
    "cdc_restore_files": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_restore_file), ctypes.c_int, RESTORE_FILE_FN,
                                         ctypes.c_void_p, _P(cdc_restore_stats)]),
    "cdc_restore_ranges": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_restore_file), ctypes.c_int, _P(cdc_read_range),
                                          ctypes.c_int, READ_RANGE_FN, ctypes.c_void_p, _P(cdc_read_stats)]),
    "cdc_restore_free": (None, [ctypes.c_void_p]),
    "cdc_object_digests_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64),
                                                 _P(ctypes.c_uint64), ctypes.c_uint64, _P(ctypes.c_uint64),
                                                 ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "cdc_check_default_opts": (None, [_P(cdc_check_opts)]),
    "cdc_check_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_check_opts), _P(ctypes.c_void_p)]),
    "cdc_check_add_packfile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "cdc_check_add_packfile_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "cdc_check_add_packfiles": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_packfile_src), ctypes.c_uint32,
                                   _P(ctypes.c_int32)]),
    "cdc_check_files": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_check_file), ctypes.c_int, CHECK_FILE_FN,
                                       ctypes.c_void_p, _P(cdc_check_stats)]),
    "cdc_check_free": (None, [ctypes.c_void_p]),
    "cdc_line_table_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64),
                                             _P(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                             _P(ctypes.c_uint64), _P(ctypes.c_uint64), ctypes.c_void_p]),
    "cdc_line_ids_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.c_uint64, _P(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_int,
                                           _P(ctypes.c_uint32), _P(ctypes.c_uint32), ctypes.c_void_p]),
    "cdc_debug_set_line_threshold": (ctypes.c_int, [ctypes.c_uint32]),
    "cdc_diff_script": (ctypes.c_int, [_P(ctypes.c_uint32), ctypes.c_uint64, _P(ctypes.c_uint32), ctypes.c_uint64,
                                       ctypes.c_int, _P(cdc_diff_op), ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_diff_emit_plan": (ctypes.c_int, [_P(cdc_diff_op), ctypes.c_uint64, _P(cdc_line_rec), ctypes.c_uint64,
                                          _P(cdc_line_rec), ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p,
                                          ctypes.c_uint64, ctypes.c_uint64, _P(cdc_emit_rec), ctypes.c_uint64,
                                          ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64), _P(ctypes.c_uint64),
                                          _P(ctypes.c_uint64)]),
    "cdc_diff_emit_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_uint64, _P(cdc_emit_rec), ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p]),
    "cdc_diff_default_opts": (None, [_P(cdc_diff_opts)]),
    "cdc_diff_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_diff_opts), _P(ctypes.c_void_p)]),
    "cdc_diff_add_packfile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "cdc_diff_add_packfile_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "cdc_diff_add_packfiles": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_packfile_src), ctypes.c_uint32,
                                   _P(ctypes.c_int32)]),
    "cdc_diff_files": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_diff_pair), ctypes.c_int, DIFF_PAIR_FN,
                                      ctypes.c_void_p, _P(cdc_diff_stats)]),
    "cdc_diff_free": (None, [ctypes.c_void_p]),
    "cdc_grep_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64),
                                       _P(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p, _P(ctypes.c_uint32),
                                       ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p,
                                       ctypes.c_uint64, _P(ctypes.c_uint64), _P(ctypes.c_uint64), _u8p,
                                       _P(ctypes.c_uint64), ctypes.c_void_p]),
    "cdc_debug_set_grep_blocks": (ctypes.c_int, [ctypes.c_uint32]),
    "cdc_grep_default_opts": (None, [_P(cdc_grep_opts)]),
    "cdc_grep_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_grep_opts), _P(ctypes.c_void_p)]),
    "cdc_grep_add_packfile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "cdc_grep_add_packfile_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "cdc_grep_add_packfiles": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_packfile_src), ctypes.c_uint32,
                                   _P(ctypes.c_int32)]),
    "cdc_grep_files": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_grep_query), _P(cdc_check_file), ctypes.c_int,
                                      GREP_FILE_FN, ctypes.c_void_p, _P(cdc_grep_stats)]),
    "cdc_grep_free": (None, [ctypes.c_void_p]),
    "cdc_sync_default_opts": (None, [_P(cdc_sync_opts)]),
    "cdc_sync_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_sync_opts), _P(ctypes.c_void_p)]),
    "cdc_sync_add_packfile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "cdc_sync_add_packfile_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "cdc_sync_add_packfiles": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_packfile_src), ctypes.c_uint32,
                                   _P(ctypes.c_int32)]),
    "cdc_sync_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, BACKUP_PACK_FN, SYNC_BLOB_FN,
                                    ctypes.c_void_p, _P(cdc_sync_stats)]),
    "cdc_sync_free": (None, [ctypes.c_void_p]),
    "cdc_sync_set_packfile_form": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "cdc_archive_default_opts": (None, [_P(cdc_archive_opts)]),
    "cdc_archive_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_archive_opts), _P(ctypes.c_void_p)]),
    "cdc_archive_new_zip": (ctypes.c_int, [ctypes.c_int, _P(cdc_archive_opts), _P(ctypes.c_void_p)]),
    "cdc_archive_add_packfile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "cdc_archive_add_packfile_path": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "cdc_archive_add_packfiles": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_packfile_src), ctypes.c_uint32,
                                   _P(ctypes.c_int32)]),
    "cdc_archive_run": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_archive_entry), ctypes.c_int, ctypes.c_char_p,
                                       ARCHIVE_DATA_FN, ARCHIVE_ENTRY_FN, ctypes.c_void_p, _P(cdc_archive_stats)]),
    "cdc_archive_free": (None, [ctypes.c_void_p]),
    "cdc_archive_set_level": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "cdc_set_debug_mode": (ctypes.c_int, [ctypes.c_int]),
    "cdc_gear_is_placeholder": (ctypes.c_int, []),
    "cdc_set_maskl_index_mode": (ctypes.c_int, [ctypes.c_int]),
    "cdc_backup_run": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_char_p), ctypes.c_int, _P(cdc_backup_opts),
                                      BACKUP_FILE_FN, BACKUP_PACK_FN, ctypes.c_void_p, _P(cdc_backup_stats)]),
    "cdc_backup_run_level": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_char_p), ctypes.c_int, _P(cdc_backup_opts),
                                            BACKUP_FILE_FN, BACKUP_PACK_FN, ctypes.c_void_p, _P(cdc_backup_stats),
                                            ctypes.c_int]),
    "cdc_backup_new": (ctypes.c_int, [ctypes.c_int, _P(cdc_backup_opts), _P(ctypes.c_void_p)]),
    "cdc_backup_files": (ctypes.c_int, [ctypes.c_void_p, _P(ctypes.c_char_p), ctypes.c_int, BACKUP_FILE_FN,
                                        BACKUP_PACK_FN, ctypes.c_void_p, _P(cdc_backup_stats)]),
    "cdc_backup_free": (None, [ctypes.c_void_p]),
    "cdc_backup_set_level": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "cdc_backup_set_packfile_form": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "cdc_sha256": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, _P(ctypes.c_uint8)]),
    "cdc_sha256_accelerated": (ctypes.c_int, []),
    "cdc_chunk_entropy_device_async": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
    "cdc_debug_maskl_state": (ctypes.c_int, [ctypes.c_int, _P(ctypes.c_uint32), _P(ctypes.c_uint64)]),
    "cdc_debug_stream_read": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                             ctypes.c_double * 3, ctypes.c_double * 3, ctypes.c_void_p]),
    "cdc_debug_set_digest_lanes": (ctypes.c_int, [ctypes.c_uint64]),
    "cdc_debug_set_state_blocks": (ctypes.c_int, [ctypes.c_uint32]),
    "cdc_state_new": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, _P(ctypes.c_void_p)]),
    "cdc_state_free": (None, [ctypes.c_void_p]),
    "cdc_state_merge": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_state_src), ctypes.c_uint32, _P(ctypes.c_int32)]),
    "cdc_state_lookup": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_void_p]),
    "cdc_state_lookup_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.c_void_p, ctypes.c_void_p]),
    "cdc_state_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                      _P(ctypes.c_uint64)]),
    "cdc_state_extends": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_state_info": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_state_stats)]),
    "cdc_state_serialize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           _P(ctypes.c_uint64)]),
    "cdc_state_serialize_deleted": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_state_delete_snapshots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64,
                                                  _P(ctypes.c_int32)]),
    "cdc_state_mark": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                      _P(ctypes.c_uint64)]),
    "cdc_state_mark_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "cdc_state_clear_marks": (ctypes.c_int, [ctypes.c_void_p]),
    "cdc_sweep_default_opts": (None, [_P(cdc_sweep_opts)]),
    "cdc_state_sweep": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_sweep_opts), _P(ctypes.c_void_p)]),
    "cdc_sweep_packs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_sweep_kept_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_sweep_repack_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _P(ctypes.c_uint64)]),
    "cdc_sweep_info": (ctypes.c_int, [ctypes.c_void_p, _P(cdc_sweep_stats)]),
    "cdc_sweep_free": (None, [ctypes.c_void_p]),
    "cdc_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "cdc_profile_collect": (ctypes.c_int, [_P(ctypes.c_double), _P(ctypes.c_double),
                                           _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
}

_lib = None


def lib():
    """Load libplakar_cdc.so (once).  Raises if the HIP extension was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"libplakar_cdc.so not found at {LIB_PATH}: the HIP extension is required "
                "(build it with `python -m plakar_amd.build`); there is no CPU fallback")
        # With PyTorch in the process there are two HIP runtimes (torch's bundled
        # one and the system's, which this library links); torch's must come up
        # first, or torch then finds no device.  Only when torch is already
        # imported is its runtime brought up here: loading the library never
        # imports torch itself (the modules that use torch tensors -- device,
        # hashing, snapshot, encode -- import it before they load the library).
        torch = sys.modules.get("torch")
        if torch is not None:
            try:
                torch.cuda.is_available()
            except Exception:
                pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("PLAKAR_CDC_LIB") and not hasattr(L, name):
                continue  # an older variant build (A/B runs) may lack newer entry points
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class CdcError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().cdc_strerror(status).decode()
        super().__init__(f"{what}: {msg} ({status})" if what else f"{msg} ({status})")


def check(status, what=""):
    if status < 0:
        raise CdcError(status, what)
    return status


_init_key = None
_warned_placeholder = False


def ensure_init(gear=None, mask_s=0, mask_l=0, cut_convention=0, dev_mask=0):
    """cdc_init once per parameter set (the Gear table / masks are library-global,
    like the package-level G of ext chunkers/fastcdc).  Called with no
    arguments it initialises with the defaults only if the library is not
    initialised yet, and otherwise keeps the current parameters."""
    global _init_key
    explicit = (gear is not None or mask_s or mask_l or cut_convention or dev_mask)
    if not explicit and _init_key is not None:
        return
    key = (None if gear is None else tuple(int(x) for x in gear), int(mask_s), int(mask_l),
           int(cut_convention), int(dev_mask))
    if key == _init_key:
        return
    arr = None
    if gear is not None:
        if len(gear) != 256:
            raise ValueError("gear table must have 256 entries")
        arr = (ctypes.c_uint64 * 256)(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in gear])
    check(lib().cdc_init(dev_mask, arr, mask_s, mask_l, cut_convention), "cdc_init")
    _init_key = key
    global _warned_placeholder
    if gear is None and not _warned_placeholder:
        _warned_placeholder = True
        warnings.warn("plakar_amd: the built-in Gear table is a PLACEHOLDER (the go-cdc-chunkers v0.0.8 fastcdc.G "
                      "is not available here): cut points differ from plakar's; pass the real table as gear=",
                      stacklevel=2)


def default_gear():
    arr = (ctypes.c_uint64 * 256)()
    lib().cdc_default_gear(arr)
    return [int(x) for x in arr]
