"""Diff on the device: unified diffs of snapshot files.

The reference's `plakar diff` (cmd/plakar/subcommands/diff/diff.go:152-196)
reads both files whole, splits them with difflib.SplitLines, runs go-difflib's
UnifiedDiff with three lines of context and prints the text; equal object
checksums print "identical" without a read.  cdc_diff_files takes a batch of
pairs: every distinct blob of both sides is read, decoded and checked once,
the images are split into lines and the lines numbered on the device
(cdc_line_table_device, cdc_line_ids_device), the matcher (difflib's
SequenceMatcher over the ids, cdc_diff_script) runs on host threads, and the
text is put together on the device from an emit plan (cdc_diff_emit_device).
Every call goes through the C ABI."""
import ctypes
import os

import numpy as np

from . import _lib
from . import stored as _stored
from ._lib import check, ensure_init, lib

DEFAULT_BATCH_BYTES = 256 << 20
LINE_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("reserved", "<u4"), ("hash", "<u8", (2,))])
OP_DTYPE = np.dtype([(n, "<u4") for n in ("tag", "group", "i1", "i2", "j1", "j2")])
EMIT_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("len", "<u4"), ("flags", "<u4")])
TAGS = ("equal", "replace", "delete", "insert")
_p64 = ctypes.POINTER(ctypes.c_uint64)
_p32 = ctypes.POINTER(ctypes.c_uint32)


def _u64(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    return a, (a.ctypes.data_as(_p64) if a.size else None)


def _stream(t, stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(t.device.index)
    return ctypes.c_void_p(s.cuda_stream)


def line_table_device(src, texts, capacity=None, stream=None):
    """cdc_line_table_device over a torch uint8 tensor: `texts` is a list of
    (offset, length) in src.  Returns (records, counts): records a device
    tensor of n_lines x 32 bytes (view it with LINE_DTYPE on the host), counts
    the lines of each text.  capacity: room for that many records only
    (CdcError CDC_E_NOSPACE, with .needed, when it is too small); by default
    the call is made twice, the first time for the count."""
    import torch
    ensure_init()
    n = len(texts)
    t = np.asarray(texts, dtype=np.uint64).reshape(-1, 2)
    off, poff = _u64(t[:, 0])
    ln, pln = _u64(t[:, 1])
    counts = np.zeros(max(n, 1), dtype=np.uint64)
    total = ctypes.c_uint64(0)
    dev = src.device.index
    s = _stream(src, stream)

    def call(recs, cap):
        return lib().cdc_line_table_device(int(dev), ctypes.c_void_p(src.data_ptr()), src.numel(), poff, pln, n,
                                           ctypes.c_void_p(recs.data_ptr()) if recs is not None else None, cap,
                                           counts.ctypes.data_as(_p64), ctypes.byref(total), s)

    if capacity is None:
        rc = call(None, 0)
        if rc != _lib.CDC_E_NOSPACE:
            check(rc, "cdc_line_table_device")
        capacity = int(total.value)
    recs = torch.zeros((max(int(capacity), 1), 32), dtype=torch.uint8, device=src.device)
    rc = call(recs, int(capacity))
    if rc == _lib.CDC_E_NOSPACE:
        e = _lib.CdcError(rc, "cdc_line_table_device")
        e.needed = int(total.value)
        raise e
    check(rc, "cdc_line_table_device")
    return recs[:int(total.value)], counts[:n].copy()


def line_ids_device(src, records, groups, hash_bits=0, stream=None):
    """cdc_line_ids_device: `records` a host array of LINE_DTYPE over src,
    `groups` the ascending line numbers where each pair's lines start, ending
    with the number of lines.  Returns (ids, rounds): ids[i] the first line of
    i's group with i's bytes, counted from the group's start."""
    ensure_init()
    recs = np.ascontiguousarray(records, dtype=LINE_DTYPE)
    g, pg = _u64(groups)
    if g.size < 1:
        raise ValueError("groups needs at least its end entry")
    ids = np.zeros(max(recs.size, 1), dtype=np.uint32)
    rounds = ctypes.c_uint32(0)
    rc = lib().cdc_line_ids_device(int(src.device.index), ctypes.c_void_p(src.data_ptr()), src.numel(),
                                   ctypes.c_void_p(recs.ctypes.data), recs.size, pg, g.size - 1, int(hash_bits),
                                   ids.ctypes.data_as(_p32), ctypes.byref(rounds), _stream(src, stream))
    check(rc, "cdc_line_ids_device")
    return ids[:recs.size], int(rounds.value)


def diff_script(a_ids, b_ids, context=3):
    """cdc_diff_script: difflib.SequenceMatcher(None, a, b).get_grouped_opcodes(context)
    over 32-bit ids, as a list of groups of (tag, i1, i2, j1, j2).  Host only."""
    if context < 0:
        raise ValueError("context is not negative")
    ops = diff_ops(a_ids, b_ids, context)
    groups = []
    for o in ops:
        if int(o["group"]) == len(groups):
            groups.append([])
        groups[-1].append((TAGS[int(o["tag"])], int(o["i1"]), int(o["i2"]), int(o["j1"]), int(o["j2"])))
    return groups


def diff_ops(a_ids, b_ids, context=3):
    """cdc_diff_script's records (OP_DTYPE)."""
    a = np.ascontiguousarray(np.asarray(a_ids, dtype=np.uint32))
    b = np.ascontiguousarray(np.asarray(b_ids, dtype=np.uint32))
    pa = a.ctypes.data_as(_p32) if a.size else None
    pb = b.ctypes.data_as(_p32) if b.size else None
    need = ctypes.c_uint64(0)
    rc = lib().cdc_diff_script(pa, a.size, pb, b.size, int(context), None, 0, ctypes.byref(need))
    if rc != _lib.CDC_E_NOSPACE:
        check(rc, "cdc_diff_script")
    ops = np.zeros(max(int(need.value), 1), dtype=OP_DTYPE)
    rc = lib().cdc_diff_script(pa, a.size, pb, b.size, int(context),
                               ctypes.cast(ops.ctypes.data, ctypes.POINTER(_lib.cdc_diff_op)), int(need.value),
                               ctypes.byref(need))
    check(rc, "cdc_diff_script")
    return ops[:int(need.value)]


def diff_emit_plan(ops, a_lines, b_lines, from_name, to_name, dst_base=0, lit_base=0):
    """cdc_diff_emit_plan: the records (EMIT_DTYPE), the literal area (bytes)
    and the output size of one pair's unified diff.  Host only."""
    ops = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    al = np.ascontiguousarray(a_lines, dtype=LINE_DTYPE)
    bl = np.ascontiguousarray(b_lines, dtype=LINE_DTYPE)
    P = ctypes.POINTER
    args = [ctypes.cast(ops.ctypes.data, P(_lib.cdc_diff_op)), ops.size, ctypes.cast(al.ctypes.data, P(_lib.cdc_line_rec)),
            al.size, ctypes.cast(bl.ctypes.data, P(_lib.cdc_line_rec)), bl.size, os.fsencode(from_name),
            os.fsencode(to_name), int(dst_base), int(lit_base)]
    nrecs, nlit, nout = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    tail = [ctypes.byref(nrecs), ctypes.byref(nlit), ctypes.byref(nout)]
    rc = lib().cdc_diff_emit_plan(*args, None, 0, None, 0, *tail)
    if rc != _lib.CDC_E_NOSPACE:
        check(rc, "cdc_diff_emit_plan")
    recs = np.zeros(max(int(nrecs.value), 1), dtype=EMIT_DTYPE)
    lit = ctypes.create_string_buffer(max(int(nlit.value), 1))
    rc = lib().cdc_diff_emit_plan(*args, ctypes.cast(recs.ctypes.data, P(_lib.cdc_emit_rec)), int(nrecs.value),
                                  ctypes.cast(lit, ctypes.c_void_p), int(nlit.value), *tail)
    check(rc, "cdc_diff_emit_plan")
    return recs[:int(nrecs.value)], lit.raw[:int(nlit.value)], int(nout.value)


def diff_emit_device(plain, literal, records, dst, stream=None):
    """cdc_diff_emit_device: execute the records (EMIT_DTYPE, host) over the
    torch uint8 tensors plain and literal into dst.  Asynchronous on the
    current stream."""
    ensure_init()
    recs = np.ascontiguousarray(records, dtype=EMIT_DTYPE)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    size = lambda t: t.numel() if t is not None else 0  # noqa: E731
    rc = lib().cdc_diff_emit_device(int(dst.device.index), ptr(plain), size(plain), ptr(literal), size(literal),
                                    ctypes.cast(recs.ctypes.data, ctypes.POINTER(_lib.cdc_emit_rec)) if recs.size else None,
                                    recs.size, ptr(dst), size(dst), _stream(dst, stream))
    check(rc, "cdc_diff_emit_device")


def _file(f, obj, keep):
    chunks = obj.Chunks
    sums = b"".join(bytes(c.Checksum) for c in chunks)
    if len(sums) != 32 * len(chunks):
        raise ValueError("a chunk checksum is 32 bytes (SHA-256)")
    lens = np.array([int(c.Length) for c in chunks], dtype=np.uint32)
    sbuf = ctypes.create_string_buffer(sums, max(len(sums), 1))
    obuf = None
    osum = getattr(obj, "Checksum", None)
    if osum is not None:
        osum = bytes(osum)
        if len(osum) != 32:
            raise ValueError("an object checksum is 32 bytes (SHA-256)")
        obuf = ctypes.create_string_buffer(osum, 32)
    keep.append((sbuf, lens, obuf))
    f.nchunks = len(chunks)
    f.checksums = ctypes.cast(sbuf, ctypes.c_void_p)
    f.lengths = lens.ctypes.data if lens.size else None
    f.object_checksum = ctypes.cast(obuf, ctypes.c_void_p) if obuf is not None else None


class DiffSession:
    """A native diff context (cdc_diff_new): Decode's configuration
    (compression "LZ4", "GZIP" or None, the 32-byte key or None), the
    registered packfiles and their locator, with its stream and buffers kept
    across runs.  context: lines of context (3, as the reference).  hash_bits:
    diagnostic, only so many bits of the line hashes propose equal lines (0:
    all 128); the output never depends on it."""

    def __init__(self, key=None, compression="LZ4", context=3, threads=8, batch_bytes=DEFAULT_BATCH_BYTES, max_lines=0,
                 hash_bits=0, device=0):
        code = _lib.compress_code(compression)
        self._h = None
        self._keep = []
        keybuf = None
        if key is not None:
            key = bytes(key)
            if len(key) != 32:
                raise ValueError("the repository key is 32 bytes (AES-256)")
            keybuf = ctypes.create_string_buffer(key, 32)
        if int(context) < 1:
            raise ValueError("context is at least 1 (cdc_diff_script takes 0)")
        if not 0 <= int(hash_bits) <= 128:
            raise ValueError("hash_bits is 0..128")
        ensure_init()
        o = _lib.cdc_diff_opts()
        lib().cdc_diff_default_opts(ctypes.byref(o))
        o.compress = code
        o.key = ctypes.cast(keybuf, ctypes.c_void_p) if keybuf is not None else None
        o.context, o.threads, o.batch_bytes = int(context), int(threads), int(batch_bytes)
        o.max_lines, o.hash_bits = int(max_lines), int(hash_bits)
        h = ctypes.c_void_p()
        check(lib().cdc_diff_new(int(device), ctypes.byref(o), ctypes.byref(h)), "cdc_diff_new")
        self._h = h

    def add_packfile(self, packfile):
        """Register a packfile: bytes (kept alive by the session) or a path."""
        if not self._h:
            raise ValueError("session closed")
        if isinstance(packfile, (str, os.PathLike)):
            check(lib().cdc_diff_add_packfile_path(self._h, os.fsencode(packfile)), "cdc_diff_add_packfile_path")
            return
        buf = bytes(packfile)
        check(lib().cdc_diff_add_packfile(self._h, buf, len(buf)), "cdc_diff_add_packfile")
        self._keep.append(buf)

    def add_packfiles(self, packfiles, form="plain", rows=None):
        """Register many packfiles (bytes and/or paths) in one call
        (cdc_diff_add_packfiles): form "plain" or "stored", the form a repository
        keeps, whose footers and indexes are all decoded in two device calls;
        or rows, one list of (type, checksum, offset, length) per packfile
        (the repository state's), and nothing of a file's tail is read.
        Returns the per-source statuses: 0, or the CDC_E_* code of a source
        that was not entered."""
        if not self._h:
            raise ValueError("session closed")
        return _stored.add_packfiles("cdc_diff_add_packfiles", self._h, self._keep, packfiles, form, rows)

    def run(self, pairs):
        """Diff the pairs, each (object_a, object_b, from_name, to_name) with
        snapshot.Objects (Chunks' Checksum and Length, and Checksum or None).
        Returns (results, stats): results[i] a dict of status (0 or the pair's
        CDC_E_* code), bad_side, bad_chunk, identical, a_lines, b_lines, hunks
        and text (bytes: the unified diff, empty when identical); stats the
        fields of cdc_diff_stats."""
        if not self._h:
            raise ValueError("session closed")
        n = len(pairs)
        arr = (_lib.cdc_diff_pair * max(n, 1))()
        keep = []
        for i, (a, b, from_name, to_name) in enumerate(pairs):
            _file(arr[i].a, a, keep)
            _file(arr[i].b, b, keep)
            arr[i].from_name = os.fsencode(from_name)
            arr[i].to_name = os.fsencode(to_name)
        results = [None] * n
        errors = []

        def on_pair(_ctx, rp):
            try:
                r = rp.contents
                text = ctypes.string_at(r.text, int(r.text_len)) if r.text_len else b""
                results[int(r.index)] = dict(status=int(r.status), bad_side=int(r.bad_side), bad_chunk=int(r.bad_chunk),
                                             identical=bool(r.identical), a_lines=int(r.a_lines), b_lines=int(r.b_lines),
                                             hunks=int(r.hunks), text=text)
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)

        cb = _lib.DIFF_PAIR_FN(on_pair)
        st = _lib.cdc_diff_stats()
        st.struct_size = ctypes.sizeof(st)
        rc = lib().cdc_diff_files(self._h, arr, n, cb, None, ctypes.byref(st))
        check(rc, "cdc_diff_files")
        if errors:
            raise errors[0]
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_diff_stats._fields_
                 if name not in ("struct_size", "reserved")}
        return results, stats

    def close(self):
        if self._h:
            lib().cdc_diff_free(self._h)
            self._h = None
            self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def diff_files(pairs, packfiles, key=None, compression="LZ4", context=3, threads=8, batch_bytes=DEFAULT_BATCH_BYTES,
               max_lines=0, hash_bits=0, device=0, packfile_form="plain"):
    """One diff through the native pipeline (a DiffSession for this call
    only): packfiles is a list of serialised packfiles (bytes) and/or paths.
    Returns (results, stats) as DiffSession.run."""
    with DiffSession(key, compression, context, threads, batch_bytes, max_lines, hash_bits, device) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(pairs)


__all__ = ["line_table_device", "line_ids_device", "diff_script", "diff_ops", "diff_emit_plan", "diff_emit_device",
           "DiffSession", "diff_files", "DEFAULT_BATCH_BYTES", "LINE_DTYPE", "OP_DTYPE", "EMIT_DTYPE"]
