"""Grep on the device: fixed strings in snapshot files, per matching line.

The reference's only search (Snapshot.Search behind `plakar find`) matches
names, sizes and content types; it cannot look inside a file.  cdc_grep_files
takes a batch of files: every distinct blob is read, decoded and checked once,
the images are laid out in device memory, split into lines
(cdc_line_table_device's kernels) and searched by k_grep_scan for up to 32
fixed strings at once, `grep -F -e ... [-i]`; one 32-byte record per matching
line comes back (line number, byte offset, length, first column, which
patterns, how many occurrences), and on request the lines' bytes.  Every call
goes through the C ABI."""
import ctypes
import os

import numpy as np

from . import _lib
from . import stored as _stored
from ._lib import check, ensure_init, lib
from .diff import _file, _stream, _u64

DEFAULT_BATCH_BYTES = 256 << 20
HIT_DTYPE = np.dtype([("text", "<u4"), ("line", "<u4"), ("off", "<u8"), ("len", "<u4"), ("col", "<u4"), ("mask", "<u4"),
                      ("nocc", "<u4")])
_p64 = ctypes.POINTER(ctypes.c_uint64)


class _Patterns:
    """The patterns as the C ABI takes them: an array of pointers and one of lengths, kept alive here."""

    def __init__(self, patterns):
        if isinstance(patterns, (bytes, bytearray, memoryview)):
            patterns = [patterns]
        self.raw = [bytes(p) for p in patterns]
        n = len(self.raw)
        self.bufs = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in self.raw]
        self.ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in self.bufs])
        self.lens = (ctypes.c_uint32 * max(n, 1))(*[len(p) for p in self.raw])
        self.n = n


def grep_device(src, texts, patterns, ignore_case=False, limit=0, capacity=None, stream=None):
    """cdc_grep_device over a torch uint8 tensor: `texts` is a list of
    (offset, length) in src, ascending and not overlapping; `patterns` a list
    of bytes.  Returns (hits, lines, matched, binary): hits a host array of
    HIT_DTYPE in text and line order (at most `limit` per text when limit > 0),
    lines / matched the lines and the matching lines of each text, binary
    whether it holds a 0x00 byte.  capacity: room for that many records only
    (CdcError CDC_E_NOSPACE, with .needed, .lines, .matched and .binary, when
    it is too small); by default the call is made twice, the first time for
    the count."""
    import torch
    ensure_init()
    n = len(texts)
    t = np.asarray(texts, dtype=np.uint64).reshape(-1, 2)
    off, poff = _u64(t[:, 0])
    ln, pln = _u64(t[:, 1])
    P = _Patterns(patterns)
    lines = np.zeros(max(n, 1), dtype=np.uint64)
    matched = np.zeros(max(n, 1), dtype=np.uint64)
    binary = np.zeros(max(n, 1), dtype=np.uint8)
    total = ctypes.c_uint64(0)
    dev = src.device.index
    s = _stream(src, stream)
    flags = _lib.GREP_IGNORE_CASE if ignore_case else 0

    def call(hits, cap):
        return lib().cdc_grep_device(int(dev), ctypes.c_void_p(src.data_ptr()) if src.numel() else None, src.numel(), poff, pln, n,
                                     P.ptrs, P.lens, P.n, flags, int(limit),
                                     ctypes.c_void_p(hits.data_ptr()) if hits is not None else None, cap,
                                     lines.ctypes.data_as(_p64), matched.ctypes.data_as(_p64),
                                     binary.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(total), s)

    if capacity is None:
        rc = call(None, 0)
        if rc != _lib.CDC_E_NOSPACE:
            check(rc, "cdc_grep_device")
            return np.zeros(0, dtype=HIT_DTYPE), lines[:n].copy(), matched[:n].copy(), binary[:n].astype(bool)
        capacity = int(total.value)
    hits = torch.zeros((max(int(capacity), 1), 32), dtype=torch.uint8, device=src.device)
    rc = call(hits, int(capacity))
    if rc == _lib.CDC_E_NOSPACE:
        e = _lib.CdcError(rc, "cdc_grep_device")
        e.needed = int(total.value)
        e.lines, e.matched, e.binary = lines[:n].copy(), matched[:n].copy(), binary[:n].astype(bool)
        raise e
    check(rc, "cdc_grep_device")
    out = hits[:int(total.value)].cpu().numpy().reshape(-1).view(HIT_DTYPE).copy()
    return out, lines[:n].copy(), matched[:n].copy(), binary[:n].astype(bool)


class GrepSession:
    """A native grep context (cdc_grep_new): Decode's configuration
    (compression "LZ4", "GZIP" or None, the 32-byte key or None), the
    registered packfiles and their locator, with its stream and buffers kept
    across runs."""

    def __init__(self, key=None, compression="LZ4", threads=8, batch_bytes=DEFAULT_BATCH_BYTES, max_lines=0, device=0):
        code = _lib.compress_code(compression)
        self._h = None
        self._keep = []
        keybuf = None
        if key is not None:
            key = bytes(key)
            if len(key) != 32:
                raise ValueError("the repository key is 32 bytes (AES-256)")
            keybuf = ctypes.create_string_buffer(key, 32)
        ensure_init()
        o = _lib.cdc_grep_opts()
        lib().cdc_grep_default_opts(ctypes.byref(o))
        o.compress = code
        o.key = ctypes.cast(keybuf, ctypes.c_void_p) if keybuf is not None else None
        o.threads, o.batch_bytes, o.max_lines = int(threads), int(batch_bytes), int(max_lines)
        h = ctypes.c_void_p()
        check(lib().cdc_grep_new(int(device), ctypes.byref(o), ctypes.byref(h)), "cdc_grep_new")
        self._h = h

    def add_packfile(self, packfile):
        """Register a packfile: bytes (kept alive by the session) or a path."""
        if not self._h:
            raise ValueError("session closed")
        if isinstance(packfile, (str, os.PathLike)):
            check(lib().cdc_grep_add_packfile_path(self._h, os.fsencode(packfile)), "cdc_grep_add_packfile_path")
            return
        buf = bytes(packfile)
        check(lib().cdc_grep_add_packfile(self._h, buf, len(buf)), "cdc_grep_add_packfile")
        self._keep.append(buf)

    def add_packfiles(self, packfiles, form="plain", rows=None):
        """Register many packfiles (bytes and/or paths) in one call
        (cdc_grep_add_packfiles): form "plain" or "stored", or rows, as
        DiffSession.add_packfiles.  Returns the per-source statuses."""
        if not self._h:
            raise ValueError("session closed")
        return _stored.add_packfiles("cdc_grep_add_packfiles", self._h, self._keep, packfiles, form, rows)

    def run(self, files, patterns, ignore_case=False, limit=0, want_text=False, max_line_bytes=0):
        """Search the files (snapshot.Objects: Chunks' Checksum and Length) for
        the patterns (a list of bytes).  Returns (results, stats): results[i] a
        dict of status (0 or the file's CDC_E_* code), bad_chunk, binary, size,
        lines, matched, hits (HIT_DTYPE; text is i, off the line's offset in
        the file; at most `limit` of them, 0: 65,536) and text (bytes: with
        want_text, per hit the line's first max_line_bytes bytes, 0: 4,096, and
        a newline); stats the fields of cdc_grep_stats."""
        if not self._h:
            raise ValueError("session closed")
        n = len(files)
        arr = (_lib.cdc_check_file * max(n, 1))()
        keep = []
        for i, obj in enumerate(files):
            _file(arr[i], obj, keep)
        P = _Patterns(patterns)
        q = _lib.cdc_grep_query()
        q.struct_size = ctypes.sizeof(q)
        q.flags = _lib.GREP_IGNORE_CASE if ignore_case else 0
        q.patterns = ctypes.cast(P.ptrs, ctypes.c_void_p)
        q.pattern_len = ctypes.cast(P.lens, ctypes.c_void_p)
        q.npatterns = P.n
        q.limit, q.want_text, q.max_line_bytes = int(limit), int(bool(want_text)), int(max_line_bytes)
        results = [None] * n
        errors = []

        def on_file(_ctx, rp):
            try:
                r = rp.contents
                hits = np.zeros(int(r.nhits), dtype=HIT_DTYPE)
                if r.nhits:
                    ctypes.memmove(hits.ctypes.data, r.hits, 32 * int(r.nhits))
                text = ctypes.string_at(r.text, int(r.text_len)) if r.text_len else b""
                results[int(r.index)] = dict(status=int(r.status), bad_chunk=int(r.bad_chunk), binary=bool(r.binary),
                                             size=int(r.size), lines=int(r.lines), matched=int(r.matched), hits=hits,
                                             text=text)
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)

        cb = _lib.GREP_FILE_FN(on_file)
        st = _lib.cdc_grep_stats()
        st.struct_size = ctypes.sizeof(st)
        rc = lib().cdc_grep_files(self._h, ctypes.byref(q), arr, n, cb, None, ctypes.byref(st))
        check(rc, "cdc_grep_files")
        if errors:
            raise errors[0]
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_grep_stats._fields_
                 if name not in ("struct_size", "reserved")}
        return results, stats

    def close(self):
        if self._h:
            lib().cdc_grep_free(self._h)
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


def grep_files(files, packfiles, patterns, key=None, compression="LZ4", ignore_case=False, limit=0, want_text=False,
               max_line_bytes=0, threads=8, batch_bytes=DEFAULT_BATCH_BYTES, max_lines=0, device=0, packfile_form="plain"):
    """One search through the native pipeline (a GrepSession for this call
    only): packfiles is a list of serialised packfiles (bytes) and/or paths.
    Returns (results, stats) as GrepSession.run."""
    with GrepSession(key, compression, threads, batch_bytes, max_lines, device) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(files, patterns, ignore_case, limit, want_text, max_line_bytes)


__all__ = ["grep_device", "GrepSession", "grep_files", "DEFAULT_BATCH_BYTES", "HIT_DTYPE"]
