"""Check on the device: a snapshot's chunks and object checksums verified.

The reference's `plakar check` (snapshot/check.go:56-113) reads every chunk of
a file, compares its SHA-256 with Chunk.Checksum and feeds it into a second
hasher whose sum must be Object.Checksum; `plakar checksum`
(cmd/plakar/subcommands/checksum/checksum.go:108-119) computes the same sum.
cdc_check_files does it per batch of file bytes: every distinct blob is read,
decoded and checked once, and each object is hashed where its blobs lie
(k_object_digest over the chunks' places in the plaintext buffer) or, the long
ones, on host threads.  No image is assembled and nothing but digests comes
back for the device's objects.  Every call goes through the C ABI
(cdc_object_digests_device, cdc_check_*)."""
import ctypes
import os

import numpy as np

from . import _lib
from . import stored as _stored
from ._lib import check, ensure_init, lib

DEFAULT_BATCH_BYTES = 256 << 20


def object_digests_device(src, objects, device=None, stream=None):
    """cdc_object_digests_device over a torch uint8 tensor: `objects` is a list
    of segment lists, a segment an (offset, length) in src; returns a device
    tensor of n x 32 bytes, row i the SHA-256 of object i's segments put
    together.  Synchronous on the current stream."""
    import torch
    ensure_init()
    n = len(objects)
    seg0 = np.zeros(n + 1, dtype=np.uint64)
    flat = []
    for i, segs in enumerate(objects):
        flat.extend(segs)
        seg0[i + 1] = len(flat)
    seg = np.asarray(flat, dtype=np.uint64).reshape(-1, 2)
    off, ln = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
    dev = src.device.index if device is None else device
    out = torch.zeros((n, 32), dtype=torch.uint8, device=src.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    p64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib().cdc_object_digests_device(int(dev), ctypes.c_void_p(src.data_ptr()), src.numel(), off.ctypes.data_as(p64),
                                         ln.ctypes.data_as(p64), len(off), seg0.ctypes.data_as(p64), n,
                                         ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s.cuda_stream))
    check(rc, "cdc_object_digests_device")
    return out


class CheckSession:
    """A native check context (cdc_check_new): Decode's configuration
    (compression "LZ4", "GZIP" or None, the 32-byte key or None), the
    registered packfiles and their locator, with its streams and buffers kept
    across runs.  fast: presence of the chunks only (check -fast), no device
    work.  host_min_len: 0 lets the model split a batch's objects between the
    device and the host, otherwise objects of at least that many bytes are
    hashed on the host."""

    def __init__(self, key=None, compression="LZ4", fast=False, threads=8, batch_bytes=DEFAULT_BATCH_BYTES,
                 host_min_len=0, device=0):
        code = _lib.compress_code(compression)
        self._h = None
        self._keep = []  # packfile bytes the context reads from until it is freed
        keybuf = None
        if key is not None:
            key = bytes(key)
            if len(key) != 32:
                raise ValueError("the repository key is 32 bytes (AES-256)")
            keybuf = ctypes.create_string_buffer(key, 32)
        ensure_init()
        o = _lib.cdc_check_opts()
        lib().cdc_check_default_opts(ctypes.byref(o))
        o.compress = code
        o.key = ctypes.cast(keybuf, ctypes.c_void_p) if keybuf is not None else None
        o.fast, o.threads, o.batch_bytes = int(bool(fast)), int(threads), int(batch_bytes)
        o.host_min_len = int(host_min_len)
        h = ctypes.c_void_p()
        check(lib().cdc_check_new(int(device), ctypes.byref(o), ctypes.byref(h)), "cdc_check_new")
        self._h = h

    def add_packfile(self, packfile):
        """Register a packfile: bytes (kept alive by the session) or a path."""
        if not self._h:
            raise ValueError("session closed")
        if isinstance(packfile, (str, os.PathLike)):
            check(lib().cdc_check_add_packfile_path(self._h, os.fsencode(packfile)), "cdc_check_add_packfile_path")
            return
        buf = bytes(packfile)
        check(lib().cdc_check_add_packfile(self._h, buf, len(buf)), "cdc_check_add_packfile")
        self._keep.append(buf)

    def add_packfiles(self, packfiles, form="plain", rows=None):
        """Register many packfiles (bytes and/or paths) in one call
        (cdc_check_add_packfiles): form "plain" or "stored", the form a repository
        keeps, whose footers and indexes are all decoded in two device calls;
        or rows, one list of (type, checksum, offset, length) per packfile
        (the repository state's), and nothing of a file's tail is read.
        Returns the per-source statuses: 0, or the CDC_E_* code of a source
        that was not entered."""
        if not self._h:
            raise ValueError("session closed")
        return _stored.add_packfiles("cdc_check_add_packfiles", self._h, self._keep, packfiles, form, rows)

    def run(self, objects, verify_checksum=True):
        """Check the objects (snapshot.Object: Chunks' Checksum and Length, and
        Checksum).  verify_checksum=False only computes the object checksums
        (plakar checksum).  Returns (results, stats): results[i] a dict of
        status (0 or the file's CDC_E_* code), bad_chunk, hashed (0 not, 1 on
        the device, 2 on the host), checksum (bytes, or None when not hashed)
        and size; stats the fields of cdc_check_stats."""
        if not self._h:
            raise ValueError("session closed")
        n = len(objects)
        files = (_lib.cdc_check_file * max(n, 1))()
        keep = []
        for i, obj in enumerate(objects):
            chunks = obj.Chunks
            sums = b"".join(bytes(c.Checksum) for c in chunks)
            if len(sums) != 32 * len(chunks):
                raise ValueError("a chunk checksum is 32 bytes (SHA-256)")
            lens = np.array([int(c.Length) for c in chunks], dtype=np.uint32)
            sbuf = ctypes.create_string_buffer(sums, max(len(sums), 1))
            obuf = None
            if verify_checksum:
                osum = bytes(obj.Checksum)
                if len(osum) != 32:
                    raise ValueError("an object checksum is 32 bytes (SHA-256)")
                obuf = ctypes.create_string_buffer(osum, 32)
            keep.append((sbuf, lens, obuf))
            files[i].nchunks = len(chunks)
            files[i].checksums = ctypes.cast(sbuf, ctypes.c_void_p)
            files[i].lengths = lens.ctypes.data if lens.size else None
            files[i].object_checksum = ctypes.cast(obuf, ctypes.c_void_p) if obuf is not None else None
        results = [None] * n
        errors = []

        def on_file(_ctx, rp):
            try:
                r = rp.contents
                results[int(r.index)] = dict(status=int(r.status), bad_chunk=int(r.bad_chunk), hashed=int(r.hashed),
                                             checksum=bytes(r.checksum) if r.hashed else None, size=int(r.size))
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)

        cb = _lib.CHECK_FILE_FN(on_file)
        st = _lib.cdc_check_stats()
        st.struct_size = ctypes.sizeof(st)
        rc = lib().cdc_check_files(self._h, files, n, cb, None, ctypes.byref(st))
        check(rc, "cdc_check_files")
        if errors:
            raise errors[0]
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_check_stats._fields_
                 if name not in ("struct_size", "reserved")}
        return results, stats

    def close(self):
        if self._h:
            lib().cdc_check_free(self._h)
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


def check_files(objects, packfiles, key=None, compression="LZ4", fast=False, threads=8,
                batch_bytes=DEFAULT_BATCH_BYTES, host_min_len=0, device=0, verify_checksum=True, packfile_form="plain"):
    """One check through the native pipeline (a CheckSession for this call
    only): packfiles is a list of serialised packfiles (bytes) and/or paths.
    Returns (results, stats) as CheckSession.run."""
    with CheckSession(key, compression, fast, threads, batch_bytes, host_min_len, device) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(objects, verify_checksum)


__all__ = ["object_digests_device", "CheckSession", "check_files", "DEFAULT_BATCH_BYTES"]
