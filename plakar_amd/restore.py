"""Restore on the device: packfiles and object records in, files out.

The reference reads a file back chunk by chunk (snapshot/restore.go:103-110,
snapshot/vfs/vfilep.go:58-122: one repo.GetBlob per chunk; repository/
repository.go:449-466 and 407-429: a state lookup, one ranged packfile read and
one Decode each).  cdc_restore_files does it per batch of output bytes: every
distinct blob of the batch is read and decoded once (and, with verify, hashed
and compared with its checksum), cdc_assemble_device copies it to every place
it occurs, and writer threads put the files on disk.  cdc_restore_ranges reads
byte ranges of files on the same context (read_ranges, SnapshotFile): a blob
is decoded only as far as the last byte asked for.  Every call goes through
the C ABI (cdc_packfile_index, cdc_assemble_device, cdc_restore_*)."""
import ctypes
import io
import os

import numpy as np

from . import _lib
from . import stored as _stored
from ._lib import check, ensure_init, lib

DEFAULT_BATCH_BYTES = 256 << 20


def packfile_index(data):
    """packfile.NewFromBytes (packfile/packfile.go:152-239) of a serialised
    packfile: (footer, rows), footer a dict of version, timestamp, count,
    index_offset and index_checksum, rows a list of (type, checksum, offset,
    length).  Raises CdcError(CDC_E_CORRUPT) for a malformed packfile."""
    data = bytes(data)
    L = lib()
    f = _lib.cdc_packfile_footer()
    need = ctypes.c_uint64()
    rc = L.cdc_packfile_index(data, len(data), ctypes.byref(f), None, 0, ctypes.byref(need))
    rows = None
    if rc == _lib.CDC_E_NOSPACE:
        rows = (_lib.cdc_packfile_row * need.value)()
        rc = L.cdc_packfile_index(data, len(data), ctypes.byref(f), rows, need.value, ctypes.byref(need))
    check(rc, "cdc_packfile_index")
    footer = dict(version=int(f.version), timestamp=int(f.timestamp), count=int(f.count),
                  index_offset=int(f.index_offset), index_checksum=bytes(f.index_checksum))
    return footer, [(int(r.type), bytes(r.checksum), int(r.offset), int(r.length)) for r in (rows or [])]


packfile_index_stored = _stored.packfile_index_stored


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1))


def assemble_device(src, segments, dst, device=None, stream=None):
    """cdc_assemble_device over torch uint8 tensors: dst[dst_off:dst_off + len] =
    src[src_off:src_off + len] for every (src_off, len, dst_off) of `segments`
    (destinations sorted and disjoint).  Asynchronous on the current stream."""
    import torch
    ensure_init()
    seg = np.asarray(segments, dtype=np.uint64).reshape(-1, 3)
    so, ln, do = _u64(seg[:, 0]), _u64(seg[:, 1]), _u64(seg[:, 2])
    dev = dst.device.index if device is None else device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    p64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib().cdc_assemble_device(int(dev), ctypes.c_void_p(src.data_ptr()), src.numel(), so.ctypes.data_as(p64),
                                   ln.ctypes.data_as(p64), do.ctypes.data_as(p64), len(so),
                                   ctypes.c_void_p(dst.data_ptr()), dst.numel(), ctypes.c_void_p(s.cuda_stream))
    check(rc, "cdc_assemble_device")


def _files(objects, dests=None):
    """The cdc_restore_file array of the objects, and what must outlive its use."""
    n = len(objects)
    files = (_lib.cdc_restore_file * max(n, 1))()
    keep = []
    for i, obj in enumerate(objects):
        chunks = obj.Chunks
        sums = b"".join(bytes(c.Checksum) for c in chunks)
        if len(sums) != 32 * len(chunks):
            raise ValueError("a chunk checksum is 32 bytes (SHA-256)")
        lens = np.array([int(c.Length) for c in chunks], dtype=np.uint32)
        sbuf = ctypes.create_string_buffer(sums, max(len(sums), 1))
        keep.append((sbuf, lens))
        files[i].path = os.fsencode(dests[i]) if dests is not None else None
        files[i].nchunks = len(chunks)
        files[i].checksums = ctypes.cast(sbuf, ctypes.c_void_p)
        files[i].lengths = lens.ctypes.data if lens.size else None
    return files, keep


class RestoreSession:
    """A native restore context (cdc_restore_new): Decode's configuration
    (compression "LZ4", "GZIP" or None, the 32-byte key or None), the registered
    packfiles and their locator, with its streams and buffers kept across
    runs.  add_packfile() takes a serialised packfile (bytes) or a path;
    run() restores a list of objects."""

    def __init__(self, key=None, compression="LZ4", verify=True, writers=8, batch_bytes=DEFAULT_BATCH_BYTES,
                 device=0):
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
        o = _lib.cdc_restore_opts()
        lib().cdc_restore_default_opts(ctypes.byref(o))
        o.compress = code
        o.key = ctypes.cast(keybuf, ctypes.c_void_p) if keybuf is not None else None
        o.verify, o.writers, o.batch_bytes = int(bool(verify)), int(writers), int(batch_bytes)
        h = ctypes.c_void_p()
        check(lib().cdc_restore_new(int(device), ctypes.byref(o), ctypes.byref(h)), "cdc_restore_new")
        self._h = h

    def add_packfile(self, packfile):
        """Register a packfile: bytes (kept alive by the session) or a path."""
        if not self._h:
            raise ValueError("session closed")
        if isinstance(packfile, (str, os.PathLike)):
            check(lib().cdc_restore_add_packfile_path(self._h, os.fsencode(packfile)), "cdc_restore_add_packfile_path")
            return
        buf = bytes(packfile)
        check(lib().cdc_restore_add_packfile(self._h, buf, len(buf)), "cdc_restore_add_packfile")
        self._keep.append(buf)

    def add_packfiles(self, packfiles, form="plain", rows=None):
        """Register many packfiles (bytes and/or paths) in one call
        (cdc_restore_add_packfiles): form "plain" or "stored", the form a repository
        keeps, whose footers and indexes are all decoded in two device calls;
        or rows, one list of (type, checksum, offset, length) per packfile
        (the repository state's), and nothing of a file's tail is read.
        Returns the per-source statuses: 0, or the CDC_E_* code of a source
        that was not entered."""
        if not self._h:
            raise ValueError("session closed")
        return _stored.add_packfiles("cdc_restore_add_packfiles", self._h, self._keep, packfiles, form, rows)

    def run(self, objects, dests=None):
        """Restore the objects (snapshot.Object, as backup_files returns them;
        only Chunks' Checksum and Length are read).  dests: one destination
        path per object, or None: the bytes come back.  Returns (contents,
        statuses, stats): contents[i] the file's bytes (None for a failed
        file, and for every file when dests are given), statuses[i] 0 or the
        file's CDC_E_* code, stats the fields of cdc_restore_stats."""
        if not self._h:
            raise ValueError("session closed")
        n = len(objects)
        if dests is not None and len(dests) != n:
            raise ValueError("one destination per object")
        files, keep = _files(objects, dests)  # noqa: F841 - keep holds the arrays the call reads
        statuses = [None] * n
        parts = [[] for _ in range(n)]
        errors = []

        def on_file(_ctx, rp):
            try:
                r = rp.contents
                i = int(r.index)
                statuses[i] = int(r.status)
                if r.status == 0 and dests is None:
                    parts[i].append(ctypes.string_at(r.data, int(r.data_len)) if r.data_len else b"")
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)

        cb = _lib.RESTORE_FILE_FN(on_file)
        st = _lib.cdc_restore_stats()
        rc = lib().cdc_restore_files(self._h, files, n, cb, None, ctypes.byref(st))
        check(rc, "cdc_restore_files")
        if errors:
            raise errors[0]
        contents = [b"".join(parts[i]) if dests is None and statuses[i] == 0 else None for i in range(n)]
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_restore_stats._fields_}
        return contents, statuses, stats

    def read_ranges(self, objects, ranges):
        """cdc_restore_ranges: byte ranges (object index, offset, length) of
        the objects, each meaning the file's bytes [offset, min(offset +
        length, size)).  Every blob a batch of ranges touches is decoded once
        and only as far as the last byte asked for.  Returns (contents,
        statuses, stats): contents[i] the range's bytes (None for a failed
        range), statuses[i] 0 or the range's CDC_E_* code (CDC_E_INVALID for
        an offset past the size), stats the fields of cdc_read_stats."""
        if not self._h:
            raise ValueError("session closed")
        n = len(ranges)
        rr = (_lib.cdc_read_range * max(n, 1))()
        for i, r in enumerate(ranges):
            fi, off, length = (int(v) for v in r)
            if fi < 0 or off < 0 or length < 0:
                raise ValueError("a range is (object index, offset, length), none of them negative")
            rr[i].file, rr[i].offset, rr[i].length = min(fi, 0xFFFFFFFF), off, length
        files, keep = _files(objects)  # noqa: F841 - keep holds the arrays the call reads
        statuses = [None] * n
        parts = [[] for _ in range(n)]
        errors = []

        def on_range(_ctx, rp):
            try:
                r = rp.contents
                i = int(r.index)
                statuses[i] = int(r.status)
                if r.status == 0:
                    parts[i].append(ctypes.string_at(r.data, int(r.data_len)) if r.data_len else b"")
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)

        cb = _lib.READ_RANGE_FN(on_range)
        st = _lib.cdc_read_stats()
        st.struct_size = ctypes.sizeof(st)
        rc = lib().cdc_restore_ranges(self._h, files, len(objects), rr, n, cb, None, ctypes.byref(st))
        check(rc, "cdc_restore_ranges")
        if errors:
            raise errors[0]
        contents = [b"".join(parts[i]) if statuses[i] == 0 else None for i in range(n)]
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_read_stats._fields_ if name not in ("struct_size", "reserved")}
        return contents, statuses, stats

    def close(self):
        if self._h:
            lib().cdc_restore_free(self._h)
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


def restore_files(objects, packfiles, dests=None, key=None, compression="LZ4", verify=True, writers=8,
                  batch_bytes=DEFAULT_BATCH_BYTES, device=0, packfile_form="plain"):
    """One restore through the native pipeline (a RestoreSession for this call
    only): packfiles is a list of serialised packfiles (bytes) and/or paths.
    Returns (contents, statuses, stats) as RestoreSession.run."""
    with RestoreSession(key, compression, verify, writers, batch_bytes, device) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(objects, dests)


def read_ranges(objects, ranges, packfiles, key=None, compression="LZ4", verify=True, writers=8,
                batch_bytes=DEFAULT_BATCH_BYTES, device=0, packfile_form="plain"):
    """One ranged read through the native pipeline (a RestoreSession for this
    call only), as restore_files.  Returns what RestoreSession.read_ranges does."""
    with RestoreSession(key, compression, verify, writers, batch_bytes, device) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.read_ranges(objects, ranges)


class SnapshotFile(io.RawIOBase):
    """A read-only binary file over one object of a RestoreSession, with
    VFilep's semantics (snapshot/vfs/vfilep.go:58-122, 168-197): read at the
    end returns b"", a seek before 0 or past the size raises.  Each device call
    (session.read_ranges) fetches max(asked, readahead) bytes into a host
    buffer, and reads are served from that window until they leave it; it is
    the only cache.  device_calls counts the calls."""

    def __init__(self, session, obj, readahead=4 << 20):
        super().__init__()
        if int(readahead) < 0:
            raise ValueError("readahead is a byte count: not negative")
        self._s, self._obj, self._ra = session, obj, int(readahead)
        self._size = sum(int(c.Length) for c in obj.Chunks)
        self._pos = 0
        self._win, self._win_off = b"", 0
        self.device_calls = 0

    @property
    def size(self):
        return self._size

    def readable(self):
        return True

    def seekable(self):
        return True

    def writable(self):
        return False

    def tell(self):
        self._open()
        return self._pos

    def _open(self):
        if self.closed:
            raise ValueError("I/O operation on closed file")

    def seek(self, offset, whence=io.SEEK_SET):
        self._open()
        offset = int(offset)
        if whence == io.SEEK_SET:
            new = offset
        elif whence == io.SEEK_CUR:
            new = self._pos + offset
        elif whence == io.SEEK_END:
            new = self._size + offset
        else:
            raise ValueError(f"invalid whence ({whence!r})")
        if new < 0:
            raise OSError("seek before the start of the file")
        if new > self._size:
            raise OSError("seek past the end of the file")
        self._pos = new
        return new

    def _fetch(self, n):
        """n bytes at the position (n <= what is left), through the window."""
        lo = self._pos - self._win_off
        if lo < 0 or lo + n > len(self._win):
            want = min(max(n, self._ra), self._size - self._pos)
            contents, statuses, _ = self._s.read_ranges([self._obj], [(0, self._pos, want)])
            self.device_calls += 1
            if statuses[0] != 0:
                raise _lib.CdcError(statuses[0], f"read of {want} bytes at {self._pos}")
            self._win, self._win_off, lo = contents[0], self._pos, 0
        return self._win[lo:lo + n]

    def read(self, size=-1):
        self._open()
        left = self._size - self._pos
        n = left if size is None or size < 0 else min(int(size), left)
        if n == 0:
            return b""
        data = self._fetch(n)
        self._pos += len(data)
        return data

    def readall(self):
        return self.read(-1)

    def readinto(self, b):
        m = memoryview(b).cast("B")
        data = self.read(len(m))
        m[:len(data)] = data
        return len(data)


__all__ = ["packfile_index", "packfile_index_stored", "assemble_device", "RestoreSession", "restore_files", "read_ranges", "SnapshotFile",
           "DEFAULT_BATCH_BYTES"]
