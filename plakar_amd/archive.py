"""Archive on the device: the byte path of `plakar archive`
(cmd/plakar/subcommands/archive/archive.go) for its tar, tarball and zip formats.
The reference reads each file chunk by chunk, copies the bytes into an
archive/tar writer and pushes the tar stream through one gzip.NewWriter.
cdc_archive_run plans the tar stream in batches, decodes every distinct blob
of a batch once, assembles header blocks, chunk occurrences and padding into
the batch's image of the stream on the device, and for tarball deflates it
there: GzipStream writes one gzip member out of many device pieces.  For zip
(ZipSession, zip_files) a batch's image holds only file bytes, every entry of
the batch is deflated as its own raw stream in one call (zip_pieces_device),
the local headers and data descriptors are placed on the device and the host
writes the central directory after the last batch.  Every call goes through the
C ABI (cdc_gzip_stream_*, cdc_zip_pieces_device, cdc_archive_*)."""
import ctypes
import os

import numpy as np

from . import _lib
from . import stored as _stored
from ._lib import check, ensure_init, lib

DEFAULT_BATCH_BYTES = 256 << 20
FORMATS = {"tar": _lib.CDC_ARCHIVE_TAR, "tarball": _lib.CDC_ARCHIVE_TARGZ}


def gzip_stream_bound(n):
    """The most one piece call with n input bytes writes (header, joiner and
    trailer included)."""
    return int(lib().cdc_gzip_stream_bound(int(n)))


class GzipStream:
    """One RFC 1952 member written piece by piece: the outputs of piece(),
    concatenated, are what gzip.NewWriter(out) ... Close() gives for the
    concatenated inputs (any inflater reads them as one member).  Every
    piece ends on a byte boundary; the piece given with last=True closes the
    member (CRC-32 of the whole stream, ISIZE mod 2^32).  `level`: 0, 1
    for matches from up to 32 KiB back inside a piece, or 9 for the longest of
    four candidates and a lazy parse as well (set_level changes it until the
    first piece is written)."""

    def __init__(self, device=0, level=0):
        import torch  # noqa: F401  (torch's HIP runtime comes up before the library's)
        level = _lib.level_code(level)
        ensure_init()
        self.device = device
        self._h = ctypes.c_void_p()
        check(lib().cdc_gzip_stream_new(int(device), ctypes.byref(self._h)), "cdc_gzip_stream_new")
        if level:
            self.set_level(level)

    def set_level(self, level):
        """cdc_gzip_stream_set_level: CdcError CDC_E_INVALID once a piece has been written."""
        if not self._h:
            raise ValueError("the stream is closed")
        check(lib().cdc_gzip_stream_set_level(self._h, _lib.level_code(level)), "cdc_gzip_stream_set_level")

    def close(self):
        if self._h:
            lib().cdc_gzip_stream_free(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def piece_device(self, src, n, out, last=False, out_cap=None, stream=None):
        """Deflate the first n bytes of the device tensor `src` (uint8) into
        the device tensor `out`; returns the bytes written.  `out_cap`
        (default: all of `out`) is the room the library may use: CdcError
        CDC_E_NOSPACE when the piece needs more, nothing written then."""
        import torch
        if not self._h:
            raise ValueError("the stream is closed")
        n = int(n)
        if n > src.numel():
            raise ValueError("n is larger than src")
        cap = out.numel() if out_cap is None else int(out_cap)
        if cap > out.numel():
            raise ValueError("out_cap is larger than out")
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        got = ctypes.c_uint64()
        check(lib().cdc_gzip_stream_piece(self._h, ctypes.c_void_p(src.data_ptr() if n else None), n, int(bool(last)),
                                          ctypes.c_void_p(out.data_ptr()), cap, ctypes.byref(got),
                                          ctypes.c_void_p(st.cuda_stream)), "cdc_gzip_stream_piece")
        return int(got.value)

    def piece(self, data, last=False):
        """Deflate host bytes (bytes or a numpy uint8 array): the piece's
        output as bytes (empty for an empty piece that is not the last)."""
        import torch
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
            else np.asarray(data, np.uint8).ravel()
        dev = torch.device("cuda", self.device)
        src = torch.empty(max(a.size, 1), dtype=torch.uint8, device=dev)
        if a.size:
            src[:a.size].copy_(torch.from_numpy(np.array(a, copy=True)))  # a writable copy: bytes are not
        out = torch.empty(gzip_stream_bound(a.size), dtype=torch.uint8, device=dev)
        n = self.piece_device(src, a.size, out, last=last)
        return out[:n].cpu().numpy().tobytes()


class ArchiveEntry:
    """One entry of an archive: a file (its snapshot.Object, or any object
    with Chunks of Checksum and Length) or a directory (obj None).  `name` is
    str (UTF-8 in the archive) or bytes; `mode` the permission bits; `mtime`
    whole seconds."""

    def __init__(self, name, obj=None, mode=None, mtime=0, directory=False):
        self.name = os.fsencode(name) if isinstance(name, str) else bytes(name)
        self.obj = obj
        self.directory = bool(directory)
        if self.directory and obj is not None:
            raise ValueError("a directory has no object")
        self.mode = (0o755 if self.directory else 0o644) if mode is None else int(mode)
        self.mtime = int(mtime)


class ArchiveSession:
    """A native archive context (cdc_archive_new): the repository's Decode
    configuration (compression "LZ4", "GZIP" or None, the 32-byte key or
    None), the output format ("tar", or "tarball": tar.gz, the reference's
    default) and the registered packfiles.  `level`: the match search of the
    tar.gz member (0; 1: a 32-KiB window; 9: and four candidates per bucket, a
    lazy parse; cdc_archive_set_level)."""

    def __init__(self, key=None, compression="LZ4", format="tarball", verify=True, writers=8,
                 batch_bytes=DEFAULT_BATCH_BYTES, device=0, level=0):
        code = _lib.compress_code(compression)
        if format not in FORMATS:
            raise ValueError(f"unsupported format {format!r} (tar and tarball are implemented)")
        self._open("cdc_archive_new", key, code, FORMATS[format], verify, writers, batch_bytes, device, level)

    def _open(self, constructor, key, code, format_code, verify, writers, batch_bytes, device, level=0):
        self._h = None
        self._keep = []
        level = _lib.level_code(level)
        keybuf = None
        if key is not None:
            key = bytes(key)
            if len(key) != 32:
                raise ValueError("the repository key is 32 bytes (AES-256)")
            keybuf = ctypes.create_string_buffer(key, 32)
        ensure_init()
        o = _lib.cdc_archive_opts()
        lib().cdc_archive_default_opts(ctypes.byref(o))
        o.compress = code
        o.key = ctypes.cast(keybuf, ctypes.c_void_p) if keybuf is not None else None
        o.verify, o.writers, o.batch_bytes = int(bool(verify)), int(writers), int(batch_bytes)
        o.format = format_code
        h = ctypes.c_void_p()
        check(getattr(lib(), constructor)(int(device), ctypes.byref(o), ctypes.byref(h)), constructor)
        self._h = h
        if level:
            check(lib().cdc_archive_set_level(h, level), "cdc_archive_set_level")

    def add_packfile(self, packfile):
        """Register a packfile: bytes (kept alive by the session) or a path."""
        if not self._h:
            raise ValueError("session closed")
        if isinstance(packfile, (str, os.PathLike)):
            check(lib().cdc_archive_add_packfile_path(self._h, os.fsencode(packfile)), "cdc_archive_add_packfile_path")
            return
        buf = bytes(packfile)
        check(lib().cdc_archive_add_packfile(self._h, buf, len(buf)), "cdc_archive_add_packfile")
        self._keep.append(buf)

    def add_packfiles(self, packfiles, form="plain", rows=None):
        """Register many packfiles (bytes and/or paths) in one call
        (cdc_archive_add_packfiles): form "plain" or "stored", the form a repository
        keeps, whose footers and indexes are all decoded in two device calls;
        or rows, one list of (type, checksum, offset, length) per packfile
        (the repository state's), and nothing of a file's tail is read.
        Returns the per-source statuses: 0, or the CDC_E_* code of a source
        that was not entered."""
        if not self._h:
            raise ValueError("session closed")
        return _stored.add_packfiles("cdc_archive_add_packfiles", self._h, self._keep, packfiles, form, rows)

    def run(self, entries, path=None, on_data=None):
        """Write the entries (ArchiveEntry, in order) as one archive to `path`,
        or hand its bytes in order to on_data(bytes) (the reference's "-"), or
        with neither return them.  Returns (data, statuses, stats): data the
        archive's bytes when neither path nor on_data is given (else None),
        statuses[i] 0, CDC_E_NOTFOUND for an entry left out because a blob of
        it is in no packfile, or None for an entry a failed run did not
        reach; stats the fields of cdc_archive_stats.  A run that fails
        raises CdcError (its `entry` names the entry) and leaves no file."""
        if not self._h:
            raise ValueError("session closed")
        n = len(entries)
        ents = (_lib.cdc_archive_entry * max(n, 1))()
        keep = []
        for i, e in enumerate(entries):
            if b"\0" in e.name or not e.name:
                raise ValueError("an entry's name is not empty and holds no NUL byte")
            chunks = [] if e.directory or e.obj is None else e.obj.Chunks
            sums = b"".join(bytes(c.Checksum) for c in chunks)
            if len(sums) != 32 * len(chunks):
                raise ValueError("a chunk checksum is 32 bytes (SHA-256)")
            lens = np.array([int(c.Length) for c in chunks], dtype=np.uint32)
            sbuf = ctypes.create_string_buffer(sums, max(len(sums), 1))
            keep.append((sbuf, lens))
            ents[i].name = e.name
            ents[i].type = _lib.CDC_ARCHIVE_DIR if e.directory else _lib.CDC_ARCHIVE_FILE
            ents[i].mode, ents[i].mtime, ents[i].nchunks = e.mode, e.mtime, len(chunks)
            ents[i].checksums = ctypes.cast(sbuf, ctypes.c_void_p)
            ents[i].lengths = lens.ctypes.data if lens.size else None
        statuses = [None] * n
        parts, errors = [], []
        sink = on_data if on_data is not None else parts.append

        def data_cb(_ctx, p, ln):
            try:
                sink(ctypes.string_at(p, int(ln)))
                return 0
            except Exception as ex:  # noqa: BLE001 - re-raised after the call
                errors.append(ex)
                return 1

        def entry_cb(_ctx, index, status):
            statuses[int(index)] = int(status)

        dcb, ecb = _lib.ARCHIVE_DATA_FN(data_cb), _lib.ARCHIVE_ENTRY_FN(entry_cb)
        st = _lib.cdc_archive_stats()
        st.struct_size = ctypes.sizeof(st)
        rc = lib().cdc_archive_run(self._h, ents, n, os.fsencode(path) if path is not None else None, dcb, ecb, None,
                                   ctypes.byref(st))
        if errors:
            raise errors[0]
        if rc < 0:
            err = _lib.CdcError(rc, "cdc_archive_run")
            err.entry = int(st.failed_entry)
            raise err
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_archive_stats._fields_}
        return (b"".join(parts) if path is None and on_data is None else None), statuses, stats

    def close(self):
        if self._h:
            lib().cdc_archive_free(self._h)
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


class ZipSession(ArchiveSession):
    """A native archive context in zip mode (cdc_archive_new_zip): the
    reference's third format.  add_packfile, run and close are
    ArchiveSession's.  Directories among the entries are accepted and not
    written, as the reference writes none; names lose their leading slashes.
    `level`: the match search of the entries' DEFLATE streams, as ArchiveSession's."""

    def __init__(self, key=None, compression="LZ4", verify=True, writers=8, batch_bytes=DEFAULT_BATCH_BYTES, device=0,
                 level=0):
        self._h = None
        self._keep = []
        self._open("cdc_archive_new_zip", key, _lib.compress_code(compression), 0, verify, writers, batch_bytes, device,
                   level)


def zip_files(entries, packfiles, path=None, on_data=None, key=None, compression="LZ4", verify=True, writers=8,
              batch_bytes=DEFAULT_BATCH_BYTES, device=0, level=0, packfile_form="plain"):
    """One zip archive through the native pipeline (a ZipSession for this call
    only).  Returns (data, statuses, stats) as ArchiveSession.run; a
    directory's status is 0 though nothing is written for it."""
    with ZipSession(key, compression, verify, writers, batch_bytes, device, level) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(entries, path, on_data)


def zip_piece_bound(n, header_len=0):
    """The most one piece of n input bytes writes: its header, n and 5 bytes
    per 32-KiB span, the 6 of the longest joiner, the 24-byte descriptor."""
    return int(header_len) + int(n) + 5 * (-(-int(n) // 32768)) + 6 + 24


def zip_pieces_device(src, pieces, headers, out, out_cap=None, device=0, stream=None, level=0):
    """cdc_zip_pieces_device: deflate the pieces, each a dict with off and len
    (in the device tensor `src`, uint8), first, last, hdr_off and hdr_len (in
    the bytes `headers`), crc_reg (default 0xFFFFFFFF), csize_before and
    usize_before (default 0), into the device tensor `out`.  Returns (total,
    outs): outs[i] a dict of out_off, out_len, deflate_len, crc_reg and zip64.
    CdcError CDC_E_NOSPACE (its `total` the bytes needed) when out_cap
    (default: all of `out`) is smaller; nothing is written then.  `level`: 0,
    or 1 for matches from up to 32 KiB back inside a piece
    (cdc_zip_pieces_device_level)."""
    import torch
    level = _lib.level_code(level)
    ensure_init()
    n = len(pieces)
    pcs = (_lib.cdc_zip_piece * max(n, 1))()
    for i, p in enumerate(pieces):
        pcs[i].src_off, pcs[i].len = int(p["off"]), int(p["len"])
        pcs[i].first, pcs[i].last = int(bool(p.get("first"))), int(bool(p.get("last")))
        pcs[i].hdr_off, pcs[i].hdr_len = int(p.get("hdr_off", 0)), int(p.get("hdr_len", 0))
        pcs[i].crc_reg = int(p.get("crc_reg", 0xFFFFFFFF))
        pcs[i].csize_before, pcs[i].usize_before = int(p.get("csize_before", 0)), int(p.get("usize_before", 0))
    cap = out.numel() if out_cap is None else int(out_cap)
    if cap > out.numel():
        raise ValueError("out_cap is larger than out")
    headers = bytes(headers)
    outs = (_lib.cdc_zip_piece_out * max(n, 1))()
    total = ctypes.c_uint64()
    st = stream if stream is not None else torch.cuda.current_stream(device)
    args = (int(device), ctypes.c_void_p(src.data_ptr()), src.numel(), pcs, n, headers, len(headers),
            ctypes.c_void_p(out.data_ptr()), cap, outs, ctypes.byref(total))
    if level:
        rc = lib().cdc_zip_pieces_device_level(*args, level, ctypes.c_void_p(st.cuda_stream))
    else:
        rc = lib().cdc_zip_pieces_device(*args, ctypes.c_void_p(st.cuda_stream))
    if rc < 0:
        err = _lib.CdcError(rc, "cdc_zip_pieces_device")
        err.total = int(total.value)
        raise err
    fields = [name for name, _ in _lib.cdc_zip_piece_out._fields_]
    return int(total.value), [{f: int(getattr(outs[i], f)) for f in fields} for i in range(n)]


def archive_files(entries, packfiles, path=None, on_data=None, key=None, compression="LZ4", format="tarball",
                  verify=True, writers=8, batch_bytes=DEFAULT_BATCH_BYTES, device=0, level=0, packfile_form="plain"):
    """One archive through the native pipeline (an ArchiveSession for this call
    only): packfiles is a list of serialised packfiles (bytes) and/or paths.
    Returns (data, statuses, stats) as ArchiveSession.run."""
    with ArchiveSession(key, compression, format, verify, writers, batch_bytes, device, level) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(entries, path, on_data)


__all__ = ["GzipStream", "gzip_stream_bound", "ArchiveEntry", "ArchiveSession", "archive_files", "ZipSession", "zip_files",
           "zip_pieces_device", "zip_piece_bound", "DEFAULT_BATCH_BYTES"]
