"""Sync on the device: the blobs of one repository as blobs of another.

The reference's synchronize() (cmd/plakar/subcommands/sync/sync.go:182-266)
handles every blob the destination lacks the same way: GetBlob decodes it with
the source repository's compression and key, PutBlob encodes it with the
destination's, and a packer writes destination packfiles.  transcode_device
does the first two for a batch without the plaintext leaving the device, and,
when both repositories name the same compression, without inflating at all:
only the GCM envelope changes (the re-key; with both keys set the plaintext
never exists in device memory either).  SyncSession is synchronize()'s loop over
source packfiles, one stage after the other, in Python.  SyncPipeline is the
same loop behind the C ABI (cdc_sync_*): batch k + 1 is gathered and uploaded
while batch k is transcoded and batch k - 1 is downloaded and packed, and the
blobs are never copied in Python.  Every device call goes through the C ABI
(cdc_transcode_device, cdc_transcode_size, cdc_sync_*; cdc_packfile_index and
cdc_packer_* through restore.packfile_index and packer.Packer).

SyncPipeline reads and writes packfiles in either form: the plain Serialize
form, or the form a repository keeps (PutPackfile; stored.py), per source with
add_packfiles(form=) and for the destination with dst_packfile_form=.

Out of scope: the snapshot, state and header records, and more than one device."""
import ctypes
import os
import time

import numpy as np

from . import _lib, packer
from . import stored as _stored
from ._lib import CdcError, ensure_init, lib
from .decode import _key, _ptr, _u64, _upload
from .encode import RANDOM_BYTES, _reservoir, encode_bound
from .restore import packfile_index

DEFAULT_BATCH_BYTES = 64 << 20
PATHS = ("copy", "rekey", "open", "seal", "reencode")


class TranscodeError(CdcError):
    """One blob's failure: CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_UNSUPPORTED or CDC_E_MISMATCH in .status."""


def _codec(c):
    """(key, compression) -> (key bytes or None, the C selector)."""
    key, compression = c
    return _key(key), _lib.compress_code(compression)


def path_of(src, dst):
    """The path cdc_transcode_device takes between two (key, compression)
    codecs: "copy", "rekey", "open", "seal" (same compression: the envelope
    only) or "reencode"."""
    (sk, sc), (dk, dc) = _codec(src), _codec(dst)
    if sc != dc:
        return "reencode"
    if sk is not None:
        return "rekey" if dk is not None else "open"
    return "seal" if dk is not None else "copy"


def transcode_size(length, src_encrypted, dst_encrypted):
    """cdc_transcode_size: the stored length after a transcode that keeps the
    compression; raises CdcError(CDC_E_CORRUPT) for a length no writer produces."""
    r = int(lib().cdc_transcode_size(int(length), int(bool(src_encrypted)), int(bool(dst_encrypted))))
    if r < 0:
        raise CdcError(r, "cdc_transcode_size")
    return r


def transcode_device(base, offsets, lens, out, src=(None, "LZ4"), dst=(None, "LZ4"), checksums=None, random=None,
                     device=0, stream=None, level=0):
    """cdc_transcode_device_level over torch uint8 tensors: the stored blobs at
    base[offsets[i]:offsets[i] + lens[i]], written by a repository with the codec
    `src` = (key, compression), as blobs of a repository with the codec `dst`,
    packed into `out`.  Returns (out_offsets, status): n + 1 int64 offsets and n
    int32 codes; a failed blob has status[i] != 0 and no bytes.  checksums: None,
    or one 32-byte SHA-256 per blob to verify first (CDC_E_MISMATCH).  random:
    56 bytes per blob when dst has a key (default: fresh OS random bytes).
    Raises CdcError(CDC_E_NOSPACE) when `out` is too small (.needed: the bytes
    to retry with).  Without checksums and with the same compression on both
    sides nothing is inflated: an encrypted source is authenticated by its GCM
    tags, an unencrypted one is copied unvalidated.  level: the match search of
    the re-encode path (0, 1 or 9, as encode.encode_device); the other paths
    ignore it."""
    import torch
    level = _lib.level_code(level)
    ensure_init()
    n = len(lens)
    (skey, scomp), (dkey, dcomp) = _codec(src), _codec(dst)
    offs_a, lens_a = _u64(offsets, n), _u64(lens, n)
    oo_a = np.zeros(n + 1, dtype=np.uint64)
    st_a = np.zeros(n, dtype=np.int32)
    sums = None
    if checksums is not None:
        sums = b"".join(bytes(c) for c in checksums)
        if len(sums) != 32 * n:
            raise ValueError("one 32-byte checksum (SHA-256) per blob")
    if dkey is not None:
        if random is None:  # fresh OS random bytes, drawn ahead (encode's reservoir)
            random = _reservoir.take_into(RANDOM_BYTES * n)
        elif len(random) != RANDOM_BYTES * n:
            raise ValueError(f"random: {RANDOM_BYTES} bytes per blob")
        else:
            random = bytes(random)
    else:
        random = None
    sc, dc = _lib.cdc_codec(scomp, skey), _lib.cdc_codec(dcomp, dkey)
    s = stream if stream is not None else torch.cuda.current_stream(device)
    rc = lib().cdc_transcode_device_level(int(device), ctypes.c_void_p(base.data_ptr()), _ptr(offs_a, ctypes.c_uint64),
                                          _ptr(lens_a, ctypes.c_uint64), n, ctypes.byref(sc), ctypes.byref(dc), sums,
                                          random, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                          _ptr(oo_a, ctypes.c_uint64), _ptr(st_a, ctypes.c_int32), level,
                                          ctypes.c_void_p(s.cuda_stream))
    if rc < 0:
        err = CdcError(rc, "cdc_transcode_device_level")
        err.needed = int(oo_a[n]) if rc == _lib.CDC_E_NOSPACE else None
        raise err
    return oo_a.astype(np.int64), st_a


def _first_cap(lens, src, dst):
    """A first capacity for `out`: exact when the compression stays, a guess
    (the call reports the need) when the blobs are decoded and encoded again."""
    (skey, scomp), (dkey, dcomp) = _codec(src), _codec(dst)
    total = int(np.asarray(lens, dtype=np.uint64).sum())
    if scomp == dcomp:
        return total + (88 * len(lens) + 28 * (total // 65536) if dkey is not None else 0)
    return sum(encode_bound(int(n) * (4 if scomp else 1), {0: False, 1: True, 2: "GZIP"}[dcomp], dkey is not None)
               for n in lens)


def _transcode_grow(base, offs, lens, src, dst, checksums, random, device, level=0):
    import torch
    cap = max(_first_cap(lens, src, dst), 1 << 16)
    while True:
        out = torch.empty(cap, dtype=torch.uint8, device=base.device)
        try:
            oo, st = transcode_device(base, offs, lens, out, src=src, dst=dst, checksums=checksums, random=random,
                                      device=device, level=level)
            return out, oo, st
        except CdcError as e:
            if e.status != _lib.CDC_E_NOSPACE or e.needed <= cap:
                raise
            cap = e.needed


def transcode_blobs(blobs, src=(None, "LZ4"), dst=(None, "LZ4"), checksums=None, random=None, device=0, level=0):
    """Transcode host byte buffers (upload, one transcode_device, download): a
    list with each blob's new encoding (bytes), or a TranscodeError in the
    place of a blob that failed.  level: as transcode_device."""
    level = _lib.level_code(level)
    if not len(blobs):
        return []
    base, offs, lens = _upload(blobs, device)
    out, oo, st = _transcode_grow(base, offs, lens, src, dst, checksums, random, device, level)
    host = out[:int(oo[-1])].cpu().numpy()
    return [TranscodeError(int(st[i]), f"blob {i}") if st[i] else host[oo[i]:oo[i + 1]].tobytes()
            for i in range(len(blobs))]


class SyncSession:
    """synchronize()'s loop (sync.go:182-266) over source packfiles in the
    Serialize form (what backup_files and packer.Packer produce and
    restore_files reads).

    For every index row of the source packfiles, in order, of every blob type:
    the row is skipped when its (type, checksum) is in `known` (the
    destination's BlobExists: a set of (type, checksum) tuples) or was already
    taken in this run, and, when run() is given `wanted`, unless it is in it.
    Up to batch_bytes of stored bytes are gathered, uploaded once, transcoded
    by one transcode_device call (with verify: the index checksums are checked
    first) and downloaded once; the surviving blobs go through
    packer.Packer.AddBlob with their type and checksum, and the packer flushes
    when AddBlob says so and at the end.

    run() returns (packfiles, failures, stats).  failures maps (type, checksum)
    to the blob's status, and the run goes on past a failed blob, as restore
    goes on past a failed file.  The reference aborts the snapshot at the first
    failed GetBlob, so a caller must not commit the destination snapshot when
    failures is not empty."""

    def __init__(self, src_key=None, src_compression="LZ4", dst_key=None, dst_compression="LZ4", verify=True,
                 known=None, max_size=None, batch_bytes=DEFAULT_BATCH_BYTES, timestamp=None, device=0, level=0):
        self.level = _lib.level_code(level)  # the re-encode path's match search (0, 1 or 9)
        self.src, self.dst = (src_key, src_compression), (dst_key, dst_compression)
        _codec(self.src), _codec(self.dst)  # ValueError for a bad key or compression name
        self.path = path_of(self.src, self.dst)
        self.verify = bool(verify)
        self.known = set() if known is None else known
        self.max_size = packer.DEFAULT_MAX_SIZE if max_size is None else int(max_size)
        self.batch_bytes = max(int(batch_bytes), 1)
        self.timestamp = timestamp
        self.device = device
        self._packs = []  # (bytes, rows)

    def add_packfile(self, packfile):
        """Register a source packfile: bytes or a path.  Raises
        CdcError(CDC_E_CORRUPT) for a malformed one."""
        if isinstance(packfile, (str, os.PathLike)):
            with open(packfile, "rb") as f:
                packfile = f.read()
        data = bytes(packfile)
        _, rows = packfile_index(data)
        self._packs.append((data, rows))

    def _batches(self, wanted, seen, stats):
        batch, size = [], 0
        for data, rows in self._packs:
            for typ, checksum, off, length in rows:
                k = (typ, checksum)
                if wanted is not None and k not in wanted:
                    continue
                if k in self.known or k in seen:
                    stats["skipped"] += 1
                    continue
                seen.add(k)
                if batch and size + length > self.batch_bytes:
                    yield batch
                    batch, size = [], 0
                batch.append((k, data, off, length))
                size += length
        if batch:
            yield batch

    def run(self, wanted=None):
        import torch
        stats = dict(blobs=0, skipped=0, failed=0, bytes_in=0, bytes_out=0, batches=0, packfiles=0, path=self.path,
                     gather_s=0.0, h2d_s=0.0, transcode_s=0.0, d2h_s=0.0, pack_s=0.0)
        wanted = None if wanted is None else set(wanted)
        packfiles, failures, seen = [], {}, set()
        pk = packer.Packer(self.max_size, self.timestamp)
        dev = torch.device("cuda", self.device)
        try:
            for batch in self._batches(wanted, seen, stats):
                t0 = time.perf_counter()
                lens = np.array([b[3] for b in batch], dtype=np.uint64)
                offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
                host = np.empty(max(int(offs[-1]), 1), dtype=np.uint8)
                for (_, data, off, length), o in zip(batch, offs):
                    host[int(o):int(o) + length] = np.frombuffer(data, dtype=np.uint8, count=length, offset=off)
                t1 = time.perf_counter()
                base = torch.from_numpy(host).to(dev)
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                sums = [b[0][1] for b in batch] if self.verify else None
                out, oo, st = _transcode_grow(base, offs[:-1], lens, self.src, self.dst, sums, None, self.device, self.level)
                t3 = time.perf_counter()
                got = out[:int(oo[-1])].cpu().numpy()
                t4 = time.perf_counter()
                for i, (k, _, _, length) in enumerate(batch):
                    stats["blobs"] += 1
                    stats["bytes_in"] += length
                    if st[i]:
                        failures[k] = int(st[i])
                        stats["failed"] += 1
                        continue
                    stats["bytes_out"] += int(oo[i + 1] - oo[i])
                    if pk.AddBlob(k[0], k[1], got[oo[i]:oo[i + 1]]):
                        packfiles.append(pk.Serialize())
                        pk.Reset()
                t5 = time.perf_counter()
                stats["batches"] += 1
                for name, dt in (("gather_s", t1 - t0), ("h2d_s", t2 - t1), ("transcode_s", t3 - t2),
                                 ("d2h_s", t4 - t3), ("pack_s", t5 - t4)):
                    stats[name] += dt
            if pk.Count():
                packfiles.append(pk.Serialize())
        finally:
            pk.close()
        stats["packfiles"] = len(packfiles)
        return packfiles, failures, stats


def _records(pairs):
    """(type, checksum) pairs as cdc_sync's 33-byte records, sorted ascending."""
    recs = sorted(bytes([int(t)]) + bytes(c) for t, c in pairs)
    if any(len(r) != 33 for r in recs):
        raise ValueError("a checksum is 32 bytes (SHA-256)")
    return b"".join(recs), len(recs)


class SyncPipeline:
    """A native sync context (cdc_sync_new): SyncSession's loop as a pipeline
    whose reads, uploads, downloads and packing overlap the device work.

    The arguments are SyncSession's, and known, wanted and failures are keyed
    the same way ((type, checksum) tuples).  readers and packers: threads (0: 8
    each).  With packers=1 the packfiles are SyncSession's, row for row; with
    more, every packfile still holds its rows in source order.  timestamp=None
    takes the time of the call, once, for every packfile of the context."""

    def __init__(self, src_key=None, src_compression="LZ4", dst_key=None, dst_compression="LZ4", verify=True,
                 known=None, max_size=None, batch_bytes=DEFAULT_BATCH_BYTES, timestamp=None, device=0, level=0,
                 readers=0, packers=0, dst_packfile_form="plain"):
        self._h = None
        self._keep = []  # packfile bytes the context reads from until it is freed
        dst_form = _lib.packfile_form_code(dst_packfile_form)
        level = _lib.level_code(level)
        self.src, self.dst = (src_key, src_compression), (dst_key, dst_compression)
        (skey, scomp), (dkey, dcomp) = _codec(self.src), _codec(self.dst)  # ValueError for a bad key or name
        self.path = path_of(self.src, self.dst)
        recs, nrecs = _records(known if known is not None else ())
        ensure_init()
        o = _lib.cdc_sync_opts()
        lib().cdc_sync_default_opts(ctypes.byref(o))
        o.src, o.dst = _lib.cdc_codec(scomp, skey), _lib.cdc_codec(dcomp, dkey)
        o.verify, o.level = int(bool(verify)), level
        o.packfile_max = 0 if max_size is None else int(max_size)
        o.batch_bytes = max(int(batch_bytes), 1)
        o.readers, o.packers = int(readers), int(packers)
        o.timestamp = time.time_ns() if timestamp is None else int(timestamp)
        kbuf = ctypes.create_string_buffer(recs, max(len(recs), 1))
        o.known, o.nknown = (ctypes.cast(kbuf, ctypes.c_void_p) if nrecs else None), nrecs
        h = ctypes.c_void_p()
        _lib.check(lib().cdc_sync_new(int(device), ctypes.byref(o), ctypes.byref(h)), "cdc_sync_new")
        self._h = h
        if dst_form != _lib.PACKFILE_PLAIN:
            _lib.check(lib().cdc_sync_set_packfile_form(self._h, dst_form), "cdc_sync_set_packfile_form")

    def add_packfile(self, packfile):
        """Register a source packfile: bytes (kept alive by the context) or a
        path, whose blobs are read during a run.  Raises CdcError(CDC_E_CORRUPT)
        for a malformed one."""
        if not self._h:
            raise ValueError("pipeline closed")
        if isinstance(packfile, (str, os.PathLike)):
            _lib.check(lib().cdc_sync_add_packfile_path(self._h, os.fsencode(packfile)), "cdc_sync_add_packfile_path")
            return
        buf = bytes(packfile)
        _lib.check(lib().cdc_sync_add_packfile(self._h, buf, len(buf)), "cdc_sync_add_packfile")
        self._keep.append(buf)

    def add_packfiles(self, packfiles, form="plain", rows=None):
        """Register many source packfiles (bytes and/or paths) in one call
        (cdc_sync_add_packfiles): form "plain" or "stored", the form a
        repository keeps, whose footers and indexes are all decoded with the
        source codec in two device calls; or rows, one list of (type,
        checksum, offset, length) per packfile (the repository state's), and
        nothing of a file's tail is read.  Returns the per-source statuses: 0,
        or the CDC_E_* code of a source that was not entered."""
        if not self._h:
            raise ValueError("pipeline closed")
        return _stored.add_packfiles("cdc_sync_add_packfiles", self._h, self._keep, packfiles, form, rows)

    def run(self, wanted=None, on_pack=None):
        """One sync (cdc_sync_run).  Returns (packfiles, failures, stats) as
        SyncSession.run does; stats holds the fields of cdc_sync_stats, `path`
        as its name in PATHS.  on_pack: None, or a callable that is handed
        each packfile (bytes) instead of the returned list and whose negative
        return value stops the run (CdcError with that status)."""
        if not self._h:
            raise ValueError("pipeline closed")
        packfiles, failures, errors = [], {}, []

        def pack_cb(_ctx, data, n):
            try:
                raw = ctypes.string_at(data, n)
                if on_pack is None:
                    packfiles.append(raw)
                    return 0
                r = on_pack(raw)
                return 0 if r is None else int(r)
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)
                return _lib.CDC_E_IO

        def fail_cb(_ctx, typ, checksum, status):
            try:
                failures[(int(typ), ctypes.string_at(checksum, 32))] = int(status)
            except Exception as e:  # noqa: BLE001 - re-raised after the call
                errors.append(e)

        wrecs, nw = (None, 0) if wanted is None else _records(wanted)
        wbuf = None if wrecs is None else ctypes.create_string_buffer(wrecs, max(len(wrecs), 1))
        st = _lib.cdc_sync_stats()
        st.struct_size = ctypes.sizeof(st)
        pcb, fcb = _lib.BACKUP_PACK_FN(pack_cb), _lib.SYNC_BLOB_FN(fail_cb)
        rc = lib().cdc_sync_run(self._h, None if wbuf is None else ctypes.cast(wbuf, ctypes.c_void_p), nw, pcb, fcb,
                                None, ctypes.byref(st))
        if errors:
            raise errors[0]
        _lib.check(rc, "cdc_sync_run")
        stats = {name: getattr(st, name) for name, _ in _lib.cdc_sync_stats._fields_ if name != "struct_size"}
        stats["path"] = PATHS[stats["path"]]
        return packfiles, failures, stats

    def close(self):
        if self._h:
            lib().cdc_sync_free(self._h)
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


def sync_packfiles(packfiles, src_key=None, src_compression="LZ4", dst_key=None, dst_compression="LZ4", verify=True,
                   known=None, wanted=None, max_size=None, batch_bytes=DEFAULT_BATCH_BYTES, timestamp=None, device=0,
                   level=0, readers=0, packers=0, packfile_form="plain", dst_packfile_form="plain"):
    """One sync through the native pipeline (a SyncPipeline for this call
    only): packfiles is a list of serialised packfiles (bytes) and/or paths.
    Returns (packfiles, failures, stats) as SyncPipeline.run."""
    with SyncPipeline(src_key, src_compression, dst_key, dst_compression, verify, known, max_size, batch_bytes,
                      timestamp, device, level, readers, packers, dst_packfile_form) as s:
        _stored.add_all(s, packfiles, packfile_form)
        return s.run(wanted)


__all__ = ["transcode_device", "transcode_blobs", "transcode_size", "path_of", "SyncSession", "SyncPipeline",
           "sync_packfiles", "TranscodeError", "DEFAULT_BATCH_BYTES", "PATHS"]
