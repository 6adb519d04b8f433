"""The repository state: its blob index, read, merged and queried on the device.

    RebuildState                     repository/repository.go:58-164
    DeserializeStream, Merge         repository/state/state.go:235-348, 384-455
    BlobExists, GetSubpartForBlob    state.go:512-562, 457-510
    ListBlobs, ListSnapshots         state.go:649-719
    SerializeStream                  state.go:132-216

State is the aggregate every plakar command builds when it opens a repository:
merge() takes the state files as the repository stores them (Encode of the
serialised state), decodes them all in one device call and inserts their rows
into a hash table in device memory; the queries run against that table.  It is
the producer of what the sessions consume: BackupSession's `known`
(list_blobs), add_packfiles' `rows` (packfile_rows), check's BlobExists.  The
merge rule is SetPackfileForBlob's, a key already present keeps its location,
with the state given first winning (the reference's order among duplicates is
Go's map order).  Everything goes through the C ABI (cdc_state_*)."""
import ctypes
import hashlib
import time

import numpy as np

from . import _lib
from ._lib import check, lib

# packfile.Type (packfile/packfile.go:17-25)
TYPE_SNAPSHOT, TYPE_CHUNK, TYPE_OBJECT, TYPE_FILE, TYPE_DIRECTORY, TYPE_CHILD, TYPE_DATA, TYPE_SIGNATURE, TYPE_ERROR = \
    range(9)
TYPES = tuple(range(9))

ROW_DTYPE = np.dtype(_lib.STATE_ROW_DTYPE_FIELDS)
assert ROW_DTYPE.itemsize == ctypes.sizeof(_lib.cdc_state_row) == 80


def _type(typ):
    typ = int(typ)
    if not 0 <= typ <= 8:
        raise ValueError(f"invalid blob type {typ} (packfile.TYPE_* are 0..8)")
    return typ


def _sums(checksums):
    """n checksums as one contiguous (n, 32) uint8 array: a list of 32-byte
    strings, one bytes object of 32 * n, or an array of that shape."""
    if isinstance(checksums, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(checksums), dtype=np.uint8)
    elif isinstance(checksums, np.ndarray):
        a = np.ascontiguousarray(checksums, dtype=np.uint8).reshape(-1)
    else:
        parts = [bytes(c) for c in checksums]
        if any(len(p) != 32 for p in parts):
            raise ValueError("a checksum is 32 bytes (SHA-256)")
        a = np.frombuffer(b"".join(parts), dtype=np.uint8)
    if a.size % 32:
        raise ValueError("a checksum is 32 bytes (SHA-256)")
    return a.reshape(-1, 32)


def _column(rows, name):
    """The 32-byte column `name` of a row array as a list of bytes."""
    raw = np.ascontiguousarray(rows[name]).tobytes()
    return [raw[k:k + 32] for k in range(0, len(raw), 32)]


class State:
    """A native aggregate state (cdc_state_new) for a repository with this
    key (32 bytes or None) and compression ("LZ4", "GZIP" or None)."""

    def __init__(self, key=None, compression="LZ4", device=0):
        self._h = None
        code = _lib.compress_code(compression)
        if key is not None:
            key = bytes(key)
            if len(key) != 32:
                raise ValueError("the repository key is 32 bytes (AES-256)")
        h = ctypes.c_void_p()
        check(lib().cdc_state_new(int(device), code, key, ctypes.byref(h)), "cdc_state_new")
        self._h = h

    def _handle(self):
        if not self._h:
            raise ValueError("state closed")
        return self._h

    def merge(self, states, ids=None, form="stored"):
        """cdc_state_merge: enter the state files `states` (bytes each; form
        "stored": as the repository keeps them, "plain": the serialised
        bytes), named ids[i] (32 bytes; default: the SHA-256 of the bytes
        given).  Returns the per-state statuses: 0, or the CDC_E_* code of a
        state that was rejected as a whole (CDC_E_AUTH, CDC_E_CORRUPT, ...).
        Earlier states, of this call and of earlier calls, keep precedence."""
        code = _lib.state_form_code(form)
        states = [bytes(s) for s in states]
        n = len(states)
        if ids is None:
            ids = [hashlib.sha256(s).digest() for s in states]
        ids = [bytes(i) for i in ids]
        if len(ids) != n or any(len(i) != 32 for i in ids):
            raise ValueError("ids: one 32-byte checksum per state")
        arr = (_lib.cdc_state_src * max(n, 1))()
        keep = []
        for i, s in enumerate(states):
            buf = ctypes.create_string_buffer(s, max(len(s), 1))
            keep.append(buf)
            arr[i].bytes = ctypes.cast(buf, ctypes.c_void_p)
            arr[i].len = len(s)
            ctypes.memmove(arr[i].id, ids[i], 32)
            arr[i].form = code
        status = (ctypes.c_int32 * max(n, 1))()
        check(lib().cdc_state_merge(self._handle(), arr, n, status), "cdc_state_merge")
        del keep
        return [int(status[i]) for i in range(n)]

    def lookup(self, type, checksums):
        """cdc_state_lookup: one row (ROW_DTYPE) per checksum, `found` 0 or 1."""
        typ = _type(type)
        q = _sums(checksums)
        out = np.zeros(len(q), dtype=ROW_DTYPE)
        check(lib().cdc_state_lookup(self._handle(), typ, q.ctypes.data, len(q), out.ctypes.data), "cdc_state_lookup")
        return out

    def lookup_device(self, type, digests, stream=None):
        """cdc_state_lookup_device: digests an (n, 32) uint8 CUDA tensor (as
        hashing.chunk_digests returns them); the rows come back as an (n, 80)
        uint8 CUDA tensor (view its .cpu().numpy() as ROW_DTYPE).  Asynchronous
        on `stream` (default: the current stream)."""
        import torch
        typ = _type(type)
        if digests.dtype != torch.uint8 or not digests.is_cuda or not digests.is_contiguous() or \
                digests.dim() != 2 or digests.shape[1] != 32:
            raise ValueError("expected a contiguous (n, 32) uint8 CUDA tensor")
        n = digests.shape[0]
        out = torch.empty((n, 80), dtype=torch.uint8, device=digests.device)
        if stream is None:
            stream = torch.cuda.current_stream(digests.device)
        check(lib().cdc_state_lookup_device(self._handle(), typ, ctypes.c_void_p(digests.data_ptr()), n,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream.cuda_stream)),
              "cdc_state_lookup_device")
        return out

    def blob_exists(self, type, checksums):
        """BlobExists (state.go:512-562) for many checksums: a numpy bool array."""
        return self.lookup(type, checksums)["found"].astype(bool)

    def get_subpart_for_blob(self, type, checksums):
        """GetSubpartForBlob (state.go:457-510) for many checksums: (found bool
        array, list of packfile checksums, offsets, lengths); a blob that is
        not there has the zero checksum, 0 and 0, as in the reference."""
        r = self.lookup(type, checksums)
        return r["found"].astype(bool), _column(r, "packfile"), r["offset"].copy(), r["length"].copy()

    def rows(self, type):
        """cdc_state_rows: the aggregate's rows of one type (ROW_DTYPE), in no
        particular order; of TYPE_SNAPSHOT, those not deleted."""
        typ = _type(type)
        need = ctypes.c_uint64()
        h = self._handle()
        rc = lib().cdc_state_rows(h, typ, None, 0, ctypes.byref(need))
        out = np.zeros(need.value, dtype=ROW_DTYPE)
        if rc == _lib.CDC_E_NOSPACE:
            rc = lib().cdc_state_rows(h, typ, out.ctypes.data, len(out), ctypes.byref(need))
        check(rc, "cdc_state_rows")
        return out[:need.value]

    def list_blobs(self, type):
        """ListBlobs (state.go:649-696): the checksums of one type, as a list."""
        return _column(self.rows(type), "checksum")

    def list_snapshots(self):
        """ListSnapshots (state.go:698-719): the snapshots no merged state deleted."""
        return _column(self.rows(TYPE_SNAPSHOT), "checksum")

    def extends(self):
        """Metadata.Extends: the ids of the states entered, in order."""
        need = ctypes.c_uint64()
        h = self._handle()
        rc = lib().cdc_state_extends(h, None, 0, ctypes.byref(need))
        buf = ctypes.create_string_buffer(max(32 * need.value, 1))
        if rc == _lib.CDC_E_NOSPACE:
            rc = lib().cdc_state_extends(h, buf, need.value, ctypes.byref(need))
        check(rc, "cdc_state_extends")
        raw = buf.raw[:32 * need.value]
        return [raw[k:k + 32] for k in range(0, len(raw), 32)]

    def info(self):
        """cdc_state_info as a dict (rows: a list by type)."""
        st = _lib.cdc_state_stats()
        st.struct_size = ctypes.sizeof(st)
        check(lib().cdc_state_info(self._handle(), ctypes.byref(st)), "cdc_state_info")
        d = {name: getattr(st, name) for name, _ in _lib.cdc_state_stats._fields_ if name not in ("struct_size", "reserved")}
        d["rows"] = [int(x) for x in st.rows]
        return d

    def packfile_rows(self, type=TYPE_CHUNK, checksums=None):
        """{packfile checksum: [(type, checksum, offset, length), ...]} in the
        shape add_packfiles(..., rows=...) takes, sorted by offset within a
        packfile: every row of `type`, or with `checksums` only the rows of
        those blobs, so only the packfiles they need.  A checksum the state
        does not have raises KeyError."""
        if checksums is None:
            r = self.rows(type)
        else:
            r = self.lookup(type, checksums)
            missing = np.flatnonzero(r["found"] == 0)
            if missing.size:
                raise KeyError(bytes(r["checksum"][missing[0]].tobytes()).hex())
        r = r[np.argsort(r["offset"], kind="stable")]
        out = {}
        seen = set()
        for pack, csum, off, ln, typ in zip(_column(r, "packfile"), _column(r, "checksum"), r["offset"].tolist(),
                                            r["length"].tolist(), r["type"].tolist()):
            if (pack, csum) in seen:
                continue
            seen.add((pack, csum))
            out.setdefault(pack, []).append((typ, csum, off, ln))
        return out

    def delete_snapshots(self, checksums, when_ns=None):
        """cdc_state_delete_snapshots: State.DeleteSnapshot (state.go:628-647)
        for many snapshots.  Returns the statuses: 0, or CDC_E_NOTFOUND for a
        checksum the aggregate has no snapshot row for.  rows(TYPE_SNAPSHOT)
        leaves the deleted ones out from then on; serialize_rows(deleted=...)
        writes the delta that stores the deletion."""
        q = _sums(checksums)
        when = time.time_ns() if when_ns is None else int(when_ns)
        status = (ctypes.c_int32 * max(len(q), 1))()
        check(lib().cdc_state_delete_snapshots(self._handle(), q.ctypes.data, len(q), when, status),
              "cdc_state_delete_snapshots")
        return [int(status[i]) for i in range(len(q))]

    def mark(self, refs):
        """cdc_state_mark: mark the rows that `refs` name, (type, checksum)
        pairs in any order, duplicates welcome (what a kept snapshot's
        ListChunks, ListObjects, ... yield), or their 33-byte records as one
        bytes object.  Returns (found, missing): a numpy bool array in the
        order given, and the count of references the aggregate does not have.
        Marks accumulate until clear_marks()."""
        if isinstance(refs, (bytes, bytearray, memoryview)):
            raw = bytes(refs)
        else:
            parts = []
            for typ, csum in refs:
                csum = bytes(csum)
                if len(csum) != 32:
                    raise ValueError("a checksum is 32 bytes (SHA-256)")
                parts.append(bytes([_type(typ)]) + csum)
            raw = b"".join(parts)
        if len(raw) % 33:
            raise ValueError("a reference is 33 bytes: the type, then the checksum")
        n = len(raw) // 33
        found = np.zeros(n, dtype=np.uint8)
        missing = ctypes.c_uint64()
        check(lib().cdc_state_mark(self._handle(), raw if n else None, n, found.ctypes.data if n else None,
                                   ctypes.byref(missing)), "cdc_state_mark")
        return found.astype(bool), int(missing.value)

    def mark_device(self, type, digests, found=False, stream=None):
        """cdc_state_mark_device: mark the rows of `type` that the digests
        name, an (n, 32) uint8 CUDA tensor as hashing.chunk_digests returns
        them.  Asynchronous on `stream` (default: the current stream).  With
        found=True an (n,) uint8 CUDA tensor of 0/1 comes back, else None."""
        import torch
        typ = _type(type)
        if digests.dtype != torch.uint8 or not digests.is_cuda or not digests.is_contiguous() or \
                digests.dim() != 2 or digests.shape[1] != 32:
            raise ValueError("expected a contiguous (n, 32) uint8 CUDA tensor")
        n = digests.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=digests.device) if found else None
        if stream is None:
            stream = torch.cuda.current_stream(digests.device)
        check(lib().cdc_state_mark_device(self._handle(), typ, ctypes.c_void_p(digests.data_ptr()), n,
                                          ctypes.c_void_p(out.data_ptr()) if found and n else None,
                                          ctypes.c_void_p(stream.cuda_stream)), "cdc_state_mark_device")
        return out

    def clear_marks(self):
        """cdc_state_clear_marks: forget every mark."""
        check(lib().cdc_state_clear_marks(self._handle()), "cdc_state_clear_marks")

    def sweep(self, keep_types=(TYPE_SNAPSHOT,), repack_permille=500):
        """cdc_state_sweep: the plan of a cleanup (a SweepPlan) from the marks
        set so far.  keep_types: the types whose rows are live without a mark
        (an iterable, or the bit mask itself); repack_permille: a packfile
        with live rows whose live bytes are below this many thousandths of
        its extent is to be rewritten."""
        o = _lib.cdc_sweep_opts()
        lib().cdc_sweep_default_opts(ctypes.byref(o))
        if isinstance(keep_types, int):
            o.keep_types = keep_types
        else:
            o.keep_types = 0
            for t in keep_types:
                o.keep_types |= 1 << _type(t)
        if not 0 <= int(repack_permille) <= 1000:
            raise ValueError("repack_permille: 0..1000")
        o.repack_permille = int(repack_permille)
        h = ctypes.c_void_p()
        check(lib().cdc_state_sweep(self._handle(), ctypes.byref(o), ctypes.byref(h)), "cdc_state_sweep")
        try:
            return SweepPlan._from_handle(h)
        finally:
            lib().cdc_sweep_free(h)

    def close(self):
        if self._h:
            lib().cdc_state_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


PACK_DTYPE = np.dtype(_lib.SWEEP_PACK_DTYPE_FIELDS)
assert PACK_DTYPE.itemsize == ctypes.sizeof(_lib.cdc_sweep_pack) == 88
VERDICTS = {_lib.SWEEP_KEEP: "keep", _lib.SWEEP_DROP: "drop", _lib.SWEEP_REPACK: "repack"}


class SweepPlan:
    """What State.sweep found (cdc_sweep_*), copied to the host:

    packs        PACK_DTYPE array, ascending in first_record
    kept_rows    ROW_DTYPE array: the live rows of KEEP packfiles in
                 record-number order
    repack_rows  ROW_DTYPE array: the live rows of REPACK packfiles, grouped
                 by packfile in the order of `packs`, ascending in offset;
                 packs[i]'s are repack_rows[row_first : row_first + row_count]
    info         cdc_sweep_stats as a dict"""

    def __init__(self, packs, kept_rows, repack_rows, info):
        self.packs, self.kept_rows, self.repack_rows, self.info = packs, kept_rows, repack_rows, info

    @classmethod
    def _from_handle(cls, h):
        L = lib()

        def fetch(fn, dtype):
            need = ctypes.c_uint64()
            rc = fn(h, None, 0, ctypes.byref(need))
            out = np.zeros(need.value, dtype=dtype)
            if rc == _lib.CDC_E_NOSPACE:
                rc = fn(h, out.ctypes.data, len(out), ctypes.byref(need))
            check(rc, "cdc_sweep")
            return out

        st = _lib.cdc_sweep_stats()
        st.struct_size = ctypes.sizeof(st)
        check(L.cdc_sweep_info(h, ctypes.byref(st)), "cdc_sweep_info")
        info = {name: getattr(st, name) for name, _ in _lib.cdc_sweep_stats._fields_ if name not in ("struct_size", "reserved")}
        return cls(fetch(L.cdc_sweep_packs, PACK_DTYPE), fetch(L.cdc_sweep_kept_rows, ROW_DTYPE),
                   fetch(L.cdc_sweep_repack_rows, ROW_DTYPE), info)

    def packfiles(self, verdict):
        """The checksums of the packfiles with this verdict ("keep", "drop",
        "repack" or a CDC_SWEEP_* value), in the list's order."""
        code = {v: k for k, v in VERDICTS.items()}.get(verdict, verdict)
        return _column(self.packs[self.packs["verdict"] == code], "packfile")

    def repack_slices(self):
        """[(packfile checksum, [(type, checksum, offset, length), ...])] of
        the REPACK packfiles: add_packfiles(..., rows=...)'s shape."""
        out = []
        sums = _column(self.repack_rows, "checksum")
        typ, off, ln = (self.repack_rows[k].tolist() for k in ("type", "offset", "length"))
        for pack, v, first, count in zip(_column(self.packs, "packfile"), self.packs["verdict"].tolist(),
                                         self.packs["row_first"].tolist(), self.packs["row_count"].tolist()):
            if v == _lib.SWEEP_REPACK:
                out.append((pack, [(typ[k], sums[k], off[k], ln[k]) for k in range(first, first + count)]))
        return out


def rows_as_tuples(rows):
    """A ROW_DTYPE array as serialize_rows' (type, checksum, packfile, offset, length) tuples."""
    return list(zip(rows["type"].tolist(), _column(rows, "checksum"), _column(rows, "packfile"), rows["offset"].tolist(),
                    rows["length"].tolist()))


def serialize_rows(rows, timestamp_ns, aggregate=False, extends=(), deleted=()):
    """cdc_state_serialize_deleted: SerializeStream of a state holding `rows`,
    an iterable of (type, blob checksum, packfile checksum, offset, length),
    entered in order with SetPackfileForBlob, and the deleted snapshots
    `deleted`, (checksum, time_ns) pairs.  Host only."""
    rows = list(rows)
    arr = np.zeros(len(rows), dtype=ROW_DTYPE)
    for k, (typ, csum, pack, off, ln) in enumerate(rows):
        csum, pack = bytes(csum), bytes(pack)
        if len(csum) != 32 or len(pack) != 32:
            raise ValueError("a checksum is 32 bytes (SHA-256)")
        arr[k] = (csum, pack, int(off), int(ln), _type(typ), 0, b"")
    ext = b"".join(bytes(e) for e in extends)
    if len(ext) % 32:
        raise ValueError("extends: 32-byte state ids")
    deleted = [(bytes(c), int(t)) for c, t in deleted]
    if any(len(c) != 32 for c, _ in deleted):
        raise ValueError("a checksum is 32 bytes (SHA-256)")
    gone = b"".join(c for c, _ in deleted)
    times = np.array([t for _, t in deleted], dtype=np.int64)
    n = ctypes.c_uint64()
    L = lib()
    args = (arr.ctypes.data if len(rows) else None, len(rows), gone or None, times.ctypes.data if deleted else None,
            len(deleted), int(timestamp_ns), int(bool(aggregate)), ext or None, len(ext) // 32)
    rc = L.cdc_state_serialize_deleted(*args, None, 0, ctypes.byref(n))
    if rc == _lib.CDC_E_NOSPACE:
        out = ctypes.create_string_buffer(n.value)
        check(L.cdc_state_serialize_deleted(*args, out, n.value, ctypes.byref(n)), "cdc_state_serialize_deleted")
        return out.raw[:n.value]
    check(rc, "cdc_state_serialize_deleted")
    return b""


def delta_from_packfiles(packfiles, form="plain", key=None, compression="LZ4", timestamp_ns=0, extends=(), device=0):
    """The serialised delta state Snapshot.Commit would store (snapshot/
    snapshot.go:325-334) after PutPackfile entered these packfiles (snapshot.go:
    269-296): each packfile's checksum is the SHA-256 of its bytes, and every
    row of its index becomes SetPackfileForBlob(type, packfile, blob, offset,
    length).  form: how the packfiles are given ("plain": Serialize's form,
    "stored": the repository's, read with key and compression).  The result is
    plaintext: store it through Encode."""
    from . import restore, stored
    _lib.packfile_form_code(form)
    rows = []
    for p in packfiles:
        p = bytes(p)
        pack = hashlib.sha256(p).digest()
        if form == "stored":
            _, idx = stored.packfile_index_stored(p, key=key, compression=compression, device=device)
        else:
            _, idx = restore.packfile_index(p)
        rows.extend((typ, csum, pack, off, ln) for typ, csum, off, ln in idx)
    return serialize_rows(rows, timestamp_ns, aggregate=False, extends=extends)
