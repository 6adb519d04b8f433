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


def serialize_rows(rows, timestamp_ns, aggregate=False, extends=()):
    """cdc_state_serialize: SerializeStream of a state holding `rows`, an
    iterable of (type, blob checksum, packfile checksum, offset, length),
    entered in order with SetPackfileForBlob.  Host only."""
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
    n = ctypes.c_uint64()
    L = lib()
    args = (arr.ctypes.data if len(rows) else None, len(rows), int(timestamp_ns), int(bool(aggregate)), ext or None,
            len(ext) // 32)
    rc = L.cdc_state_serialize(*args, None, 0, ctypes.byref(n))
    if rc == _lib.CDC_E_NOSPACE:
        out = ctypes.create_string_buffer(n.value)
        check(L.cdc_state_serialize(*args, out, n.value, ctypes.byref(n)), "cdc_state_serialize")
        return out.raw[:n.value]
    check(rc, "cdc_state_serialize")
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
