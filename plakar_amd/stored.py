"""The stored packfile form: what a repository keeps.

snapshot.PutPackfile (snapshot/snapshot.go:232-267) stores

    data || Encode(index) || Encode(footer) || u32le version || u8 len(Encode(footer))

with Encode the repository's compression and AES-256-GCM stream.  The sessions
that read packfiles (restore, check, diff, archive, sync) register any number of
them in one cdc_*_add_packfiles call, which decodes all their footers and all
their indexes in two device calls; the writers (backup, sync) hand on_pack the
stored bytes when asked to.  Everything here goes through the C ABI."""
import ctypes
import os

from . import _lib
from ._lib import check, lib


def _keybuf(key):
    if key is None:
        return None
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("the repository key is 32 bytes (AES-256)")
    return key


def packfile_index_stored(data, key=None, compression="LZ4", device=0):
    """cdc_packfile_index_stored: (footer, rows) of one stored packfile, as
    restore.packfile_index returns them for the plain form.  Raises
    CdcError(CDC_E_CORRUPT) for a malformed packfile and CdcError(CDC_E_AUTH)
    for a GCM tag of the footer or the index that does not verify."""
    data = bytes(data)
    code = _lib.compress_code(compression)
    key = _keybuf(key)
    L = lib()
    f = _lib.cdc_packfile_footer()
    need = ctypes.c_uint64()
    rc = L.cdc_packfile_index_stored(int(device), data, len(data), code, key, ctypes.byref(f), None, 0,
                                     ctypes.byref(need))
    rows = None
    if rc == _lib.CDC_E_NOSPACE:
        rows = (_lib.cdc_packfile_row * need.value)()
        rc = L.cdc_packfile_index_stored(int(device), data, len(data), code, key, ctypes.byref(f), rows, need.value,
                                         ctypes.byref(need))
    check(rc, "cdc_packfile_index_stored")
    footer = dict(version=int(f.version), timestamp=int(f.timestamp), count=int(f.count),
                  index_offset=int(f.index_offset), index_checksum=bytes(f.index_checksum))
    return footer, [(int(r.type), bytes(r.checksum), int(r.offset), int(r.length)) for r in (rows or [])]


def sources(packfiles, form="plain", rows=None):
    """The cdc_packfile_src array of `packfiles` (bytes and/or paths) and what
    must outlive its use: (array, n, buffers the context reads from later,
    buffers only the call needs).  rows: one list of (type, checksum, offset,
    length) per packfile, which then comes with CDC_PACKFILE_ROWS."""
    if rows is None:
        code = _lib.packfile_form_code(form)
    else:
        code = _lib.PACKFILE_ROWS
        if len(rows) != len(packfiles):
            raise ValueError("rows: one list per packfile")
    n = len(packfiles)
    arr = (_lib.cdc_packfile_src * max(n, 1))()
    keep, temp = [], []
    for i, p in enumerate(packfiles):
        if isinstance(p, (str, os.PathLike)):
            arr[i].path = os.fsencode(p)
        else:
            buf = bytes(p)
            cbuf = ctypes.create_string_buffer(buf, max(len(buf), 1))
            keep.append(cbuf)
            arr[i].bytes = ctypes.cast(cbuf, ctypes.c_void_p)
            arr[i].len = len(buf)
        arr[i].form = code
        if rows is not None:
            r = (_lib.cdc_packfile_row * max(len(rows[i]), 1))()
            for k, (typ, csum, off, length) in enumerate(rows[i]):
                csum = bytes(csum)
                if len(csum) != 32:
                    raise ValueError("a row's checksum is 32 bytes (SHA-256)")
                r[k].type, r[k].offset, r[k].length = int(typ), int(off), int(length)
                ctypes.memmove(r[k].checksum, csum, 32)
            temp.append(r)
            arr[i].rows = r
            arr[i].nrows = len(rows[i])
    return arr, n, keep, temp


def add_packfiles(fn_name, handle, keep, packfiles, form="plain", rows=None):
    """One cdc_*_add_packfiles call (fn_name) on a session's handle; the memory
    sources' buffers are appended to the session's `keep`.  Returns the list of
    per-source statuses (0, or a negative CDC_E_* code; only sources with 0
    were entered)."""
    packfiles = list(packfiles)
    arr, n, bufs, temp = sources(packfiles, form, rows)
    status = (ctypes.c_int32 * max(n, 1))()
    check(getattr(lib(), fn_name)(handle, arr, n, status), fn_name)
    keep.extend(bufs)
    del temp
    return [int(status[i]) for i in range(n)]


def add_all(session, packfiles, packfile_form="plain"):
    """What the one-shot helpers do with their packfiles: the plain form one by
    one as before, another form in one call, raising on the first source that
    was not entered."""
    if packfile_form == "plain":
        for p in packfiles:
            session.add_packfile(p)
        return
    for st in session.add_packfiles(packfiles, form=packfile_form):
        check(st, "add_packfiles")
