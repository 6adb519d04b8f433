"""Decode on the device: plakar's (*Repository).Decode (repository/repository.go:
186-210) for a batch of blobs -- encryption.DecryptStream (encryption/
symmetric.go:165-243) when a key is configured, then compression.
InflateLZ4Stream or InflateGzipStream (compression/compression.go:130-160) --
and the blob check of snapshot/check.go:83-98 (decode, SHA-256, compare) with
the plaintext staying on the device; decode_prefix is Decode for the first
bytes of each blob, which is what a reader of a byte range needs.  Every call
goes through the C ABI (cdc_decode_device, cdc_decode_prefix_device,
cdc_check_device)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import CdcError, check, ensure_init, lib


class DecodeError(CdcError):
    """One blob's failure: CDC_E_AUTH, CDC_E_CORRUPT or CDC_E_UNSUPPORTED in .status."""


def _key(key):
    if key is None:
        return None
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("the repository key is 32 bytes (AES-256)")
    return key


def _u64(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1))
    if a.size != n:
        raise ValueError("offsets and lens differ in length")
    return a


def _sel(compressed):
    """The C selector: False / True (the LZ4 frame) or the string "GZIP"."""
    if isinstance(compressed, str):
        return _lib.compress_code(compressed)
    return int(bool(compressed))


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype)) if a.size else (ctype * 1)()


def decode_device(base, offsets, lens, out, key=None, compressed=True, device=0, stream=None):
    """Decode the encoded blobs that live in the device tensor `base` (uint8)
    at the given byte offsets/lengths into the device tensor `out`: returns
    (out_offsets, status), n + 1 int64 offsets and n int32 codes.  Blob i's
    plaintext is out[out_offsets[i]:out_offsets[i + 1]]; a failed blob has
    status[i] != 0 and no bytes.  Raises CdcError(CDC_E_NOSPACE) when `out` is
    too small (.needed: the bytes to retry with).  `compressed`: False, True
    (an LZ4 frame) or "GZIP" (a gzip member)."""
    import torch
    ensure_init()
    n = len(lens)
    offs_a, lens_a = _u64(offsets, n), _u64(lens, n)
    oo_a = np.zeros(n + 1, dtype=np.uint64)
    st_a = np.zeros(n, dtype=np.int32)
    s = stream if stream is not None else torch.cuda.current_stream(device)
    rc = lib().cdc_decode_device(int(device), ctypes.c_void_p(base.data_ptr()), _ptr(offs_a, ctypes.c_uint64),
                                 _ptr(lens_a, ctypes.c_uint64), n, _sel(compressed), _key(key),
                                 ctypes.c_void_p(out.data_ptr()), out.numel(), _ptr(oo_a, ctypes.c_uint64),
                                 _ptr(st_a, ctypes.c_int32), ctypes.c_void_p(s.cuda_stream))
    if rc < 0:
        err = CdcError(rc, "cdc_decode_device")
        err.needed = int(oo_a[n]) if rc == _lib.CDC_E_NOSPACE else None
        raise err
    return oo_a.astype(np.int64), st_a


def _upload(blobs, device):
    import torch
    arrs = [np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview))
            else np.asarray(b, np.uint8).ravel() for b in blobs]
    lens = np.array([a.size for a in arrs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.empty(max(int(offs[-1]), 1), dtype=torch.uint8, device=torch.device("cuda", device))
    if int(offs[-1]):
        base[:int(offs[-1])].copy_(torch.from_numpy(np.concatenate(arrs)))
    return base, offs[:-1], lens


def decode_blobs(blobs, key=None, compressed=True, device=0):
    """Decode host byte buffers: a list with each blob's plaintext (bytes), or
    a DecodeError in the place of a blob that did not decode.  `compressed`
    as for decode_device."""
    import torch
    if not len(blobs):
        return []
    base, offs, lens = _upload(blobs, device)
    # decoded sizes are not stored in the blobs: a first guess, then the size the call reports
    cap = max(int(lens.sum()) * (4 if compressed else 1), 1 << 16)
    while True:
        out = torch.empty(cap, dtype=torch.uint8, device=base.device)
        try:
            oo, st = decode_device(base, offs, lens, out, key=key, compressed=compressed, device=device)
            break
        except CdcError as e:
            if e.status != _lib.CDC_E_NOSPACE or e.needed <= cap:
                raise
            cap = e.needed
    host = out[:int(oo[-1])].cpu().numpy()
    return [DecodeError(int(st[i]), f"blob {i}") if st[i] else host[oo[i]:oo[i + 1]].tobytes()
            for i in range(len(blobs))]


def decode_prefix_device(base, offsets, lens, upto, out, key=None, compressed=True, device=0, stream=None):
    """cdc_decode_prefix_device: the first upto[i] plaintext bytes of the
    encoded blob i of the device tensor `base` into the device tensor `out`,
    at out_offsets[i], the exclusive sum of `upto` (the sizes are an input:
    nothing is sized on the device).  Returns (out_offsets, status).  A walk
    stops at upto[i] and validates nothing after it; one that reaches the
    stream's end verifies what decode_device verifies.  A stream that ends
    before upto[i] is CDC_E_MISMATCH.  Nothing at or beyond out_offsets[n] is
    written.  Raises CdcError(CDC_E_NOSPACE) when `out` is smaller than that."""
    import torch
    ensure_init()
    n = len(lens)
    offs_a, lens_a = _u64(offsets, n), _u64(lens, n)
    upto_a = np.ascontiguousarray(np.asarray(upto, dtype=np.uint64).reshape(-1))
    if upto_a.size != n:
        raise ValueError("one upto per blob")
    oo_a = np.zeros(n + 1, dtype=np.uint64)
    st_a = np.zeros(n, dtype=np.int32)
    s = stream if stream is not None else torch.cuda.current_stream(device)
    rc = lib().cdc_decode_prefix_device(int(device), ctypes.c_void_p(base.data_ptr()), _ptr(offs_a, ctypes.c_uint64),
                                        _ptr(lens_a, ctypes.c_uint64), _ptr(upto_a, ctypes.c_uint64), n,
                                        _sel(compressed), _key(key), ctypes.c_void_p(out.data_ptr()), out.numel(),
                                        _ptr(oo_a, ctypes.c_uint64), _ptr(st_a, ctypes.c_int32),
                                        ctypes.c_void_p(s.cuda_stream))
    if rc < 0:
        err = CdcError(rc, "cdc_decode_prefix_device")
        err.needed = int(oo_a[n]) if rc == _lib.CDC_E_NOSPACE else None
        raise err
    return oo_a.astype(np.int64), st_a


def _upto(upto, n):
    vals = [int(u) for u in upto]
    if len(vals) != n:
        raise ValueError("one upto per blob")
    if any(u < 0 for u in vals):
        raise ValueError("upto is a byte count: not negative")
    return np.array(vals, dtype=np.uint64)


def decode_prefix(blobs, upto, key=None, compression="LZ4", device=0):
    """The first upto[i] plaintext bytes of each encoded blob (host byte
    buffers): a list of bytes, a DecodeError in the place of a blob that did
    not decode.  `compression`: "LZ4", "GZIP" or None, as DeviceDecoder's."""
    import torch
    code = _lib.compress_code(compression)
    key = _key(key)
    upto_a = _upto(upto, len(blobs))
    if not len(blobs):
        return []
    base, offs, lens = _upload(blobs, device)
    out = torch.empty(max(int(upto_a.sum()), 1), dtype=torch.uint8, device=base.device)
    compressed = "GZIP" if code == _lib.CDC_COMPRESS_GZIP else bool(code)
    oo, st = decode_prefix_device(base, offs, lens, upto_a, out, key=key, compressed=compressed, device=device)
    host = out[:int(oo[-1])].cpu().numpy()
    return [DecodeError(int(st[i]), f"blob {i}") if st[i] else host[oo[i]:oo[i + 1]].tobytes()
            for i in range(len(blobs))]


def check_blobs(blobs, checksums, key=None, compressed=True, device=0):
    """snapshot/check.go:83-98 for a batch: decode each blob, hash it and
    compare with its 32-byte checksum, all on the device.  Returns the int32
    status array: 0, CDC_E_MISMATCH, or the blob's decode error."""
    import torch
    n = len(blobs)
    if len(checksums) != n:
        raise ValueError("one checksum per blob")
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    want = b"".join(bytes(c) for c in checksums)
    if len(want) != 32 * n:
        raise ValueError("a checksum is 32 bytes (SHA-256)")
    ensure_init()
    base, offs, lens = _upload(blobs, device)
    st_a = np.zeros(n, dtype=np.int32)
    needed = ctypes.c_uint64()
    s = torch.cuda.current_stream(device)
    cap = max(int(lens.sum()) * (4 if compressed else 1), 1 << 16)
    while True:
        scratch = torch.empty(cap, dtype=torch.uint8, device=base.device)
        rc = lib().cdc_check_device(int(device), ctypes.c_void_p(base.data_ptr()), _ptr(offs, ctypes.c_uint64),
                                    _ptr(lens, ctypes.c_uint64), n, _sel(compressed), _key(key), want,
                                    ctypes.c_void_p(scratch.data_ptr()), cap, ctypes.byref(needed),
                                    _ptr(st_a, ctypes.c_int32), ctypes.c_void_p(s.cuda_stream))
        if rc == _lib.CDC_E_NOSPACE and needed.value > cap:
            cap = needed.value
            continue
        check(rc, "cdc_check_device")
        return st_a


class DeviceDecoder:
    """(*Repository).Decode with the repository's configuration, the
    counterpart of DeviceEncoder: compression "LZ4", "GZIP" or None, and the
    encryption key (None: not encrypted).  `decode_many` decodes a batch in
    one device call, `decode_prefix_many` only each blob's first bytes,
    `check_many` verifies a batch against its checksums;
    calling the object decodes one blob, like Decode (and raises its error)."""

    def __init__(self, key=None, compression="LZ4", device=0):
        code = _lib.compress_code(compression)
        self.key = _key(key)
        self.compressed = "GZIP" if code == _lib.CDC_COMPRESS_GZIP else bool(code)
        self.device = device

    def decode_many(self, blobs):
        return decode_blobs(blobs, key=self.key, compressed=self.compressed, device=self.device)

    def decode_prefix_many(self, blobs, upto):
        return decode_prefix(blobs, upto, key=self.key,
                             compression="GZIP" if self.compressed == "GZIP" else "LZ4" if self.compressed else None,
                             device=self.device)

    def check_many(self, blobs, checksums):
        return check_blobs(blobs, checksums, key=self.key, compressed=self.compressed, device=self.device)

    def __call__(self, blob):
        r = self.decode_many([blob])[0]
        if isinstance(r, DecodeError):
            raise r
        return r
