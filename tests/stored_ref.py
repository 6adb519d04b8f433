"""The stored packfile form with system libraries only (TEST INFRASTRUCTURE:
the independent writer and reader for libplakar_cdc.so's stored-form entry
points; nothing here calls the library).

  writer  packfile_ref.put_packfile_layout (snapshot/snapshot.go:249-267) with
          Encode = compression (liblz4's frame with pierrec/lz4's options, or
          Python's gzip), then encryption.EncryptStream over libcrypto
          (decode_ref.seal_stream);
  reader  cmd/plakar/subcommands/info/info.go:387-426 restated: the last byte
          is the encoded footer's length, the four before it the version, the
          footer decodes to 52 bytes and names the index offset, the index
          decodes to 41-byte rows whose SHA-256 is the footer's.
"""
import gzip
import hashlib
import struct

import crypto_ref
import decode_ref
import packfile_ref as pf

CONFIGS = [(c, k) for c in (None, "LZ4", "GZIP") for k in (False, True)]
KEY = bytes(range(32))
KEY_B = bytes(range(100, 132))


def config_id(cfg):
    return f"{cfg[0] or 'NONE'}-{'key' if cfg[1] else 'nokey'}"


def compress(data, compression):
    """compression.DeflateStream: an empty input is an empty stream (compression.go:58-62)."""
    if compression is None or len(data) == 0:
        return bytes(data)
    if compression == "LZ4":
        return decode_ref.lz4f_compress(data)  # 4-MiB independent blocks, content checksum: pierrec's defaults
    return gzip.compress(bytes(data), compresslevel=6, mtime=0)


def inflate(data, compression):
    if compression is None or len(data) == 0:
        return bytes(data)
    if compression == "LZ4":
        return crypto_ref.lz4f_decompress(data)
    return gzip.decompress(data)


def encoder(compression, key, seed=1):
    """Encode of repository.go:212-262 as a function of the plaintext; every call draws other nonces."""
    n = [seed * 1000]

    def encode(plain):
        body = compress(plain, compression)
        if key is None:
            return body
        n[0] += 1
        return decode_ref.seal_stream(key, body, n[0])
    return encode


def decode(data, compression, key):
    if key is not None:
        data, _, _ = crypto_ref.decrypt_stream(key, data)
    return inflate(data, compression)


def write(p, compression, key, seed=1):
    """The bytes PutPackfile stores for the packfile_ref.PackFile p."""
    return pf.put_packfile_layout(p, encoder(compression, key, seed))


def read(stored, compression, key):
    """info.go:387-426: (PackFile, encoded index, encoded footer).  Raises ValueError / AssertionError
    for a malformed file."""
    total = len(stored)
    flen = stored[-1]
    version = struct.unpack("<I", stored[-5:-1])[0]
    assert version == pf.VERSION, version
    enc_footer = stored[total - 5 - flen:total - 5]
    assert len(enc_footer) == flen
    footer = decode(enc_footer, compression, key)
    assert len(footer) == 52, len(footer)
    fversion, ts, count, index_offset, csum = struct.unpack("<IqII32s", footer)
    assert fversion == version
    enc_index = stored[index_offset:total - 5 - flen]
    index = decode(enc_index, compression, key)
    assert len(index) == 41 * count, (len(index), count)
    if hashlib.sha256(index).digest() != csum:
        raise ValueError("index checksum mismatch")
    p = pf.PackFile(ts)
    p.version, p.count, p.index_offset, p.index_checksum = fversion, count, index_offset, csum
    p.blobs = bytearray(stored[:index_offset])
    for k in range(0, len(index), 41):
        t, c, o, n = struct.unpack("<B32sII", index[k:k + 41])
        if o + n > index_offset:
            raise ValueError("chunk offset + chunk length exceeds total length of packfile")
        p.index.append((t, c, o, n))
    return p, enc_index, enc_footer


def small_packfile(seed=0, timestamp=1234567):
    """3 rows: a zero-length blob, a TYPE_OBJECT row, a chunk."""
    rng = decode_ref.rnd
    p = pf.PackFile(timestamp)
    p.add_blob(pf.TYPE_CHUNK, hashlib.sha256(b"").digest(), b"")
    obj = rng(77, seed + 1)
    p.add_blob(3, hashlib.sha256(obj).digest(), obj)  # packfile.TYPE_OBJECT
    chunk = rng(5000, seed + 2)
    p.add_blob(pf.TYPE_CHUNK, hashlib.sha256(chunk).digest(), chunk)
    return p


def wide_packfile(seed=0, timestamp=-5, rows=1600):
    """1,600 one-byte blobs: a 65,600-byte index, the smallest whose encoding without compression takes a
    second GCM record (LZ4 and GZIP shrink the offsets and lengths to about 59 KB: one record; 2,000 rows
    take two under either)."""
    p = pf.PackFile(timestamp)
    body = decode_ref.rnd(rows, seed + 3)
    for i in range(rows):
        p.add_blob(pf.TYPE_CHUNK, hashlib.sha256(struct.pack("<II", seed, i)).digest(), body[i:i + 1])
    return p
