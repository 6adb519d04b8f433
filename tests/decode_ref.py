"""Test infrastructure for the device Decode: fixtures made with the system's
liblz4 and libcrypto (through crypto_ref / lz4_ref), independent of this
repository's encoder, and the corruptions the GPU tests feed it.  The CPU test
runs every block below through tests/c/lz4d_host_fuzz.cpp (the same walker
under the sanitizers) before the GPU tests use them."""
import ctypes
import functools
import struct

import numpy as np

import crypto_ref
import lz4_ref

PIECE = 65536
BLOCK_FIXTURE_LEN = 68_640


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def block_fixture():
    """68,640 bytes that liblz4 turns into 4 sequences: a 40,960-byte literal
    run, a 20,480-byte match at offset 40,960, and the overlapping matches
    (offset 1, 4,999) and (offset 3, 2,097)."""
    r = rnd(40960, 1)
    c = r + r[:20480] + b"\x07" * 5000 + b"abc" * 700 + rnd(100, 2)
    assert len(c) == BLOCK_FIXTURE_LEN
    return c


@functools.lru_cache(None)
def offset_65535_content():
    r = rnd(65535, 3)
    return r + r[:4096]


def make_block(seqs, tail, seed):
    """A hand-made block of (literals, offset, match length) sequences and a
    final run of `tail` literals (fresh random bytes): (block, content)."""
    rng = np.random.default_rng(seed)
    o, content = bytearray(), bytearray()

    def ext(v):
        v -= 15
        while v >= 255:
            o.append(255)
            v -= 255
        o.append(v)

    def lits(n):
        b = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        o.extend(b)
        content.extend(b)

    for ll, off, ml in seqs:
        m = ml - 4
        o.append(min(ll, 15) << 4 | min(m, 15))
        if ll >= 15:
            ext(ll)
        lits(ll)
        o.extend(struct.pack("<H", off))
        if m >= 15:
            ext(m)
        pos = len(content)
        for i in range(ml):
            content.append(content[pos - off + i % off])
    o.append(min(tail, 15) << 4)
    if tail >= 15:
        ext(tail)
    lits(tail)
    return bytes(o), bytes(content)


@functools.lru_cache(None)
def ext_blocks():
    """Length extensions that end in a 0 byte or take a full 255 step: literal
    runs of 15 and 270, matches of 19 and 274."""
    return [make_block([(15, 7, 19), (270, 100, 274), (0, 1, 19), (3, 2, 274)], 15, 4),
            make_block([(270, 270, 4), (15, 15, 18), (14, 1, 273)], 270, 5)]


class _FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class _Prefs(ctypes.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def lz4f_compress(data, block_id=7, independent=True, content_checksum=True, block_checksum=False,
                  content_size=False):
    """liblz4's LZ4F_compressFrame."""
    L = crypto_ref.lz4()
    L.LZ4F_compressFrameBound.restype = ctypes.c_size_t
    L.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_compressFrame.restype = ctypes.c_size_t
    L.LZ4F_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.c_void_p]
    p = _Prefs()
    p.frameInfo.blockSizeID = block_id
    p.frameInfo.blockMode = 1 if independent else 0
    p.frameInfo.contentChecksumFlag = int(content_checksum)
    p.frameInfo.blockChecksumFlag = int(block_checksum)
    p.frameInfo.contentSize = len(data) if content_size else 0
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, bytes(data), len(data), ctypes.byref(p))
    assert not L.LZ4F_isError(n)
    return dst.raw[:n]


def frame_of_blocks(blocks, content):
    """lz4_ref.frame_of with the content's checksum."""
    return lz4_ref.frame_of(blocks, checksum=lz4_ref.xxh32(content))


@functools.lru_cache(None)
def fixture_frames():
    """name -> (frame, content or None for a frame Decode must refuse as unsupported)."""
    c4 = block_fixture() * 4
    out = {}
    out["lz4f-0x64"] = (lz4f_compress(c4), c4)
    out["lz4f-0x7c"] = (lz4f_compress(c4, block_id=4, block_checksum=True, content_size=True), c4)
    out["lz4f-linked"] = (lz4f_compress(c4, block_id=4, independent=False, content_checksum=False), None)
    assert out["lz4f-0x64"][0][4] == 0x64  # liblz4 picks the block maximum that fits the content (BD 0x60)
    assert out["lz4f-0x7c"][0][4:6] == b"\x7c\x40"
    assert out["lz4f-linked"][0][4] == 0x40
    tile = rnd(60_000, 6)
    big = (tile * 70)[:4 << 20]
    out["two-blocks"] = (frame_of_blocks([(False, lz4_ref.lz4_block_compress(big)),
                                          (False, lz4_ref.lz4_block_compress(b"x"))], big + b"x"), big + b"x")
    a, b, c = block_fixture(), rnd(3000, 7), offset_65535_content()
    out["mixed"] = (frame_of_blocks([(False, lz4_ref.lz4_block_compress(a)), (True, b),
                                     (False, lz4_ref.lz4_block_compress(c)), (True, b"z")], a + b + c + b"z"),
                    a + b + c + b"z")
    out["empty"] = (frame_of_blocks([], b""), b"")
    assert len(out["empty"][0]) == 15
    for i, (blk, content) in enumerate(ext_blocks()):
        out[f"ext-{i}"] = (frame_of_blocks([(False, blk)], content), content)
    many = [rnd(40, 100 + i) for i in range(300)]  # many short blocks
    out["many-blocks"] = (frame_of_blocks([(i % 2 == 0, m) if i % 2 == 0 else (False, lz4_ref.lz4_block_compress(m))
                                           for i, m in enumerate(many)], b"".join(many)), b"".join(many))
    return out


def seal_stream(key, plain, seed, piece=PIECE):
    """encryption.EncryptStream with libcrypto and random nonces: subkey nonce
    || Seal(key, nonce, subkey), then nonce || Seal(subkey, nonce, piece) for
    every 64-KiB piece."""
    rng = np.random.default_rng(seed)

    def r(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    sub, n0 = r(32), r(12)
    out = bytearray(n0 + crypto_ref.gcm_seal(key, n0, sub))
    for p in range(0, len(plain), piece):
        n = r(12)
        out += n + crypto_ref.gcm_seal(sub, n, plain[p:p + piece])
    return bytes(out)


def flip(b, at, bit=0):
    b = bytearray(b)
    b[at] ^= 1 << bit
    return bytes(b)


def bad_block(kind):
    """A block with one invalid offset, and nothing else wrong."""
    blk, _ = make_block([(10, 7, 30), (10, 12, 8)], 12, 8)
    b = bytearray(blk)
    assert b[0] == 0xAF and b[11:13] == b"\x07\x00"  # token, 10 literals, the first offset
    if kind == "offset-zero":
        b[11:13] = struct.pack("<H", 0)
    else:  # the first match reaches one byte before the block's start
        b[11:13] = struct.pack("<H", 11)
    return bytes(b)


def corrupt_frames():
    """name -> a frame Decode must report as CDC_E_CORRUPT."""
    f, _ = fixture_frames()["lz4f-0x64"]
    out = {"truncated-by-one": f[:-1], "bad-magic": flip(f, 1), "bad-hc": flip(f, 6),
           "bad-content-checksum": flip(f, len(f) - 2)}
    (size,) = struct.unpack_from("<I", f, 7)
    out["block-size-past-frame"] = f[:7] + struct.pack("<I", size + 4096) + f[11:]
    for kind in ("offset-zero", "offset-before-start"):
        out[kind] = lz4_ref.frame_of([(False, bad_block(kind))], checksum=1)
    return out


def mutated_frames(n=64, seed=9):
    """n fixed-seed mutations of the FLG 0x7c frame: bit flips, a truncation
    or a length-field edit each."""
    f, _ = fixture_frames()["lz4f-0x7c"]
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = bytearray(f)
        how = i % 4
        if how == 0:
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif how == 1:
            del b[int(rng.integers(0, len(b))):]
        elif how == 2:  # a byte near the frame's start: header, first block size, first tokens
            b[int(rng.integers(0, 40))] = int(rng.choice([0, 0x0F, 0xF0, 0xFF]))
        else:
            b[int(rng.integers(0, len(b)))] = int(rng.choice([0, 255]))
        out.append(bytes(b))
    return out


def lenient_blocks(frame):
    """The compressed block bodies of a (possibly damaged) frame, as far as
    its block headers can be followed."""
    out = []
    if len(frame) < 7:
        return out
    flg = frame[4]
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    while pos + 4 <= len(frame):
        (w,) = struct.unpack_from("<I", frame, pos)
        pos += 4
        size = w & 0x7FFFFFFF
        if w == 0 or size > (4 << 20) or pos + size > len(frame):
            break
        if not w >> 31:
            out.append(frame[pos:pos + size])
        pos += size + (4 if flg & 16 else 0)
    return out


def all_blocks():
    """Every compressed block the GPU tests decode, valid or not."""
    out = [lz4_ref.lz4_block_compress(block_fixture()), lz4_ref.lz4_block_compress(offset_65535_content())]
    out += [b for b, _ in ext_blocks()]
    out += [bad_block("offset-zero"), bad_block("offset-before-start")]
    for f, _ in fixture_frames().values():
        out += lenient_blocks(f)
    for f in list(corrupt_frames().values()) + mutated_frames():
        out += lenient_blocks(f)
    return out
