"""Test infrastructure: an independent, strict LZ4 checker for the device
Encode.  liblz4's decoder (crypto_ref.lz4f_decompress) proves that a frame is
decodable; this walker also proves that it is *well-formed* the way the LZ4
block format document asks of a compressor (the end-of-block rules, offsets
inside the block, a literal-only last sequence), returns the sequence list so
a test can assert which structures a frame really contains, and gives the
reference compressor's sizes (liblz4's LZ4_compress_default through ctypes)
to hold the kernel's ratio against.

Frame layout (LZ4 frame format 1.6.x) as the device writes it, pierrec/lz4
v4's defaults: magic 0x184D2204, FLG 0x64 (version 1, independent blocks,
content checksum), BD 0x70 (4-MiB blocks), HC, blocks (u32 size, bit 31 =
stored), end mark 0, XXH32 of the content."""
import ctypes
import struct
from collections import namedtuple

import crypto_ref

MAGIC = 0x184D2204
FLG, BD = 0x64, 0x70
BLOCK_MAX = 4 << 20   # BD 0x70
SEGMENT = 8192        # the device's match window (cdc_encode.hip kSegLZ)
MFLIMIT = 12          # a match starts at least this far before the block's end
LASTLITERALS = 5      # the block's last bytes are literals
MINMATCH = 4

# rule names: the text of the ValueError a violation raises starts with one
R_TRUNCATED = "truncated"
R_OFFSET_ZERO = "offset-zero"
R_OFFSET_RANGE = "offset-before-block-start"
R_MATCH_START = "match-start-within-last-12"
R_MATCH_END = "match-end-within-last-5"
R_LAST_NIBBLE = "last-sequence-match-nibble"
R_LAST_LITERALS = "last-literals-too-short"
R_NO_LAST = "no-final-literal-sequence"
R_OUT_LEN = "output-length"
R_NOT_SMALLER = "compressed-not-smaller"
R_MAGIC = "frame-magic"
R_DESCRIPTOR = "frame-descriptor"
R_HC = "frame-header-checksum"
R_BLOCK_SIZE = "block-size"
R_SHORT_BLOCK = "non-final-block-short"
R_END_MARK = "end-mark"
R_CHECKSUM = "content-checksum"
R_TRAILING = "trailing-bytes"

Block = namedtuple("Block", "stored size data seqs")


def _fail(rule, detail=""):
    raise ValueError(f"{rule}: {detail}" if detail else rule)


def _ext(data, ip, n):
    """The 255-extension bytes of a length whose nibble was 15."""
    end = len(data)
    while True:
        if ip >= end:
            _fail(R_TRUNCATED, "length extension runs off the block")
        b = data[ip]
        ip += 1
        n += b
        if b != 255:
            return n, ip


def walk_block(data, decoded_len=None):
    """Strict walk of one compressed LZ4 block: (decoded bytes, sequences).
    A sequence is (literal_len, offset, match_len); the last one is
    (literal_len, 0, 0).  decoded_len None: the block's own total (the frame
    does not carry it); the end-of-block rules are then checked against that.
    Any violation raises ValueError, its text starting with the rule's name.

    One pass (a 4-MiB block of text is ~500 K sequences).  Matches come in
    increasing position, so the two end-of-block limits hold for every match
    exactly when they hold for the last one: they are checked on it once the
    block's length is known."""
    data = bytes(data)
    n = len(data)
    out = bytearray()
    seqs = []
    add = seqs.append
    ip = 0
    mstart = mend = -1  # the last match
    while True:
        if ip >= n:
            _fail(R_NO_LAST, "the block ends after a match" if seqs else "empty block")
        tok = data[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            ll, ip = _ext(data, ip, ll)
        ie = ip + ll
        if ie > n:
            _fail(R_TRUNCATED, f"{ll} literals, {n - ip} bytes left")
        out += data[ip:ie]
        ip = ie
        if ip == n:  # input consumed exactly: this is the last sequence
            nib = tok & 15
            break
        if ip + 2 > n:
            _fail(R_TRUNCATED, "offset runs off the block")
        off = data[ip] | data[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            ml, ip = _ext(data, ip, ml)
        ml += MINMATCH
        pos = len(out)
        if off == 0:
            _fail(R_OFFSET_ZERO, f"at {pos}")
        if off > pos:  # blocks are independent: nothing before the block's start
            _fail(R_OFFSET_RANGE, f"offset {off} at {pos}")
        if off >= ml:
            out += out[pos - off:pos - off + ml]
        else:  # overlapping: the last `off` bytes repeat
            out += (bytes(out[pos - off:pos]) * (ml // off + 1))[:ml]
        mstart, mend = pos, pos + ml
        add((ll, off, ml))
    total = len(out)
    if decoded_len is None:
        decoded_len = total
    if mstart >= 0 and mstart + MFLIMIT > decoded_len:
        _fail(R_MATCH_START, f"match at {mstart} of {decoded_len}")
    if mend >= 0 and mend + LASTLITERALS > decoded_len:
        _fail(R_MATCH_END, f"match {mstart}..{mend} of {decoded_len}")
    if nib:
        _fail(R_LAST_NIBBLE, f"match nibble {nib} on the last sequence")
    if ll < min(LASTLITERALS, decoded_len):
        _fail(R_LAST_LITERALS, f"{ll} literals end a block of {decoded_len}")
    if total != decoded_len:
        _fail(R_OUT_LEN, f"{total} bytes decoded, {decoded_len} expected")
    add((ll, 0, 0))
    return bytes(out), seqs


def xxh32(b):
    import xxhash
    return xxhash.xxh32(bytes(b)).intdigest()


def walk_frame(frame):
    """Strict parse of one LZ4 frame as the device writes it: a list of
    Block(stored, size, data, seqs).  b"".join(block.data) is the content."""
    frame = bytes(frame)
    if len(frame) < 7 or struct.unpack_from("<I", frame, 0)[0] != MAGIC:
        _fail(R_MAGIC)
    if frame[4] != FLG or frame[5] != BD:
        _fail(R_DESCRIPTOR, f"FLG {frame[4]:#x} BD {frame[5]:#x}")
    if frame[6] != (xxh32(frame[4:6]) >> 8) & 0xFF:
        _fail(R_HC, f"{frame[6]:#x}")
    pos, blocks = 7, []
    while True:
        if pos + 4 > len(frame):
            _fail(R_TRUNCATED, "block header or end mark")
        (word,) = struct.unpack_from("<I", frame, pos)
        pos += 4
        if word == 0:
            break
        stored, size = bool(word >> 31), word & 0x7FFFFFFF
        if size == 0:
            _fail(R_END_MARK, "a stored block of no bytes")
        if size > BLOCK_MAX or pos + size > len(frame):
            _fail(R_BLOCK_SIZE if size > BLOCK_MAX else R_TRUNCATED, f"block of {size} at {pos}")
        body = frame[pos:pos + size]
        pos += size
        if blocks and len(blocks[-1].data) != BLOCK_MAX:
            _fail(R_SHORT_BLOCK, f"block {len(blocks) - 1} decodes to {len(blocks[-1].data)}")
        if stored:
            blocks.append(Block(True, size, body, []))
        else:
            data, seqs = walk_block(body)
            if not 1 <= len(data) <= BLOCK_MAX:
                _fail(R_BLOCK_SIZE, f"block {len(blocks)} decodes to {len(data)}")
            if size >= len(data):  # the device stores such a block raw (k_lz4_size)
                _fail(R_NOT_SMALLER, f"block {len(blocks)}: {size} for {len(data)}")
            blocks.append(Block(False, size, data, seqs))
    if pos + 4 > len(frame):
        _fail(R_TRUNCATED, "content checksum")
    (want,) = struct.unpack_from("<I", frame, pos)
    pos += 4
    content = b"".join(b.data for b in blocks)
    if want != xxh32(content):
        _fail(R_CHECKSUM, f"{want:#x}, content hashes to {xxh32(content):#x}")
    if pos != len(frame):
        _fail(R_TRAILING, f"{len(frame) - pos}")
    return blocks


def content(blocks):
    return b"".join(b.data for b in blocks)


_lz4c = None


def _lz4():
    global _lz4c
    if _lz4c is None:
        L = crypto_ref.lz4()
        L.LZ4_compressBound.argtypes = [ctypes.c_int]
        L.LZ4_compressBound.restype = ctypes.c_int
        L.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        L.LZ4_compress_default.restype = ctypes.c_int
        _lz4c = L
    return _lz4c


def lz4_block_compress(b):
    """liblz4's LZ4_compress_default of b: one block."""
    L = _lz4()
    b = bytes(b)
    cap = L.LZ4_compressBound(len(b))
    dst = ctypes.create_string_buffer(max(cap, 1))
    n = L.LZ4_compress_default(b, dst, len(b), cap)
    if n <= 0:
        raise ValueError("LZ4_compress_default failed")
    return dst.raw[:n]


def lz4_block_size(b):
    return len(lz4_block_compress(b))


def ref_windowed_size(b):
    """The reference compressor restricted to the device's match window: the
    sum over b's 4-MiB blocks and their 8-KiB segments of liblz4's size of the
    segment alone."""
    b = bytes(b)
    total = 0
    for k in range(0, len(b), BLOCK_MAX):
        blk = b[k:k + BLOCK_MAX]
        for s in range(0, len(blk), SEGMENT):
            total += lz4_block_size(blk[s:s + SEGMENT])
    return total


def frame_of(blocks, checksum=None, hc=None):
    """Assemble a frame from (stored, body) pairs (for the checker's own tests);
    checksum: the content's XXH32, given by the caller who knows the content."""
    out = struct.pack("<IBB", MAGIC, FLG, BD)
    out += bytes([(xxh32(bytes([FLG, BD])) >> 8) & 0xFF if hc is None else hc])
    for stored, body in blocks:
        out += struct.pack("<I", len(body) | (0x80000000 if stored else 0)) + bytes(body)
    return out + struct.pack("<II", 0, checksum or 0)
