"""The LZ4 checker itself (tests/lz4_ref.py), on the CPU: it accepts what the
reference compressor (liblz4) writes and returns its bytes, and it rejects
hand-built blocks and frames that break one rule each, naming the rule."""
import pytest

import crypto_ref
import lz4_ref as lz
from datagen import low_entropy, random_bytes, text_like

MiB = 1 << 20


def _small(n):
    return [bytes(n), text_like(n, 3), random_bytes(n, 7).tobytes(), (b"abcdefg" * (n // 7 + 1))[:n]]


def _large():
    return {
        "zeros": bytes(MiB),
        "low": low_entropy(MiB, 11).tobytes(),
        "text": text_like(MiB, 12),
        "half": random_bytes(MiB // 2, 13).tobytes() + bytes(MiB // 2),
        "zeros+random": bytes(65536) + random_bytes(MiB - 65536, 14).tobytes(),
    }


@pytest.mark.parametrize("n", list(range(1, 20)) + list(range(8192, 8206)))
def test_walker_accepts_liblz4_small(n):
    for b in _small(n):
        data, seqs = lz.walk_block(lz.lz4_block_compress(b), len(b))
        assert data == b
        assert seqs[-1][1:] == (0, 0) and sum(s[0] + s[2] for s in seqs) == n
        assert lz.walk_block(lz.lz4_block_compress(b))[0] == b  # the length taken from the block itself


@pytest.mark.parametrize("kind", ["zeros", "low", "text", "half", "zeros+random"])
def test_walker_accepts_liblz4_1mib(kind):
    b = _large()[kind]
    enc = lz.lz4_block_compress(b)
    data, seqs = lz.walk_block(enc, len(b))
    assert data == b
    assert all(1 <= off and ml >= 4 for _, off, ml in seqs[:-1])
    if kind == "zeros":  # one overlapping match (offset 1) over the whole block
        assert len(seqs) == 2 and seqs[0][1] == 1 and seqs[0][2] > MiB - 32
    assert lz.ref_windowed_size(b) >= len(enc) - 16  # the 8-KiB window never compresses better (16: slack of headers)


def test_reference_sizes():
    """The figures the structure tests' savings condition rests on."""
    L = _large()
    assert lz.ref_windowed_size(L["zeros"]) == 128 * 43
    assert lz.ref_windowed_size(b"") == 0
    assert lz.lz4_block_size(random_bytes(8192, 1).tobytes()) > 8192
    # blocks of 4 MiB, then segments: a segment never spans two blocks
    b = bytes(4 * MiB + 100)
    assert lz.ref_windowed_size(b) == 512 * 43 + lz.lz4_block_size(bytes(100))


def _seq(lit, off=None, mlen=0, nib=None):
    """One encoded sequence; off None: literal-only (match nibble `nib`)."""
    def ext(x):
        out = b""
        if x >= 15:
            x -= 15
            out = b"\xff" * (x // 255) + bytes([x % 255])
        return out
    m = 0 if off is None else mlen - 4
    tok = min(len(lit), 15) << 4 | (min(m, 15) if nib is None else nib)
    out = bytes([tok]) + ext(len(lit)) + lit
    if off is not None:
        out += bytes([off & 255, off >> 8]) + ext(m)
    return out


LIT16 = b"abcdefghijklmnop"


def test_walker_decodes_handbuilt_and_overlaps():
    blk = _seq(b"abc", 3, 10) + _seq(b"XY", 1, 5) + _seq(b"0123456789ab")
    data, seqs = lz.walk_block(blk, 32)
    assert data == b"abc" + b"abcabcabca" + b"XY" + b"YYYYY" + b"0123456789ab"
    assert seqs == [(3, 3, 10), (2, 1, 5), (12, 0, 0)]
    long_lit = bytes(range(256)) * 5  # a literal length with 255-extensions
    blk = _seq(long_lit, 256, 300) + _seq(b"tail.")
    assert lz.walk_block(blk)[0] == long_lit + (long_lit[-256:] * 2)[:300] + b"tail."


@pytest.mark.parametrize("name,blk,n,rule", [
    ("offset 0", _seq(LIT16, 0, 4) + _seq(b"x" * 12), 32, lz.R_OFFSET_ZERO),
    ("offset before the block", _seq(b"abcd", 5, 4) + _seq(b"x" * 12), 20, lz.R_OFFSET_RANGE),
    ("match ends in the last 5", _seq(LIT16, 4, 8) + _seq(b"wxyz"), 28, lz.R_MATCH_END),
    ("match starts in the last 12", _seq(LIT16, 4, 4) + _seq(b"vwxyz"), 25, lz.R_MATCH_START),
    ("last sequence's match nibble", _seq(b"vwxyz", nib=3), 5, lz.R_LAST_NIBBLE),
    ("truncated length extension", b"\xf0\xff", None, lz.R_TRUNCATED),
    ("truncated literals", b"\x50abc", None, lz.R_TRUNCATED),
    ("truncated offset", _seq(LIT16, 4, 4)[:-1], None, lz.R_TRUNCATED),
    ("ends after a match", _seq(LIT16, 4, 4), None, lz.R_NO_LAST),
    ("short last literals", _seq(LIT16, 4, 4) + _seq(b"wxyz"), None, lz.R_MATCH_START),
    ("wrong decoded length", _seq(LIT16), 17, lz.R_OUT_LEN),
    ("literals past the length", _seq(LIT16), 12, lz.R_OUT_LEN),
])
def test_walker_rejects(name, blk, n, rule):
    with pytest.raises(ValueError, match="^" + rule):
        lz.walk_block(blk, n)


def test_last_literals_rule_alone():
    """A block whose only fault is a last run shorter than 5: a match that
    obeys both limits cannot be followed by fewer than 5 bytes, so the rule
    shows alone only on a literal-only block against a longer stated length."""
    with pytest.raises(ValueError, match="^" + lz.R_LAST_LITERALS):
        lz.walk_block(_seq(b"abcd"), 9)
    assert lz.walk_block(_seq(b"abcd"), 4) == (b"abcd", [(4, 0, 0)])  # min(5, decoded_len)
    assert lz.walk_block(b"\x00", 0) == (b"", [(0, 0, 0)])


def _frame(parts):
    """A frame of liblz4-compressed (or stored, when not smaller) blocks."""
    blocks = []
    for p in parts:
        c = lz.lz4_block_compress(p)
        blocks.append((False, c) if len(c) < len(p) else (True, p))
    return lz.frame_of(blocks, lz.xxh32(b"".join(parts)))


def test_frame_walker_accepts():
    parts = [bytes(4 * MiB), text_like(4 * MiB, 5), random_bytes(1000, 9).tobytes()]
    f = _frame(parts)
    blocks = lz.walk_frame(f)
    assert [b.stored for b in blocks] == [False, False, True]
    assert lz.content(blocks) == b"".join(parts) == crypto_ref.lz4f_decompress(f)
    assert blocks[0].size == len(lz.lz4_block_compress(parts[0])) and blocks[2].seqs == []
    assert lz.walk_frame(_frame([b"x"]))[0].data == b"x"


def test_frame_walker_rejects():
    good = _frame([bytes(100)])
    lz.walk_frame(good)

    def bad(frame, rule):
        with pytest.raises(ValueError, match="^" + rule):
            lz.walk_frame(frame)
    bad(b"\x05" + good[1:], lz.R_MAGIC)
    bad(good[:4] + b"\x60" + good[5:], lz.R_DESCRIPTOR)
    bad(good[:5] + b"\x40" + good[6:], lz.R_DESCRIPTOR)
    bad(good[:6] + bytes([good[6] ^ 1]) + good[7:], lz.R_HC)  # a wrong HC byte
    bad(good[:-1] + bytes([good[-1] ^ 0x80]), lz.R_CHECKSUM)
    bad(good + b"\0", lz.R_TRAILING)
    bad(good[:-4], lz.R_TRUNCATED)
    bad(good[:-9], lz.R_TRUNCATED)
    # a "compressed" block that is not smaller than its content
    lit = b"0123456789abcdefghij"
    bad(lz.frame_of([(False, _seq(lit))], lz.xxh32(lit)), lz.R_NOT_SMALLER)
    lz.walk_frame(lz.frame_of([(True, lit)], lz.xxh32(lit)))
    # a non-final block shorter than 4 MiB (stored, and compressed)
    bad(lz.frame_of([(True, lit), (True, lit)], lz.xxh32(lit + lit)), lz.R_SHORT_BLOCK)
    z = lz.lz4_block_compress(bytes(MiB))
    bad(lz.frame_of([(False, z), (True, lit)], lz.xxh32(bytes(MiB) + lit)), lz.R_SHORT_BLOCK)
    # a block above 4 MiB
    big = bytes(4 * MiB + 1)
    bad(lz.frame_of([(True, big)], lz.xxh32(big)), lz.R_BLOCK_SIZE)
    bad(lz.frame_of([(False, lz.lz4_block_compress(big))], lz.xxh32(big)), lz.R_BLOCK_SIZE)
    # a block rule inside a frame surfaces with its own name
    blk = _seq(LIT16 * 4, 4, 4) + _seq(b"vwxyz")
    bad(lz.frame_of([(False, blk)], 0), lz.R_MATCH_START)
