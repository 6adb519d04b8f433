"""GZIP Encode where its kernels change behaviour with size, against zlib,
crypto_ref and inflate_ref: members of 64, 65 and 257 spans whose CRC-32 is
combined from non-zero span registers in every lane and on every trip of
k_gz_fin's loop, text, random and mixed content across the 4-MiB block
boundary (and exactly on it), sealed pieces that end on a stored member's
edge, the block choice held to the exact bit counts of the three forms, and
seeded random batches."""
import functools
import hashlib
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import inflate_ref as ir  # noqa: E402
from datagen import low_entropy, random_bytes  # noqa: E402
from plakar_amd import decode, encode  # noqa: E402
from test_encode_gzip import HEADER, KEY, SEG, SPAN, _alternating, _encode, _period7, _trailer  # noqa: E402

pytestmark = pytest.mark.gpu

MIB = 1 << 20
PIECE = 65536
WALK_BUDGET = 2 * MIB  # the Python walker reads about 1.5 s per MiB


def _hold(members, contents, what=""):
    """Every member against the references: the ten header bytes, zlib, the
    trailer, the bound.  An empty blob is an empty stream."""
    for i, (m, c) in enumerate(zip(members, contents)):
        tag = f"{what} blob {i} ({len(c)} bytes)"
        if not c:
            assert m == b"", f"{tag}: an empty blob is an empty stream"
            continue
        assert m[:10] == HEADER, f"{tag}: header"
        assert zlib.decompress(m, 31) == c, f"{tag}: zlib"
        assert _trailer(m) == (zlib.crc32(c), len(c)), f"{tag}: trailer"
        assert len(m) <= encode.encode_bound(len(c), "GZIP", False), f"{tag}: bound"


def _open(sealed, contents, what=""):
    """The members inside sealed outputs, each held to its length first: the
    60-byte header and 28 bytes per 64-KiB piece of the member."""
    members = []
    for i, (s, c) in enumerate(zip(sealed, contents)):
        m = crypto_ref.decrypt_stream(KEY, s)[0]
        assert len(s) == 60 + len(m) + 28 * (-(-len(m) // PIECE)), f"{what} blob {i} ({len(c)} bytes): sealed length"
        assert len(s) <= encode.encode_bound(len(c), "GZIP", True), f"{what} blob {i} ({len(c)} bytes): sealed bound"
        members.append(m)
    return members


def _splice(t, r, n):
    """Whole spans of t and of r in turn, n bytes."""
    a = np.frombuffer(t, dtype=np.uint8)[:n].copy()
    rr = np.frombuffer(r, dtype=np.uint8)
    for s in range(SPAN, n, 2 * SPAN):
        a[s:s + SPAN] = rr[s:min(s + SPAN, n)]
    return a.tobytes()


# ---- A1: large members -------------------------------------------------------------------
LENGTHS = [2 * MIB - 1, 2 * MIB, 2 * MIB + 1,       # 64 spans, 64, 65
           4 * MIB - 1, 4 * MIB, 4 * MIB + 1,       # one block, one full block, a second block of one byte
           4 * MIB + SPAN + 7,                      # 130 spans
           8 * MIB, 8 * MIB + 3]                    # two full blocks; 257 spans in three
KINDS = ("text", "random", "alternating")
# zeros with one other byte: (length, the span it lies in, its place in the span).  One span
# register is non-zero, so its place in the fold decides the CRC-32: lane 0, lane 63, the
# second trip's lane 0 (which is also a last span of one byte), the third trip, the fifth
ONES = [(2 * MIB + 1, 0, 12345), (2 * MIB + 1, 63, SPAN - 1), (2 * MIB + 1, 64, 0), (4 * MIB + SPAN + 7, 128, 129),
        (8 * MIB + 3, 256, 1)]


@functools.lru_cache(None)
def _large():
    """[(kind, length, content)]: every length once, the kinds in turn; three
    lengths with a second kind; the zeros.  About 66 MiB."""
    n = LENGTHS[-1]
    t, r = ir.text(n, 901), ir.rnd(n, 902)
    make = {"text": lambda n: t[:n], "random": lambda n: r[:n], "alternating": lambda n: _splice(t, r, n)}
    out = [(KINDS[j % 3], n, make[KINDS[j % 3]](n)) for j, n in enumerate(LENGTHS)]
    for j in (2, 4, 6):             # 2 MiB + 1 random, 4 MiB text, 4 MiB + 32,775 alternating
        k = KINDS[(j + 2) % 3]
        out.append((k, LENGTHS[j], make[k](LENGTHS[j])[::-1] if k != "alternating" else _splice(r, t, LENGTHS[j])))
    for n, span, at in ONES:
        z = bytearray(n)
        assert span == (n - 1) // SPAN or span < (n - 1) // SPAN and at < SPAN
        z[span * SPAN + at] = 0xA7
        out.append((f"one-in-span-{span}", n, bytes(z)))
    for kind in KINDS:
        assert any(n > 4 * MIB for k, n, _ in out if k == kind), f"no {kind} crosses the block boundary"
    assert 60 * MIB < sum(n for _, n, _ in out) < 70 * MIB
    return out


@pytest.mark.parametrize("sealed", [False, True], ids=["plain", "sealed"])
def test_large_members(sealed):
    batch = _large()
    contents = [c for _, _, c in batch]
    enc, _ = _encode(contents, key=KEY if sealed else None)
    members = _open(enc, contents) if sealed else enc
    _hold(members, contents, "sealed" if sealed else "plain")
    # zeros cost next to nothing whatever their length: the one byte did not make a span stored
    assert all(len(m) < 64 << 10 for m, (k, _, _) in zip(members, batch) if k.startswith("one-"))
    # and the device reads its own members past 4 MiB back, one of each kind
    pick = [max((i for i, (k, _, _) in enumerate(batch) if k == kind), key=lambda i: batch[i][1]) for kind in KINDS]
    assert all(batch[i][1] > 4 * MIB for i in pick)
    got = decode.decode_blobs([enc[i] for i in pick], key=KEY if sealed else None, compressed="GZIP")
    for i, g in zip(pick, got):
        assert g == contents[i], f"Decode of the {batch[i][0]} member of {batch[i][1]} bytes"


# ---- A2: sealed piece edges --------------------------------------------------------------
def test_sealed_piece_edges_from_frame_sourced_plaintext():
    """Random bytes are stored span by span, n + 18 + 5 * spans bytes: members
    one byte short of a piece, a piece, a byte more, and two pieces."""
    blobs = [ir.rnd(n, 950 + i) for i, n in enumerate((65507, 65508, 65509, 131034))]
    plain, _ = _encode(blobs)
    assert [len(m) for m in plain] == [65535, 65536, 65537, 131072], "this test needs these member lengths"
    _hold(plain, blobs)
    sealed, _ = _encode(blobs, key=KEY)
    assert _open(sealed, blobs) == plain
    assert [len(s) for s in sealed] == [60 + f + 28 * k for f, k in ((65535, 1), (65536, 1), (65537, 2), (131072, 2))]


# ---- A3: the block choice ----------------------------------------------------------------
_len_sym = functools.lru_cache(None)(ir.len_sym)
_dist_sym = functools.lru_cache(None)(ir.dist_sym)


def _fixed_bits(blk, content, end):
    """The block's symbols in the fixed code: the 3 header bits, the literals,
    the matches (length symbol, its extra bits, 5 bits of distance symbol, its
    extra bits) and the 7 bits of the end-of-block code."""
    first = blk["first"]
    lit = np.ones(end - first, dtype=bool)
    bits = 3 + 7
    for pos, ln, dist in blk["matches"]:
        lit[pos - first:pos - first + ln] = False
        s, eb, _ = _len_sym(ln)
        _, deb, _ = _dist_sym(dist)
        bits += ir.FIXED_LIT[s] + eb + 5 + deb
    b = np.frombuffer(content, dtype=np.uint8)[first:end][lit]
    return bits + 8 * int(b.size) + int((b >= 144).sum())


def _stored_bits(blk, content, end):
    p = blk["bit0"]
    return ((p + 3 + 7) & ~7) - p + 32 + 8 * (end - blk["first"])


def test_block_choice_is_the_smallest_by_exact_bit_count():
    """choose_block on the device: the smallest of stored, fixed and dynamic at
    the bit where the block starts; fixed when the codes tie, a code when it
    ties with stored.  Judged from the walk alone."""
    contents = []
    for n in range(1, 81):
        contents += [bytes(n), b"\x37" * n, ir.text(n, n), _period7(n)]
    for k in range(1, 5):
        for d in (-13, 13):
            n = SEG * k + d
            contents += [bytes(n), b"\x37" * n, ir.text(n, 200 + k), _period7(n)]
    for n in (SPAN - 1, SPAN, SPAN + 1):
        contents += [bytes(n), b"\x37" * n, ir.text(n, 300 + n % 7), _period7(n)]
    contents.append(_alternating(6, 500))
    assert sum(len(c) for c in contents) < WALK_BUDGET
    members, _ = _encode(contents)
    kinds = [0, 0, 0]
    stored_mid_byte = 0
    for i, (m, c) in enumerate(zip(members, contents)):
        out, end, walk = ir.inflate(m, 10)
        assert out == c and end + 8 == len(m), f"blob {i} ({len(c)} bytes)"
        assert walk[0]["bit0"] == 80 and [b["bit0"] for b in walk[1:]] == [b["bit1"] for b in walk[:-1]]
        for j, blk in enumerate(walk):
            upto = walk[j + 1]["first"] if j + 1 < len(walk) else len(c)
            size = blk["bit1"] - blk["bit0"]
            fixed, stored = _fixed_bits(blk, c, upto), _stored_bits(blk, c, upto)
            what = f"blob {i} ({len(c)} bytes) block {j}: btype {blk['btype']} of {size} bits, fixed {fixed}, " \
                   f"stored {stored} at bit {blk['bit0']}"
            kinds[blk["btype"]] += 1
            if blk["btype"] == 1:
                assert size == fixed and fixed <= stored, what
            elif blk["btype"] == 0:
                assert size == stored and stored < fixed, what
                stored_mid_byte += blk["bit0"] & 7 != 0
            else:
                assert size < fixed and size <= stored, what
        if len(c) == 1:
            # 18 bits fixed; stored is 43 or more, and a dynamic header alone is longer than 18
            assert [b["btype"] for b in walk] == [1] and walk[0]["bit1"] - walk[0]["bit0"] == 18
    assert all(kinds), f"stored, fixed and dynamic blocks all occur: {kinds}"
    assert stored_mid_byte, "no stored block started inside a byte"


# ---- A4: seeded random batches -----------------------------------------------------------
def _repeat(period, n):
    return (period * (n // len(period) + 1))[:n]


@pytest.mark.parametrize("seed", range(8))
def test_encode_gzip_random_batches(seed):
    """Random batches as test_encode_random_batches draws them for LZ4: 1-200
    blobs of 0 B-9 MiB until the batch holds 32 MiB, a quarter of them at the
    segment, span, piece, 64-span and block sizes, five kinds of content."""
    rng = np.random.default_rng(np.random.PCG64(5200 + seed))
    blobs, total = [], 0
    for i in range(int(rng.integers(1, 201))):
        if total >= 32 * MIB:
            break
        r = rng.random()
        if r < 0.05:
            n = 0
        elif r < 0.30:
            n = int(rng.choice([8192, 32768, 65536, 2 * MIB, 4 * MIB])) + int(rng.integers(-2, 3))
        else:
            n = int(np.exp(rng.uniform(0, np.log(9 << 20))))
        k = int(rng.integers(0, 5))
        s = 5300 + 512 * seed + i
        if k == 0:
            b = random_bytes(n, s).tobytes()
        elif k == 1:
            b = low_entropy(n, s, 0.02).tobytes() if n else b""
        elif k == 2:
            b = _repeat(random_bytes(int(rng.integers(1, 300)), s).tobytes(), n)
        elif k == 3:
            b = ir.text(n, s)
        else:
            b = _splice(ir.text(n, s), ir.rnd(n, s), n)
        assert len(b) == n
        blobs.append(b)
        total += n
    key = KEY if seed % 3 != 2 else None
    enc, _ = _encode(blobs, key=key)
    _hold(_open(enc, blobs, f"seed {seed}") if key else enc, blobs, f"seed {seed}")
    if seed < 2:
        assert decode.decode_blobs(enc, key=key, compressed="GZIP") == blobs
        sums = [hashlib.sha256(b).digest() for b in blobs]
        assert (decode.check_blobs(enc, sums, key=key, compressed="GZIP") == 0).all()
