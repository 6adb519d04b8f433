"""Device Encode, structurally: tests/test_encode.py proves that every frame
is decodable; these tests aim at the places where the kernels of
plakar_amd/csrc/cdc_encode.hip can go wrong while still producing decodable
or plausible output.  Every LZ4 frame goes through the strict walker
(tests/lz4_ref.py: the block format's rules, the sequence list) and through
liblz4; every GCM piece is compared byte for byte with libcrypto; sizes are
held against liblz4 restricted to the kernel's 8-KiB match window.  Each test
asserts, from the walker's sequence list or the returned offsets, that the
structure it aims at really occurred, so that no case goes stale silently."""
import functools
import hashlib
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref as ref  # noqa: E402
import lz4_ref as lz  # noqa: E402
from datagen import low_entropy, random_bytes, text_like  # noqa: E402
from plakar_amd import _lib, encode  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
KiB, MiB = 1 << 10, 1 << 20
SEG, BLK, PIECE = 8192, 4 * MiB, 65536


@pytest.fixture(scope="module", autouse=True)
def _init():
    _lib.ensure_init()


def rnd_for(n, seed):
    """The caller's random material (56 bytes per blob), fixed by the seed."""
    return random_bytes(encode.RANDOM_BYTES * n, 900_000 + seed).tobytes()


def rb(n, seed):
    return random_bytes(n, seed).tobytes()


def payload(blocks):
    return sum(b.size for b in blocks)


def check_frame(frame, blob):
    """Both decoders give the blob back; the walker's blocks."""
    if not blob:  # DeflateStream of empty input is an empty stream, not a frame
        assert frame == b""
        return []
    blocks = lz.walk_frame(frame)
    assert lz.content(blocks) == blob, f"walker: {len(blob)} bytes"
    assert ref.lz4f_decompress(frame) == blob, f"liblz4: {len(blob)} bytes"
    return blocks


def to_device(blobs, align=None):
    """The blobs in one device buffer; align: blob i starts at an offset
    congruent to align[i % len(align)] mod 16.  Returns (tensor, offs, lens)."""
    offs, pos = [], 0
    for i, b in enumerate(blobs):
        if align is not None:
            pos = (pos + 15) // 16 * 16 + align[i % len(align)]
        offs.append(pos)
        pos += len(b)
    host = np.zeros(max(pos, 1), np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(host).cuda(), offs, [len(b) for b in blobs]


def encode_at(blobs, align, key=None, compress=True, random=None):
    """encode_device over blobs placed at the given source alignments: the
    encoded bytes, blob by blob, and the output offsets."""
    t, offs, lens = to_device(blobs, align)
    cap = sum(encode.encode_bound(n, compress, key is not None) for n in lens)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(t, offs, lens, out, key=key, compress=compress, random=random)
    host = out[:int(oo[-1])].cpu().numpy()
    return [host[oo[i]:oo[i + 1]].tobytes() for i in range(len(blobs))], oo, offs


# ---------------------------------------------------------------------------
# a. mixed content inside one block
# ---------------------------------------------------------------------------
def _alternating(n, seed):
    """8-KiB segments of text alternating with 8-KiB segments of random."""
    text, rand = text_like(n // 2 + SEG, seed), rb(n // 2 + SEG, seed + 1)
    parts = []
    for i in range((n + SEG - 1) // SEG):
        src = text if i % 2 == 0 else rand
        parts.append(src[(i // 2) * SEG:(i // 2 + 1) * SEG])
    return b"".join(parts)[:n]


@functools.lru_cache(maxsize=None)
def mixed_blobs():
    """name -> (blob, random run of >= 1 MiB before compressible data, ends in
    >= 1 MiB of random, holds whole segments of zeros, number of random
    segments that lie between two text segments of one block)."""
    first = rb(2 * MiB, 101) + bytes(2 * MiB)
    alt1, alt4 = _alternating(MiB, 110), _alternating(4 * MiB + 8 * KiB + 3, 112)
    return {
        "random+zeros": (first, True, False, True, 0),
        "zeros+random": (bytes(2 * MiB) + rb(2 * MiB - 7, 102), False, True, True, 0),
        "64k-zeros+random": (bytes(64 * KiB) + rb(MiB, 103), False, True, True, 0),
        "random+text+random+zeros": (rb(MiB, 104) + text_like(24 * KiB, 105) + rb(MiB, 106) + bytes(MiB),
                                     True, False, True, 0),
        "alternating-1MiB": (alt1, False, False, False, 63),
        "alternating-4MiB+": (alt4, False, False, False, 255),
        "9MiB-repeated": ((first * 3)[:9 * MiB], True, True, True, 0),
    }


@functools.lru_cache(maxsize=None)
def mixed_encoded():
    """One compress-only batch of the mixed blobs: name -> (blob, blocks)."""
    B = mixed_blobs()
    outs = encode.encode_blobs([v[0] for v in B.values()], key=None, compress=True)
    return {name: (v[0], check_frame(o, v[0])) for (name, v), o in zip(B.items(), outs)}


MIXED = ["random+zeros", "zeros+random", "64k-zeros+random", "random+text+random+zeros", "alternating-1MiB",
         "alternating-4MiB+", "9MiB-repeated"]


@pytest.mark.parametrize("name", MIXED)
def test_mixed_content_blocks(name):
    """k_lz4_size / k_lz4_emit (rec_geom, blk_prologue's prev_end max-scan,
    kMaxSegsPerBlk = 512 segments per block, the final literal-only sequence):
    blocks whose literal runs span many segments without a record, between
    segments that have records.  A block is compressed wherever the reference
    compressor, restricted to the 8-KiB window, gains more than 64 bytes.

    Which structure a blob must show follows from how it is built: a run of
    >= 1 MiB of literals followed by a match where >= 1 MiB of random data
    precedes compressible data; a final run of >= 1 MiB where the blob ends in
    random data; a match of >= 8,000 bytes where it holds 8-KiB segments of
    zeros; and, for the alternating blobs (no run can reach 1 MiB there), a
    literal run of >= 8 KiB followed by a match for every random segment that
    lies between two text segments."""
    _, run_then_match, final_run, zero_segs, between = mixed_blobs()[name]
    blob, blocks = mixed_encoded()[name]
    assert len(blocks) == (len(blob) + BLK - 1) // BLK
    for k, b in enumerate(blocks):
        part = blob[k * BLK:(k + 1) * BLK]
        r = lz.ref_windowed_size(part)
        print(f"{name} block {k}: {len(part)} B, reference {r}, device {b.size}{' stored' if b.stored else ''}")
        if r < len(part) - 64:
            assert not b.stored, f"block {k}: stored, the reference compresses it to {r}"
    seqs = [s for b in blocks for s in b.seqs]
    if run_then_match:
        assert any(ll >= MiB and ml for ll, _, ml in seqs), "no literal run >= 1 MiB before a match"
    if final_run:
        last = blocks[-1]
        assert (last.size if last.stored else last.seqs[-1][0]) >= MiB, "no final literal run >= 1 MiB"
    if name == "zeros+random":  # the one compressed block that ends in a multi-MiB literal-only sequence
        assert not blocks[0].stored and blocks[0].seqs[-1] == (2 * MiB - 7, 0, 0)
    if name == "64k-zeros+random":
        assert not blocks[0].stored and blocks[0].seqs[-1] == (MiB, 0, 0)
    if zero_segs:
        assert any(ml >= 8000 for _, _, ml in seqs), "no match >= 8,000 bytes"
    if between:
        n = sum(1 for ll, _, ml in seqs if ll >= SEG and ml)
        assert n >= between, f"{n} literal runs >= 8 KiB before a match, {between} random segments"
    if name == "9MiB-repeated":
        assert [b.stored for b in blocks] == [False, False, True] and len(blocks[2].data) == MiB


# ---------------------------------------------------------------------------
# b. end of block, tiny sizes
# ---------------------------------------------------------------------------
EDGE_LENS = (list(range(0, 81)) + [SEG * k + r for k in (1, 2, 3) for r in range(-13, 14)] +
             [BLK + r for r in list(range(-13, 14)) + [SEG - 1, SEG, SEG + 1]] + [2 * BLK + 5])


@functools.lru_cache(maxsize=None)
def edge_master(kind):
    n = max(EDGE_LENS)
    if kind == "zeros":
        return bytes(n)
    if kind == "0xAB":
        return b"\xab" * n
    if kind == "text":
        return text_like(n, 21)
    return (b"\x01\x5a\xc3\x07\xee\x10\x99" * (n // 7 + 1))[:n]  # a 7-byte period


_edge_seen = {}  # digest of (frame, blob) -> per-block (stored, decoded length, sequences, last sequence)


def _edge_check(frame, blob):
    """check_frame, once per distinct (frame, blob): the three modes produce
    the same frames (the encoder is deterministic), and a 4-MiB block of text
    is half a million sequences to walk.  liblz4 decodes every frame."""
    if not blob:
        assert frame == b""
        return []
    key = hashlib.sha256(frame).digest() + hashlib.sha256(blob).digest()
    if key not in _edge_seen:
        blocks = lz.walk_frame(frame)
        assert lz.content(blocks) == blob, f"walker: {len(blob)} bytes"
        _edge_seen[key] = [(b.stored, len(b.data), len(b.seqs), b.seqs[-1] if b.seqs else None) for b in blocks]
    assert ref.lz4f_decompress(frame) == blob, f"liblz4: {len(blob)} bytes"
    return _edge_seen[key]


@pytest.mark.parametrize("mode", ["compress", "compress+encrypt", "device"])
@pytest.mark.parametrize("kind", ["zeros", "0xAB", "text", "period7"])
def test_end_of_block_and_tiny_sizes(kind, mode):
    """k_lz4_seq's start_lim / end_lim from S.rem (a match starts >= 12 bytes
    before the block's end, the last 5 bytes are literals), within a segment
    and across the boundary to a last segment of 1-13 bytes; blobs, last
    segments and last blocks of 1-13 bytes.  The walker's rules are the
    assertion.  A block shorter than 13 bytes is stored or literal-only.

    That the limit is reached, not merely respected: in the constant and
    periodic kinds every match runs to its limit, so a block of >= 8,179 bytes
    ends in exactly 5 literals, or, where its last segment has t = 5..13 bytes
    (too short to hold a match), in exactly t."""
    master = edge_master(kind)
    blobs = [master[:n] for n in EDGE_LENS]
    seed = ["zeros", "0xAB", "text", "period7"].index(kind)
    if mode == "compress":
        frames = encode.encode_blobs(blobs, key=None, compress=True)
    elif mode == "compress+encrypt":
        outs = encode.encode_blobs(blobs, key=KEY, compress=True, random=rnd_for(len(blobs), seed))
        frames = [ref.decrypt_stream(KEY, o)[0] for o in outs]
    else:
        frames, _, offs = encode_at(blobs, list(range(16)))
        assert {o % 16 for o, b in zip(offs, blobs) if len(b) >= SEG - 13} == set(range(16))
    limits = 0
    for n, f in zip(EDGE_LENS, frames):
        blocks = _edge_check(f, master[:n])
        assert len(blocks) == (n + BLK - 1) // BLK
        for stored, dlen, nseq, last in blocks:
            if dlen < 13:
                assert stored or nseq == 1, f"{n}: a block of {dlen} bytes holds a match"
            if dlen >= SEG - 13:
                assert not stored, f"{n}: block of {dlen} bytes stored"
                if kind != "text":
                    t = dlen % SEG
                    want = t if 5 <= t <= 13 else 5
                    assert last == (want, 0, 0), f"{n}: block of {dlen} ends in {last}, expected {want} literals"
                    limits += 1
    assert kind == "text" or limits >= 3 * 27 + 30 + 2


# ---------------------------------------------------------------------------
# c. what the kernel must find
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0x00, 0xAB])
def test_constant_blob_size_cap(byte):
    """k_lz4_seq's first step tries 64 positions against an empty table, so at
    most 64 literals precede a segment's first match, and the rest of the
    segment is one match: token 1, literal-length byte 1, literals <= 64,
    offset 2, match-length bytes <= 33: <= 101 bytes per 8-KiB segment (the
    reference: 43), and token + 5 literals end the block.  The cap asserted
    is 112 per segment plus 5 per block; anything near a multiple of it means
    lost matches."""
    lens = [SEG, MiB, BLK + SEG]
    blobs = [bytes([byte]) * n for n in lens]
    outs = encode.encode_blobs(blobs, key=None, compress=True)
    for n, b, o in zip(lens, blobs, outs):
        blocks = check_frame(o, b)
        nseg = sum((len(k.data) + SEG - 1) // SEG for k in blocks)
        print(f"constant {byte:#x} x {n}: payload {payload(blocks)}, cap {112 * nseg + 5 * len(blocks)}, "
              f"reference {lz.ref_windowed_size(b)}")
        assert payload(blocks) <= 112 * nseg + 5 * len(blocks)
        for k in blocks:
            assert not k.stored
            assert len(k.seqs) == (len(k.data) + SEG - 1) // SEG + 1  # one match per segment
            assert all(ll <= 64 and ml >= SEG - 64 - 5 for ll, _, ml in k.seqs[:-1])


SAVINGS = MIXED + ["low-1%", "low-5%", "text"]


@pytest.mark.parametrize("name", SAVINGS)
def test_savings_condition(name):
    """The kernel keeps at least half of what the reference compressor saves
    with the same 8-KiB window (kSegLZ = 8192, kHashBits = 11): payload <= n -
    (n - ref_windowed_size) / 2.
    A condition, not a tuned tolerance: losing a class of matches (backward
    extension, every segment after a block's first, ...) fails it.  Reference
    sizes for 1 MiB: zeros 5,504; low 1 % 69,533; low 5 % 248,044; text
    353,050; half random 529,216."""
    if name in MIXED:
        blob, blocks = mixed_encoded()[name]
    else:
        blob = {"low-1%": lambda: low_entropy(MiB, 31, 0.01).tobytes(),
                "low-5%": lambda: low_entropy(MiB, 32, 0.05).tobytes(),
                "text": lambda: text_like(MiB, 33)}[name]()
        (o,) = encode.encode_blobs([blob], key=None, compress=True)
        blocks = check_frame(o, blob)
    n, r, p = len(blob), lz.ref_windowed_size(blob), payload(blocks)
    print(f"{name}: n {n}, reference {r}, device payload {p}, ratio {p / r:.3f}, cap {n - (n - r) / 2:.0f}")
    assert r < n, "the blob is meant to be compressible"
    assert p <= n - (n - r) / 2, f"payload {p}, reference {r} of {n}"


# ---------------------------------------------------------------------------
# d. GCM geometry
# ---------------------------------------------------------------------------
GCM_LENS = [1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040, 1041, 2031, 2032, 2047, 2048, 2049, 2063,
            2064, 2065, 65519, 65520, 65521, 65535, 65536, 65537, 65536 + 1025, 2 * 65536 + 2049]
GCM_SRC = [0, 1, 2, 3, 5, 8, 15]


def piece_nonce(dn, k):
    return dn[:8] + (int.from_bytes(dn[8:], "big") ^ k).to_bytes(4, "big")


def check_sealed(out, blob, rnd, what):
    """out is EncryptStream(blob) under the material rnd, byte for byte: the
    header, then nonce || ciphertext || tag of every 64-KiB piece as libcrypto
    seals it.  Returns the number of pieces."""
    sub, sn, dn = rnd[:32], rnd[32:44], rnd[44:56]
    assert out[:12] == sn, what
    assert ref.gcm_open(KEY, out[:12], out[12:60]) == sub, what
    pos, k = 60, 0
    for p0 in range(0, len(blob), PIECE):
        piece = blob[p0:p0 + PIECE]
        nonce = piece_nonce(dn, k)
        assert out[pos:pos + 12] == nonce, f"{what}: nonce of piece {k}"
        sealed = ref.gcm_seal(sub, nonce, piece)
        got = out[pos + 12:pos + 12 + len(sealed)]
        assert got[:-16] == sealed[:-16], f"{what}: ciphertext of piece {k}"
        assert got[-16:] == sealed[-16:], f"{what}: tag of piece {k}"
        pos += 12 + len(sealed)
        k += 1
    assert pos == len(out), what
    return k


def test_gcm_geometry_against_libcrypto():
    """k_gcm works in rows of 64 blocks (1,024 bytes) and steps of kGcmRows = 2
    rows (2,048 bytes): piece lengths around 1,024, 2,048 and 65,536 and their
    last 16-byte block (the lanes' Horner exponent e = nb - lane - 64 (cnt -
    1), the ragged row_bytes), the source address mod 4 (pt_sh, pt_fast) and
    the destination address mod 4 (hb), every piece byte for byte against
    libcrypto."""
    blobs, aligns = [], []
    for j, s in enumerate(GCM_SRC):
        for i, n in enumerate(GCM_LENS):
            blobs.append(rb(n, 7000 + 64 * j + i))
            aligns.append(s)
        # one more byte per round: the 29 lengths sum to 2 mod 4, so with it every
        # round starts one destination alignment on (the header and the pieces'
        # nonces and tags are multiples of 4)
        blobs.append(rb(1, 7000 + 64 * j + 63))
        aligns.append(s)
    rnd = rnd_for(len(blobs), 4)
    # to_device takes the alignment of blob i from aligns[i % len(aligns)]
    outs, oo, offs = encode_at(blobs, aligns, key=KEY, compress=False, random=rnd)
    assert [o % 16 for o in offs] == aligns
    assert {int(o) % 4 for o in oo[:-1]} == {0, 1, 2, 3}
    # every length meets every destination alignment
    seen = {}
    for b, o in zip(blobs, oo[:-1]):
        seen.setdefault(len(b), set()).add(int(o) % 4)
    assert all(seen[n] == {0, 1, 2, 3} for n in GCM_LENS), seen
    for i, (b, o) in enumerate(zip(blobs, outs)):
        assert len(o) == encode.encode_bound(len(b), False, True)
        k = check_sealed(o, b, rnd[56 * i:56 * i + 56], f"blob {i}: {len(b)} B at source {aligns[i]} mod 16, "
                         f"destination {int(oo[i]) % 4} mod 4")
        assert k == (len(b) + PIECE - 1) // PIECE


# ---------------------------------------------------------------------------
# e. more than 255 pieces
# ---------------------------------------------------------------------------
def test_gcm_more_than_255_pieces():
    """k_gcm's nonce word j0[2] = the data nonce's last four bytes XOR k,
    big-endian, a piece being kPiece = 65,536 bytes: past piece 255 the index
    reaches the XOR's second byte; and
    piece_base (k_enc_plan's scan) for the blob that follows a long one."""
    blobs = [rb(17 * MiB + 123, 8001), rb(3 * PIECE + 77, 8002)]
    rnd = bytearray(rnd_for(2, 5))
    rnd[52:56] = b"\x5a\xa5\xfe\x81"  # the first blob's nonce counter bytes: set, so an OR or an add differ from XOR
    rnd = bytes(rnd)
    outs = encode.encode_blobs(blobs, key=KEY, compress=False, random=rnd)
    n0 = check_sealed(outs[0], blobs[0], rnd[:56], "long blob")
    assert n0 == 273 > 257
    dn = rnd[44:56]
    for k in (255, 256, 257):
        pos = 60 + k * (PIECE + 28)
        assert outs[0][pos:pos + 8] == dn[:8]
        assert outs[0][pos + 8:pos + 12] == struct.pack(">I", 0x5AA5FE81 ^ k)
    assert check_sealed(outs[1], blobs[1], rnd[56:], "blob after the long one") == 4
    for o, b in zip(outs, blobs):  # and DecryptStream opens every piece
        assert ref.decrypt_stream(KEY, o)[0] == b


# ---------------------------------------------------------------------------
# f. XXH32 region pipeline
# ---------------------------------------------------------------------------
def test_xxh32_region_boundaries():
    """k_xxh32's software pipeline over kXxRegion = 4,096-byte regions (chains
    over region r, store r + 1, prefetch r + 3 and r + 4; R = 1..8 regions,
    odd and even), the stripes' end within 17 bytes of a region boundary, the
    source address mod 4 (the funnel shift sh and the clamp klast), lengths
    mixed across the waves of a workgroup (the host sorts longest first)."""
    import xxhash
    lens = [4096 * k + d for k in (1, 2, 3, 4, 5, 8) for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17)]
    blobs, aligns = [], []
    for a in range(4):
        for i, n in enumerate(lens):
            # half random (stored), half text (compressed): the checksum is of the content either way
            blobs.append(rb(n, 9000 + 64 * a + i) if i % 2 else text_like(n, 9000 + 64 * a + i))
            aligns.append(4 * (i % 4) + a)
    order = np.random.default_rng(5).permutation(len(blobs))
    blobs, aligns = [blobs[i] for i in order], [aligns[i] for i in order]
    frames, _, offs = encode_at(blobs, aligns)
    assert {(len(b), o % 4) for b, o in zip(blobs, offs)} == {(n, a) for n in lens for a in range(4)}
    regions = {(len(b) // 16 * 16 + 4095) // 4096 for b in blobs}
    assert regions >= {1, 2, 3, 4, 5, 6, 8, 9}, regions
    for b, f in zip(blobs, frames):
        check_frame(f, b)
        assert f[-4:] == struct.pack("<I", xxhash.xxh32(b).intdigest()), f"{len(b)} bytes"
