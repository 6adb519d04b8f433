"""Prefix Decode on the device (cdc_decode_prefix_device): the first upto[i]
plaintext bytes of blob i, held against the full plaintext sliced.  Blobs come
from the project's own Encode (levels 0 and 9), from zlib and from liblz4.
Every call decodes into the middle of a sentinel-filled buffer whose margins,
and everything at and beyond out_offsets[n], must come back untouched."""
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import decode_ref as dr  # noqa: E402
import inflate_ref as ir  # noqa: E402
from plakar_amd import _lib, decode, encode  # noqa: E402
from plakar_amd._lib import CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_MISMATCH, CDC_E_NOSPACE  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32, 64))
SENTINEL = 0xA5
SLACK = 4096
MODES = {"LZ4": True, "GZIP": "GZIP", "NONE": False}
# the copy width, the wave width, the level-0 segment, the DEFLATE window and
# span, the GCM record (and the LZ4 distance)
UPTO = [0, 1, 15, 16, 17, 63, 64, 65, 8191, 8192, 8193, 32767, 32768, 32769, 65535, 65536, 65537]
LENGTHS = [1, 4097, 65537, (1 << 20) + 3]


def _run(blobs, pick, upto, mode, key=None, extra=SLACK):
    """One cdc_decode_prefix_device call over entries (blob pick[j], upto[j])
    into a sentinel-filled buffer: (status, out_offsets, the buffer on the host).
    An encoded blob is uploaded once however many entries read it."""
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8).copy()).cuda()
    pick = np.asarray(pick, dtype=np.int64)
    total = int(sum(upto))
    cap = max(total + extra, 0)
    buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo, st = decode.decode_prefix_device(base, offs[:-1][pick], lens[pick], upto, buf[SLACK:SLACK + cap], key=key,
                                         compressed=MODES[mode])
    return st, oo, buf.cpu().numpy()


def _hold(host, oo, st, upto, want, status):
    """want[j]: the bytes of entry j's range, or None where it may hold anything."""
    assert list(oo) == list(np.concatenate([[0], np.cumsum(upto)])), "out_offsets is the exclusive sum of upto"
    bad = [j for j in range(len(upto)) if st[j] != status[j]]
    assert not bad, [(j, int(st[j]), status[j], int(upto[j])) for j in bad[:10]]
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + int(oo[-1]):] == SENTINEL).all(), "bytes at or beyond out_offsets[n] were written"
    for j, w in enumerate(want):
        if w is not None:
            got = host[SLACK + int(oo[j]):SLACK + int(oo[j + 1])].tobytes()
            assert got == w, f"entry {j}: upto {int(upto[j])}"


def _expect(blobs, plains, entries, mode, key=None, status=None):
    """entries: (blob index, upto); every one is CDC_OK with the plaintext's
    prefix unless `status` says otherwise for it."""
    pick = [e[0] for e in entries]
    upto = np.array([e[1] for e in entries], dtype=np.uint64)
    status = status or [0] * len(entries)
    st, oo, host = _run(blobs, pick, upto, mode, key)
    want = [plains[b][:u] if s == 0 else None for (b, u), s in zip(entries, status)]
    _hold(host, oo, st, upto, want, status)


def _kind(kind, n, seed):
    if kind == "text":   # the cut falls inside matches
        return ir.text(n, seed)
    if kind == "zeros":  # one distance-1 match runs through the cut
        return bytes(n)
    if kind == "random":  # stored blocks
        return ir.rnd(n, seed)
    parts, i = [], 0
    while sum(len(p) for p in parts) < n:
        m = 1 + (7919 * (i + 1)) % 9000
        parts.append(_kind(("text", "zeros", "random")[i % 3], m, seed + i))
        i += 1
    return b"".join(parts)[:n]


@functools.lru_cache(None)
def _plains():
    return [_kind(k, n, 40 + i) for n in LENGTHS for i, k in enumerate(("text", "zeros", "random", "mix"))]


@functools.lru_cache(None)
def _encoded(mode, sealed, level):
    return encode.encode_blobs(list(_plains()), key=KEY if sealed else None, compress=MODES[mode], level=level)


def _cuts(n):
    return sorted({u for u in UPTO + [n - 1, n] if 0 <= u <= n})


@pytest.mark.parametrize("sealed", [False, True], ids=["plain", "sealed"])
@pytest.mark.parametrize("mode", list(MODES))
def test_grid(mode, sealed):
    plains = list(_plains())
    levels = (0, 9) if mode != "NONE" else (0,)
    blobs, src = [], []
    for level in levels:
        blobs += _encoded(mode, sealed, level)
        src += plains
    entries = [(b, u) for b in range(len(blobs)) for u in _cuts(len(src[b]))]
    assert len({u for _, u in entries}) >= len(UPTO) + 4
    _expect(blobs, src, entries, mode, key=KEY if sealed else None)


@functools.lru_cache(None)
def _foreign_gzip():
    content = ir.text(300_000, 5) + ir.rnd(70_000, 6) + ir.text(200_000, 7)
    return content, [ir.gz(content, level=lv) for lv in (1, 6, 9)]


def test_gzip_members_written_by_zlib():
    content, members = _foreign_gzip()
    n = len(content)
    for m in members:
        assert zlib.decompress(m, 31) == content
    cuts = _cuts(n) + [299_999, 300_000, 300_001, 335_000, 369_999, 370_000, 370_001, 500_000]
    entries = [(b, u) for b in range(3) for u in cuts]
    _expect(members, [content] * 3, entries, "GZIP")
    sealed = [dr.seal_stream(KEY, m, 900 + i) for i, m in enumerate(members)]
    _expect(sealed, [content] * 3, entries[::3], "GZIP", key=KEY)


def test_lz4_frames_with_64k_blocks_and_block_checksums():
    ff = dr.fixture_frames()
    names = ["lz4f-0x7c", "mixed", "many-blocks", "lz4f-0x64", "ext-0", "ext-1", "empty"]
    frames = [ff[k][0] for k in names]
    plains = [ff[k][1] for k in names]
    n = len(plains[0])
    assert frames[0][4:6] == b"\x7c\x40" and n > 4 * 65536, "64-KiB blocks, block checksums, five blocks"
    entries = []
    for b, p in enumerate(plains):
        cuts = set(_cuts(len(p)))
        if b == 0:  # in the first, the second and the last block, and on their edges
            cuts |= {100, 70_000, 131_071, 131_072, 131_073, 4 * 65536 - 1, 4 * 65536, 4 * 65536 + 1, n - 3}
        entries += [(b, u) for u in sorted(cuts)]
    _expect(frames, plains, entries, "LZ4")
    sealed = [dr.seal_stream(KEY, f, 950 + i) for i, f in enumerate(frames)]
    _expect(sealed, plains, entries[::2], "LZ4", key=KEY)


def _full_status(blob, mode):
    lens = np.array([len(blob)], dtype=np.uint64)
    base = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    _, st = decode.decode_device(base, [0], lens, out, compressed=MODES[mode])
    return int(st[0])


@pytest.mark.parametrize("mode", ["LZ4", "GZIP"])
def test_the_trailer_is_not_read_early(mode):
    if mode == "LZ4":
        frame, content = dr.fixture_frames()["lz4f-0x64"]
        bad = dr.flip(frame, len(frame) - 2)          # the content checksum
    else:
        content = ir.text(150_000, 11)
        good = ir.gz(content)
        bad = dr.flip(good, len(good) - 6, 3)         # the CRC-32
    n = len(content)
    assert _full_status(bad, mode) == CDC_E_CORRUPT
    cuts = [u for u in _cuts(n) if u < n]
    entries = [(0, u) for u in cuts] + [(0, n)]
    _expect([bad], [content], entries, mode, status=[0] * len(cuts) + [CDC_E_CORRUPT])


@pytest.mark.parametrize("mode", ["LZ4", "GZIP"])
def test_a_bad_tag_anywhere_fails_a_compressed_blob(mode):
    content = ir.rnd(200_000, 12) + ir.text(5000, 13)
    (good,) = encode.encode_blobs([content], key=KEY, compress=MODES[mode])
    assert len(good) > 60 + 3 * 65564, "several records"
    bad = dr.flip(good, len(good) - 1)                # the last record's tag
    n = len(content)
    entries = [(0, 1), (0, 100), (0, 65536), (0, n), (1, 0), (1, 1), (1, 17), (1, 65536), (1, n - 1), (1, n)]
    _expect([good, bad], [content, content], entries, mode, key=KEY,
            status=[0, 0, 0, 0, 0] + [CDC_E_AUTH] * 5)


def test_not_compressed_opens_only_the_records_it_needs():
    n = 3 * 65536 + 100
    content = ir.rnd(n, 14)
    (good,) = encode.encode_blobs([content], key=KEY, compress=False)
    assert len(good) == 60 + 3 * 65564 + 128, "four records"
    bad = dr.flip(good, len(good) - 1)                # the last record's tag
    ups = [0, 1, 65535, 65536, 65537, 2 * 65536, 3 * 65536]
    entries = [(0, u) for u in ups + [3 * 65536 + 1, n]] + [(1, u) for u in ups] + [(1, 3 * 65536 + 1), (1, n)]
    status = [0] * (len(ups) + 2) + [0] * len(ups) + [CDC_E_AUTH, CDC_E_AUTH]
    _expect([good, bad], [content, content], entries, "NONE", key=KEY, status=status)
    # a tag in the second record: the first record's bytes still come
    bad2 = dr.flip(good, 60 + 2 * 65564 - 1)
    _expect([bad2], [content], [(0, 65536), (0, 65537), (0, 1)], "NONE", key=KEY, status=[0, CDC_E_AUTH, 0])
    # the blob without its later records: what a ranged reader gathers
    short = good[:60 + 2 * 65564]
    _expect([short], [content], [(0, 2 * 65536), (0, 70_000)], "NONE", key=KEY)


@pytest.mark.parametrize("sealed", [False, True], ids=["plain", "sealed"])
@pytest.mark.parametrize("mode", list(MODES))
def test_upto_past_the_length_is_a_mismatch(mode, sealed):
    plains = [ir.text(3001, 15), ir.text(70_001, 16), ir.rnd(4099, 17), b"", ir.text(999, 18)]
    blobs = encode.encode_blobs(plains, key=KEY if sealed else None, compress=MODES[mode])
    entries = [(0, 3001), (1, 70_002), (2, 4099), (3, 1), (4, 999), (1, 70_001), (3, 0)]
    _expect(blobs, plains, entries, mode, key=KEY if sealed else None,
            status=[0, CDC_E_MISMATCH, 0, CDC_E_MISMATCH, 0, 0, 0])


@pytest.mark.parametrize("mode", list(MODES))
def test_a_batch_of_1500_small_blobs(mode):
    rng = np.random.default_rng(19)
    plains = [_kind(("text", "random", "zeros")[i % 3], int(rng.integers(0, 300)), 2000 + i) for i in range(1500)]
    blobs = encode.encode_blobs(plains, key=KEY, compress=MODES[mode])
    upto = [int(rng.integers(0, len(p) + 1)) if i % 4 else len(p) for i, p in enumerate(plains)]
    assert sum(1 for u in upto if u == 0) > 3
    _expect(blobs, plains, list(zip(range(1500), upto)), mode, key=KEY)


@pytest.mark.parametrize("mode", list(MODES))
def test_capacity_one_byte_short(mode):
    plains = [ir.text(5000, 20), ir.rnd(700, 21)]
    blobs = encode.encode_blobs(plains, compress=MODES[mode])
    with pytest.raises(_lib.CdcError) as e:
        _run(blobs, [0, 1], np.array([4000, 700], dtype=np.uint64), mode, extra=-1)
    assert e.value.status == CDC_E_NOSPACE and e.value.needed == 4700
    # the same call by hand, to look at the buffer afterwards
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    buf = torch.full((4700 + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.CdcError):
        decode.decode_prefix_device(base, [0, len(blobs[0])], lens, [4000, 700], buf[:4699], compressed=MODES[mode])
    assert (buf.cpu().numpy() == SENTINEL).all(), "nothing is written when the capacity is short"


def test_module_functions():
    plains = [ir.text(9000, 22), ir.rnd(100, 23), b""]
    for name in ("LZ4", "GZIP", None):
        blobs = encode.DeviceEncoder(key=KEY, compression=name).encode_many(plains)
        got = decode.decode_prefix(blobs, [8193, 100, 0], key=KEY, compression=name)
        assert got == [plains[0][:8193], plains[1], b""]
        d = decode.DeviceDecoder(key=KEY, compression=name)
        r = d.decode_prefix_many(blobs, [9001, 1, 1])
        assert isinstance(r[0], decode.DecodeError) and r[0].status == CDC_E_MISMATCH
        assert r[1] == plains[1][:1] and isinstance(r[2], decode.DecodeError)
