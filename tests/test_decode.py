"""Decode on the device (cdc_decode_device / cdc_check_device) against the
reference reader restated in crypto_ref (libcrypto's GCM, liblz4's frame
decoder): fixtures from the system libraries, this library's own Encode, the
corruptions of decode_ref, and the packfiles of a backup run."""
import functools
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
import packfile_ref as pf  # noqa: E402
from plakar_amd import _lib, decode, encode, snapshot  # noqa: E402
from plakar_amd._lib import CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_MISMATCH, CDC_E_NOSPACE, CDC_E_UNSUPPORTED  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))
SENTINEL = 0xA5
SLACK = 4096


def _device_decode(blobs, key, compressed, cap=None):
    """One cdc_decode_device call with sentinel slack on both sides of d_out:
    (plaintexts or None per blob, status, out_offsets, the whole buffer on the host, cap)."""
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8).copy()).cuda()
    if cap is None:
        cap = sum(len(crypto_ref.decode(b, key, compressed)) if _ok(b, key, compressed) else 0 for b in blobs)
    buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[SLACK:SLACK + cap]
    oo, st = decode.decode_device(base, offs[:-1], lens, out, key=key, compressed=compressed)
    host = buf.cpu().numpy()
    body = host[SLACK:]
    got = [None if st[i] else body[oo[i]:oo[i + 1]].tobytes() for i in range(len(blobs))]
    return got, st, oo, host, cap


def _ok(b, key, compressed):
    try:
        crypto_ref.decode(b, key, compressed)
        return True
    except (ValueError, AssertionError):
        return False


def _sentinels_intact(host, cap, used):
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + used:] == SENTINEL).all(), "bytes past out_offsets[n] were written"


@pytest.mark.parametrize("sealed", [False, True], ids=["bare", "sealed"])
def test_parity_with_the_reference_reader(sealed):
    frames = dr.fixture_frames()
    names = list(frames)
    key = KEY if sealed else None
    blobs = [dr.seal_stream(KEY, frames[n][0], 20 + i) if sealed else frames[n][0] for i, n in enumerate(names)]
    # the linked-block frame is refused; it decodes to nothing here
    want = [None if frames[n][1] is None else crypto_ref.decode(b, key, True) for n, b in zip(names, blobs)]
    for n, w in zip(names, want):
        assert w == frames[n][1]
    cap = sum(len(w) for w in want if w is not None)
    got, st, oo, host, _ = _device_decode(blobs, key, True, cap=cap)
    for n, g, w, s in zip(names, got, want, st):
        if w is None:
            assert s == CDC_E_UNSUPPORTED, n
        else:
            assert s == 0, (n, s)
            assert g == w, n
    assert oo[-1] == cap
    _sentinels_intact(host, cap, cap)


def test_gcm_edges_uncompressed():
    sizes = [0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 131073]
    plains = [dr.rnd(n, 40 + i) for i, n in enumerate(sizes)]
    blobs = [dr.seal_stream(KEY, p, 60 + i) for i, p in enumerate(plains)]
    # a record that is an empty Seal (28 bytes) is legal and yields nothing
    # (after a full record: boundaries follow from the length alone)
    sub_stream = dr.seal_stream(KEY, plains[9], 99)
    sub = crypto_ref.decrypt_stream(KEY, sub_stream)[1]
    n0 = bytes(range(12))
    blobs.append(sub_stream + n0 + crypto_ref.gcm_seal(sub, n0, b""))
    plains.append(plains[9])
    for b, p in zip(blobs, plains):
        assert crypto_ref.decode(b, KEY, False) == p
    got, st, oo, host, cap = _device_decode(blobs, KEY, False)
    assert (st == 0).all(), st
    assert got == plains
    _sentinels_intact(host, cap, int(oo[-1]))


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("key", [None, KEY], ids=["plain", "key"])
def test_round_trip_of_this_librarys_encode(compress, key):
    text = (b"the quick brown fox jumps over the lazy dog " * 3000)[:100_003]
    plains = [b"", b"\x42", dr.rnd(70_001, 70), bytes(200_000), text, dr.block_fixture()]
    blobs = encode.encode_blobs(plains, key=key, compress=compress)
    for b, p in zip(blobs, plains):
        assert crypto_ref.decode(b, key, compress) == p
    got, st, oo, host, cap = _device_decode(blobs, key, compress)
    assert (st == 0).all(), st
    assert got == plains
    _sentinels_intact(host, cap, int(oo[-1]))
    assert decode.decode_blobs(blobs, key=key, compressed=compress) == plains
    d = decode.DeviceDecoder(key=key, compression="LZ4" if compress else None)
    assert d(blobs[4]) == text


@functools.lru_cache(None)
def _corruption_cases():
    good, _ = dr.fixture_frames()["mixed"]
    three = dr.rnd(3 * dr.PIECE - 100, 80)  # three records uncompressed
    sealed = dr.seal_stream(KEY, good, 81)
    full = dr.seal_stream(KEY, dr.rnd(dr.PIECE, 84), 85)  # one record of exactly 65,580 bytes
    cases = {
        # name: (bad blob, key, compressed, status)
        "subkey-bit": (dr.flip(sealed, 20), KEY, True, CDC_E_AUTH),
        "subkey-tag-bit": (dr.flip(sealed, 59, 7), KEY, True, CDC_E_AUTH),
        "record-1-of-3-ciphertext-bit": (dr.flip(dr.seal_stream(KEY, three, 82), 60 + 65580 + 12 + 5000, 3), KEY, False,
                                         CDC_E_AUTH),
        "record-tag-bit": (dr.flip(sealed, len(sealed) - 1), KEY, True, CDC_E_AUTH),
        "record-nonce-bit": (dr.flip(sealed, 60 + 3), KEY, True, CDC_E_AUTH),
        "sealed-truncated-by-one": (sealed[:-1], KEY, True, CDC_E_AUTH),  # the last record's tag no longer fits
        "truncated-to-59": (sealed[:59], KEY, True, CDC_E_CORRUPT),
        # after a full record (boundaries follow from the length alone): too short for a nonce and a tag
        "trailing-record-of-27": (full + bytes(27), KEY, False, CDC_E_CORRUPT),
        "trailing-12-bytes": (full + bytes(12), KEY, False, CDC_E_CORRUPT),
    }
    for name, frame in dr.corrupt_frames().items():
        cases[name] = (frame, None, True, CDC_E_CORRUPT)
        cases[name + "-sealed"] = (dr.seal_stream(KEY, frame, 83), KEY, True, CDC_E_CORRUPT)
    return cases


@pytest.mark.parametrize("name", sorted(_corruption_cases()))
def test_corruption_is_reported_and_contained(name):
    bad, key, compressed, status = _corruption_cases()[name]
    frames = dr.fixture_frames()
    goods = [dr.rnd(1000 + 977 * i, 90 + i) if not compressed else frames[n][0]
             for i, n in enumerate(["lz4f-0x7c", "ext-0", "mixed"])]
    if key is not None:
        goods = [dr.seal_stream(key, g, 95 + i) for i, g in enumerate(goods)]
    blobs = [goods[0], bad, goods[1], goods[2]]
    want = [crypto_ref.decode(g, key, compressed) for g in goods]
    got, st, oo, host, cap = _device_decode(blobs, key, compressed, cap=sum(len(w) for w in want) + 300_000)
    assert list(st) == [0, status, 0, 0]
    assert oo[2] == oo[1], "a failed blob contributes no bytes"
    assert [got[0], got[2], got[3]] == want
    assert oo[-1] == sum(len(w) for w in want)
    # a content checksum fails only after the blob was written into its own planned range
    _sentinels_intact(host, cap, cap if name.startswith("bad-content-checksum") else int(oo[-1]))


def test_frame_header_rules():
    """Every header branch in one batch: what pierrec's writer never makes is
    refused as unsupported, what no writer may make is corrupt."""
    import struct

    import lz4_ref
    good, content = dr.fixture_frames()["ext-0"]
    body = good[7:]  # blocks, end mark, content checksum

    def hdr(flg, bd, extra=b"", magic=lz4_ref.MAGIC):
        d = bytes([flg, bd]) + extra
        return struct.pack("<I", magic) + d + bytes([(lz4_ref.xxh32(d) >> 8) & 0xFF])

    cases = [
        (good, 0),
        (hdr(0x6C, 0x70, struct.pack("<Q", len(content))) + body, 0),              # content size, right
        (hdr(0x6C, 0x70, struct.pack("<Q", len(content) + 1)) + body, CDC_E_CORRUPT),
        (hdr(0x64, 0x40) + body, 0),                                                 # another block maximum
        (hdr(0x65, 0x70, b"\1\2\3\4") + body, CDC_E_UNSUPPORTED),                   # dictionary ID
        (hdr(0x44, 0x70) + body, CDC_E_UNSUPPORTED),                                 # linked blocks
        (struct.pack("<II", 0x184C2102, 5) + b"hello", CDC_E_UNSUPPORTED),           # legacy frame
        (struct.pack("<II", 0x184D2A53, 3) + b"abc", CDC_E_UNSUPPORTED),             # skippable frame
        (hdr(0xA4, 0x70) + body, CDC_E_CORRUPT),                                     # version 10
        (hdr(0x66, 0x70) + body, CDC_E_CORRUPT),                                     # reserved FLG bit
        (hdr(0x64, 0x71) + body, CDC_E_CORRUPT),                                     # reserved BD bit
        (hdr(0x64, 0x30) + body, CDC_E_CORRUPT),                                     # block maximum ID 3
        (good + b"\0", CDC_E_CORRUPT),                                               # a byte after the frame
        (good[:7] + struct.pack("<I", 0x80000000) + good[-4:], CDC_E_CORRUPT),       # a stored block of no bytes
        (good[:5], CDC_E_CORRUPT),
        (struct.pack("<I", 0x184C2102), CDC_E_UNSUPPORTED),                          # the legacy magic alone
        (good[:3], CDC_E_CORRUPT),
    ]
    blobs = [c[0] for c in cases]
    n_ok = sum(1 for c in cases if c[1] == 0)
    got, st, oo, host, cap = _device_decode(blobs, None, True, cap=n_ok * len(content))
    assert list(st) == [c[1] for c in cases]
    assert all(g == content for g, c in zip(got, cases) if c[1] == 0)
    _sentinels_intact(host, cap, cap)


def test_random_mutations_fail_or_decode_to_the_original():
    frame, content = dr.fixture_frames()["lz4f-0x7c"]
    blobs = dr.mutated_frames(64)
    cap = 64 * len(content)
    got, st, oo, host, _ = _device_decode(blobs, None, True, cap=cap)
    assert sum(1 for s in st if s) > 16, "the mutations should break most copies"
    for i, (g, s) in enumerate(zip(got, st)):
        if s == 0:
            assert g == content, i
        else:
            assert s in (CDC_E_CORRUPT, CDC_E_UNSUPPORTED), (i, s)
            assert oo[i + 1] == oo[i]
    # Every failure of this seed is decided while sizing (the frame has block
    # checksums, and no mutation touches only the content checksum), so nothing
    # is written past the final out_offsets[n].  A seed with a mutation that
    # only the content checksum catches would write that one blob's planned
    # bytes first: widen the bound by exactly that size then.
    _sentinels_intact(host, cap, int(oo[-1]))


def test_nospace_reports_the_size_and_writes_nothing_past_the_capacity():
    frames = dr.fixture_frames()
    blobs = [frames[n][0] for n in ("lz4f-0x64", "ext-1", "mixed")]
    want = [frames[n][1] for n in ("lz4f-0x64", "ext-1", "mixed")]
    total = sum(len(w) for w in want)
    with pytest.raises(_lib.CdcError) as e:
        _device_decode(blobs, None, True, cap=total - 1)
    assert e.value.status == CDC_E_NOSPACE and e.value.needed == total
    # the same call by hand, to look at the buffer afterwards
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    buf = torch.full((total + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.CdcError):
        decode.decode_device(base, offs[:-1], lens, buf[:total - 1], compressed=True)
    assert (buf.cpu().numpy()[total - 1:] == SENTINEL).all()
    got, st, oo, host, cap = _device_decode(blobs, None, True, cap=e.value.needed)
    assert (st == 0).all() and got == want


def test_check_blobs_finds_the_one_bad_checksum_and_the_one_bad_blob():
    frames = dr.fixture_frames()
    names = ["lz4f-0x64", "empty", "ext-0", "mixed", "lz4f-0x7c"]
    blobs = [dr.seal_stream(KEY, frames[n][0], 110 + i) for i, n in enumerate(names)]
    sums = [hashlib.sha256(frames[n][1]).digest() for n in names]
    assert (decode.check_blobs(blobs, sums, key=KEY) == 0).all()
    bad_sums = list(sums)
    bad_sums[2] = dr.flip(sums[2], 31)
    assert list(decode.check_blobs(blobs, bad_sums, key=KEY)) == [0, 0, CDC_E_MISMATCH, 0, 0]
    bad_blobs = list(blobs)
    bad_blobs[3] = dr.flip(blobs[3], 60 + 12 + 100)
    assert list(decode.DeviceDecoder(key=KEY).check_many(bad_blobs, sums)) == [0, 0, 0, CDC_E_AUTH, 0]
    wrong_empty = list(sums)
    wrong_empty[1] = sums[0]
    assert list(decode.check_blobs(blobs, wrong_empty, key=KEY)) == [0, CDC_E_MISMATCH, 0, 0, 0]


def test_backup_packfiles_read_back(tmp_path):
    files = [b"", dr.rnd(1000, 120), dr.rnd(200_000, 121), (b"plakar on the device " * 20000)[:300_001],
             dr.block_fixture() * 3]
    paths = []
    for i, b in enumerate(files):
        p = tmp_path / f"f{i}"
        p.write_bytes(b)
        paths.append(str(p))
    objs, packs, _ = snapshot.backup_files(paths, key=KEY, compression="LZ4")
    want = {}
    for f, o in zip(files, objs):
        off = 0
        for c in o.Chunks:
            want[c.Checksum] = f[off:off + c.Length]
            off += c.Length
    blobs, sums = [], []
    for pk in packs:
        p = pf.parse(pk)
        for t, c, o, n in p.index:
            blobs.append(bytes(p.blobs[o:o + n]))
            sums.append(c)
    assert set(sums) == set(want)
    plains = decode.decode_blobs(blobs, key=KEY)
    assert plains == [want[c] for c in sums]
    assert (decode.check_blobs(blobs, sums, key=KEY) == 0).all()
