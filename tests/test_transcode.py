"""Transcode on the device (cdc_transcode_device) against libcrypto, liblz4 and
zlib, never against this library's own Encode or Decode: the re-key is
bit-exact to what libcrypto seals from the opened records (with `random` given
the output is fully determined), the other paths open and inflate to the
original bytes."""
import functools
import hashlib
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
from plakar_amd import _lib, sync  # noqa: E402
from plakar_amd._lib import CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_MISMATCH, CDC_E_NOSPACE  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_A = bytes(range(64, 96))
KEY_B = bytes(range(160, 192))
SENTINEL = 0xA5
SLACK = 4096
REC = 12 + 65536 + 16  # a full record


def _device_transcode(blobs, src, dst, in_offsets=None, cap=None, checksums=None, random=None):
    """One cdc_transcode_device call.  The blobs sit at in_offsets (default:
    packed) in a buffer of 0xEE pad bytes; d_out lies between sentinel slack
    on both sides.  Returns (outputs or None per blob, status, out_offsets,
    the whole output buffer on the host, cap)."""
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    if in_offsets is None:
        in_offsets = np.concatenate([[0], np.cumsum(lens)])[:-1]
    in_offsets = np.asarray(in_offsets, dtype=np.uint64)
    size = int(max([int(o) + len(b) for o, b in zip(in_offsets, blobs)] + [0])) + 16
    host_in = np.full(size, 0xEE, dtype=np.uint8)
    for o, b in zip(in_offsets, blobs):
        host_in[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    base = torch.from_numpy(host_in).cuda()
    assert base.data_ptr() % 256 == 0
    if cap is None:
        cap = int(lens.sum()) + 88 * len(blobs) + 28 * (int(lens.sum()) // 65536)
    buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    out = buf[SLACK:SLACK + cap]
    oo, st = sync.transcode_device(base, in_offsets, lens, out, src=src, dst=dst, checksums=checksums, random=random)
    host = buf.cpu().numpy()
    body = host[SLACK:]
    got = [None if st[i] else body[oo[i]:oo[i + 1]].tobytes() for i in range(len(blobs))]
    return got, st, oo, host, cap


def _sentinels_intact(host, cap, used):
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + used:] == SENTINEL).all(), "bytes past out_offsets[n] were written"


def _records(blob):
    """The records of an encrypted stream as their lengths give them: (nonce, sealed piece)."""
    out, pos = [], 60
    while pos < len(blob):
        rec = blob[pos:pos + REC]
        out.append((rec[:12], rec[12:]))
        pos += len(rec)
    return out


def _rnd_rows(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=56 * n, dtype=np.uint8).tobytes()


def _expected_rekey(blob, key_a, key_b, row):
    """What libcrypto makes of the re-key: the header sealed under key_b from
    the row of `random`, and every record's piece, opened with the source
    subkey, sealed under the new subkey with the data nonce XOR k."""
    sub_a = crypto_ref.gcm_open(key_a, blob[:12], blob[12:60])
    sub_b, n_b, dn = row[:32], row[32:44], row[44:56]
    out = bytearray(n_b + crypto_ref.gcm_seal(key_b, n_b, sub_b))
    for k, (nonce, sealed) in enumerate(_records(blob)):
        piece = crypto_ref.gcm_open(sub_a, nonce, sealed)
        nk = dn[:8] + (int.from_bytes(dn[8:], "big") ^ k).to_bytes(4, "big")
        out += nk + crypto_ref.gcm_seal(sub_b, nk, piece)
    return bytes(out)


EDGE_SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537, 131073]
# small blobs added after those, until the placement below has met every
# alignment pair: their lengths move the packed output offsets through every
# residue mod 4
FILL_SIZES = [1, 16, 2, 1024, 3, 17, 2048, 15]


@functools.lru_cache(None)
def _edge_batch():
    """(blobs, in_offsets, random): sealed by libcrypto under KEY_A, with the
    stream whose last record is an empty Seal after a full one, placed with
    pad bytes between them so that every pair (source ciphertext address mod
    4, destination ciphertext address mod 4) occurs, and whole aligned blocks
    (the kernel's 16-byte fast path) more than once."""
    blobs = [dr.seal_stream(KEY_A, dr.rnd(n, 400 + i), 500 + i) for i, n in enumerate(EDGE_SIZES)]
    full = dr.seal_stream(KEY_A, dr.rnd(65536, 390), 391)
    sub = crypto_ref.gcm_open(KEY_A, full[:12], full[12:60])
    n0 = bytes(range(100, 112))
    blobs.insert(13, full + n0 + crypto_ref.gcm_seal(sub, n0, b""))  # an empty Seal after a full record
    offs, seen, fast, pos, out_off, i = [], set(), 0, 3, 0, 0
    while i < len(blobs) or len(seen) < 16 or fast < 3:
        if i == len(blobs):
            blobs.append(dr.seal_stream(KEY_A, dr.rnd(FILL_SIZES[i % len(FILL_SIZES)], 400 + i), 500 + i))
        b = blobs[i]
        whole = len(b) > 88 and (min(len(b) - 60, REC) - 28) % 16 == 0  # its first record is whole blocks
        want = [c for c in range(4) if (c, out_off % 4) not in seen] or [0]
        c = 0 if whole and fast < 3 else want[0]
        while pos % 4 != c:
            pos += 1
        offs.append(pos)
        if len(b) > 88:
            seen.add((c, out_off % 4))
            fast += whole and c == 0
        pos += len(b) + 5
        out_off += len(b)
        i += 1
        assert i < 120, "the placement does not converge"
    return blobs, offs, _rnd_rows(len(blobs), 77)


def test_rekey_is_bit_exact_against_libcrypto():
    blobs, offs, rnd = _edge_batch()
    want = [_expected_rekey(b, KEY_A, KEY_B, rnd[56 * i:56 * i + 56]) for i, b in enumerate(blobs)]
    total = sum(len(b) for b in blobs)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (KEY_B, "LZ4"), in_offsets=offs, cap=total + 333,
                                               random=rnd)
    assert (st == 0).all(), st
    assert [int(oo[i + 1] - oo[i]) for i in range(len(blobs))] == [len(b) for b in blobs]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(blobs[i]))
    _sentinels_intact(host, cap, total)
    # the coverage this test is for: every pair of ciphertext alignments, the
    # 16-byte fast path and the slow path, and the empty trailing record
    pairs, fast, slow = set(), 0, 0
    for b, o, d in zip(blobs, offs, oo):
        for k, (_, sealed) in enumerate(_records(b)):
            m = len(sealed) - 16
            src_a, dst_a = (o + 60 + k * REC + 12) % 4, (SLACK + int(d) + 60 + k * REC + 12) % 4
            if m:
                pairs.add((src_a, dst_a))
            if src_a == 0 and m % 16 == 0 and m:
                fast += 1
            elif m:
                slow += 1
    assert len(pairs) == 16, sorted(pairs)
    assert fast >= 2 and slow >= 10, (fast, slow)
    assert any(len(_records(b)) == 2 and len(_records(b)[1][1]) == 16 for b in blobs)
    # and the new blobs open under the new key to what the old ones held
    for b, g in zip(blobs, got):
        assert crypto_ref.decrypt_stream(KEY_B, g)[0] == crypto_ref.decrypt_stream(KEY_A, b)[0]


def test_rekey_tampered_blobs_fail_and_contribute_nothing():
    plains = [dr.rnd(5000, 600), dr.rnd(3 * 65536 - 100, 601), dr.rnd(70000, 602), dr.rnd(300, 603),
              dr.rnd(65536 + 17, 604)]
    blobs = [dr.seal_stream(KEY_A, p, 610 + i) for i, p in enumerate(plains)]
    good = list(blobs)
    blobs[1] = dr.flip(blobs[1], 60 + REC + 12 + 4000, 3)      # a ciphertext bit in record 1 of 3
    blobs[2] = dr.flip(blobs[2], 60 + REC - 5, 6)              # a bit in record 0's tag
    blobs[3] = dr.flip(blobs[3], 20, 1)                        # a bit in the sealed subkey
    rnd = _rnd_rows(5, 78)
    total = sum(len(b) for b in blobs)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, None), (KEY_B, None), cap=total, random=rnd)
    assert list(st) == [0, CDC_E_AUTH, CDC_E_AUTH, CDC_E_AUTH, 0]
    assert list(oo) == [0, len(blobs[0])] + [len(blobs[0])] * 3 + [len(blobs[0]) + len(blobs[4])]
    assert got[0] == _expected_rekey(good[0], KEY_A, KEY_B, rnd[:56])
    assert got[4] == _expected_rekey(good[4], KEY_A, KEY_B, rnd[4 * 56:])
    # d_out[out_offsets[n], out_cap) is scratch after a failure; nothing outside d_out is
    assert (host[:SLACK] == SENTINEL).all() and (host[SLACK + cap:] == SENTINEL).all()


def test_rekey_wrong_key_and_malformed_lengths():
    plains = [dr.rnd(n, 620 + i) for i, n in enumerate([0, 100, 70000])]
    blobs = [dr.seal_stream(KEY_A, p, 630 + i) for i, p in enumerate(plains)]
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_B, "LZ4"), (KEY_A, "LZ4"), random=_rnd_rows(3, 79))
    assert list(st) == [CDC_E_AUTH] * 3 and list(oo) == [0] * 4 and got == [None] * 3
    assert (host[:SLACK] == SENTINEL).all() and (host[SLACK + cap:] == SENTINEL).all()
    # lengths no writer produces, between two good blobs
    ok = blobs[1]
    batch = [ok, ok[:59], ok[:60 + 12], ok[:60 + 27], blobs[2]]
    rnd = _rnd_rows(5, 80)
    got, st, oo, host, cap = _device_transcode(batch, (KEY_A, "LZ4"), (KEY_B, "LZ4"), random=rnd,
                                               cap=len(ok) + len(blobs[2]))
    assert list(st) == [0, CDC_E_CORRUPT, CDC_E_CORRUPT, CDC_E_CORRUPT, 0]
    assert got[0] == _expected_rekey(ok, KEY_A, KEY_B, rnd[:56])
    assert got[4] == _expected_rekey(blobs[2], KEY_A, KEY_B, rnd[4 * 56:])
    _sentinels_intact(host, cap, len(ok) + len(blobs[2]))


def test_rekey_nospace_reports_the_need_and_writes_nothing():
    blobs = [dr.seal_stream(KEY_A, dr.rnd(n, 640 + i), 650 + i) for i, n in enumerate([100, 65537, 0, 2048])]
    total = sum(len(b) for b in blobs)
    rnd = _rnd_rows(4, 81)
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    base = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    buf = torch.full((SLACK + total + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.CdcError) as e:
        sync.transcode_device(base, offs, lens, buf[SLACK:SLACK + total - 1], src=(KEY_A, "LZ4"), dst=(KEY_B, "LZ4"),
                              random=rnd)
    assert e.value.status == CDC_E_NOSPACE and e.value.needed == total
    assert (buf.cpu().numpy() == SENTINEL).all(), "a call that reported CDC_E_NOSPACE wrote something"
    oo, st = sync.transcode_device(base, offs, lens, buf[SLACK:SLACK + total], src=(KEY_A, "LZ4"), dst=(KEY_B, "LZ4"),
                                   random=rnd)
    assert (st == 0).all() and oo[-1] == total
    host = buf.cpu().numpy()
    for i, b in enumerate(blobs):
        assert host[SLACK + oo[i]:SLACK + oo[i + 1]].tobytes() == _expected_rekey(b, KEY_A, KEY_B, rnd[56 * i:56 * i + 56])
    _sentinels_intact(host, total, total)


def test_rekey_batch_of_1500_small_blobs():
    n = 1500  # earlier plan kernels had an edge at 1,024 blobs
    blobs = [dr.seal_stream(KEY_A, dr.rnd(16, 1000 + i), 3000 + i) for i in range(n)]
    rnd = _rnd_rows(n, 82)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "GZIP"), (KEY_B, "GZIP"), random=rnd, cap=n * 104)
    assert (st == 0).all() and oo[-1] == n * 104
    for i in (0, 1, 63, 64, 1023, 1024, 1025, 1499):
        assert got[i] == _expected_rekey(blobs[i], KEY_A, KEY_B, rnd[56 * i:56 * i + 56]), i
    subs = {}
    for i, g in enumerate(got):  # every blob opens under the new key, with its own row of random
        assert g[:12] == rnd[56 * i + 32:56 * i + 44] and g[60:72] == rnd[56 * i + 44:56 * i + 56], i
        plain, sub, _ = crypto_ref.decrypt_stream(KEY_B, g)
        assert plain == dr.rnd(16, 1000 + i) and sub == rnd[56 * i:56 * i + 32], i
        subs[sub] = i
    assert len(subs) == n
    _sentinels_intact(host, cap, n * 104)


# ---- the paths that take an envelope off or put one on ---------------------------------------

SOME_SIZES = [0, 1, 16, 1025, 65536, 65537, 131073]


def test_key_to_none_equals_the_reference_open():
    plains = [dr.rnd(n, 700 + i) for i, n in enumerate(SOME_SIZES)]
    blobs = [dr.seal_stream(KEY_A, p, 710 + i) for i, p in enumerate(plains)]
    for b, p in zip(blobs, plains):
        assert crypto_ref.decrypt_stream(KEY_A, b)[0] == p
    total = sum(len(p) for p in plains)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (None, "LZ4"), cap=total)
    assert (st == 0).all() and got == plains and oo[-1] == total
    assert [len(g) for g in got] == [sync.transcode_size(len(b), True, False) for b in blobs]
    _sentinels_intact(host, cap, total)


def test_none_to_key_opens_to_the_stored_bytes():
    stored = [dr.rnd(n, 720 + i) for i, n in enumerate(SOME_SIZES)]
    rnd = _rnd_rows(len(stored), 83)
    got, st, oo, host, cap = _device_transcode(stored, (None, "GZIP"), (KEY_B, "GZIP"), random=rnd)
    assert (st == 0).all()
    for i, (g, p) in enumerate(zip(got, stored)):
        plain, sub, nonce = crypto_ref.decrypt_stream(KEY_B, g)
        assert plain == p and sub == rnd[56 * i:56 * i + 32] and nonce == rnd[56 * i + 32:56 * i + 44]
        assert len(g) == sync.transcode_size(len(p), False, True)
    _sentinels_intact(host, cap, int(oo[-1]))


def test_no_key_on_either_side_is_a_copy():
    stored = [dr.rnd(n, 730 + i) for i, n in enumerate([0, 3, 4097, 70001])]
    got, st, oo, host, cap = _device_transcode(stored, (None, "LZ4"), (None, "LZ4"), in_offsets=[1, 7, 30, 4200],
                                               cap=sum(map(len, stored)))
    assert (st == 0).all() and got == stored
    _sentinels_intact(host, cap, int(oo[-1]))


# ---- the re-encode path -------------------------------------------------------------------------

@functools.lru_cache(None)
def _contents():
    frames = dr.fixture_frames()
    out = [c for _, c in frames.values() if c is not None]
    text = (b"the quick brown fox jumps over the lazy dog, again and again. " * 4000)[:200 * 1024]
    return out + [text]


def _gzip(data):
    if not data:
        return b""  # DeflateStream of empty input is an empty stream
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def _stored(content, compression, key, seed):
    """A blob as a repository with this codec stores it, made by liblz4 / zlib / libcrypto."""
    body = content if compression is None else _gzip(content) if compression == "GZIP" else \
        (dr.lz4f_compress(content) if content else b"")
    return dr.seal_stream(key, body, seed) if key is not None else body


def _read_back(blob, compression, key):
    body = crypto_ref.decrypt_stream(key, blob)[0] if key is not None else blob
    if compression is None:
        return body
    if not body:
        return b""
    return zlib.decompress(body, 31) if compression == "GZIP" else crypto_ref.lz4f_decompress(body)


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keys"])
@pytest.mark.parametrize("conv", [("LZ4", "GZIP"), ("GZIP", "LZ4"), (None, "LZ4")], ids=lambda c: f"{c[0]}-{c[1]}")
def test_reencode_reads_back_through_the_system_libraries(conv, keyed):
    sc, dc = conv
    ka, kb = (KEY_A, KEY_B) if keyed else (None, None)
    contents = _contents()
    blobs = [_stored(c, sc, ka, 800 + i) for i, c in enumerate(contents)]
    for b, c in zip(blobs, contents):
        assert _read_back(b, sc, ka) == c
    cap = sum(len(c) + len(c) // 8 + 4096 for c in contents)
    got, st, oo, host, cap = _device_transcode(blobs, (ka, sc), (kb, dc), cap=cap)
    assert (st == 0).all(), st
    for i, (g, c) in enumerate(zip(got, contents)):
        assert _read_back(g, dc, kb) == c, i
        if keyed:
            with pytest.raises(ValueError):
                crypto_ref.decrypt_stream(ka, g)
    _sentinels_intact(host, cap, int(oo[-1]))


def test_reencode_corrupt_frames_get_their_status_and_no_empty_blob():
    frames, bad = dr.fixture_frames(), dr.corrupt_frames()
    good = [frames["mixed"], frames["ext-0"], frames["many-blocks"]]
    # bad-magic fails in the sizing pass, bad-content-checksum after its range was written
    bodies = [good[0][0], bad["bad-magic"], good[1][0], bad["bad-content-checksum"], good[2][0]]
    blobs = [dr.seal_stream(KEY_A, f, 820 + i) for i, f in enumerate(bodies)]
    rnd = _rnd_rows(5, 84)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (KEY_B, "GZIP"), random=rnd, cap=1 << 20)
    assert list(st) == [0, CDC_E_CORRUPT, 0, CDC_E_CORRUPT, 0]
    assert oo[1] == oo[2] and oo[3] == oo[4]
    for i, (_, content) in zip((0, 2, 4), good):
        assert _read_back(got[i], "GZIP", KEY_B) == content
        # each survivor carries its own row of random, whatever failed before it
        assert crypto_ref.decrypt_stream(KEY_B, got[i])[1] == rnd[56 * i:56 * i + 32]
    # no 60-byte encoding of an empty blob stands in a failed blob's place
    assert int(oo[-1]) == sum(len(got[i]) for i in (0, 2, 4)) and all(len(got[i]) > 60 for i in (0, 2, 4))
    _sentinels_intact(host, cap, int(oo[-1]))


@pytest.mark.parametrize("dst", [(KEY_B, "LZ4"), (KEY_B, "GZIP"), (None, "LZ4")], ids=["rekey", "reencode", "open"])
def test_checksums_leave_a_mismatching_blob_out(dst):
    frames = dr.fixture_frames()
    picks = [frames[n] for n in ("mixed", "ext-0", "empty", "ext-1", "many-blocks")]
    blobs = [dr.seal_stream(KEY_A, f, 840 + i) for i, (f, _) in enumerate(picks)]
    sums = [hashlib.sha256(c).digest() for _, c in picks]
    sums[3] = hashlib.sha256(b"something else").digest()
    rnd = _rnd_rows(5, 85)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), dst, checksums=sums, random=rnd, cap=1 << 20)
    assert list(st) == [0, 0, 0, CDC_E_MISMATCH, 0]
    assert oo[3] == oo[4]
    for i in (0, 1, 2, 4):
        if dst == (KEY_B, "LZ4"):  # the re-key is still exact, with blob i's own row of random
            assert got[i] == _expected_rekey(blobs[i], KEY_A, KEY_B, rnd[56 * i:56 * i + 56])
        elif dst[0] is None:
            assert got[i] == picks[i][0]  # the frame itself, carried over
        assert _read_back(got[i], dst[1], dst[0]) == picks[i][1]
    _sentinels_intact(host, cap, int(oo[-1]))
    # without the checksums the envelope is all that is checked: every blob passes
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), dst, random=rnd, cap=1 << 20)
    assert (st == 0).all()


def test_transcode_blobs_convenience():
    contents = [b"", b"abc" * 1000, dr.rnd(70000, 860)]
    blobs = [_stored(c, "LZ4", KEY_A, 870 + i) for i, c in enumerate(contents)]
    blobs.insert(1, dr.flip(blobs[1], 70))
    out = sync.transcode_blobs(blobs, src=(KEY_A, "LZ4"), dst=(KEY_B, "GZIP"))
    assert isinstance(out[1], sync.TranscodeError) and out[1].status == CDC_E_AUTH
    assert [_read_back(out[i], "GZIP", KEY_B) for i in (0, 2, 3)] == contents
    assert sync.transcode_blobs([]) == []
