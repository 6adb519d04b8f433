"""The persistent GCM kernels (k_gcm of Encode, k_rec_open of Decode, k_rekey
of Transcode) with more records than they have waves, so that every wave goes
round its ticket loop again and rewrites its key tables in LDS for a record of
another blob; k_tc_compact when a blob's new place overlaps its old one; and
blobs of more than 256 records, where the data nonce XOR k changes more than
its last byte.

Every reference is libcrypto, liblz4 or zlib (crypto_ref, decode_ref), never
this library's own Encode or Decode.  Every output blob of every call is
compared, and every call writes into a sentinel-filled buffer whose margins
are checked."""
import ctypes
import functools
import hashlib
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
import inflate_ref as ir  # noqa: E402
from plakar_amd import decode, encode  # noqa: E402
from plakar_amd._lib import CDC_E_AUTH, CDC_E_MISMATCH  # noqa: E402
from test_decode_gzip import _decode, _whole_buffer  # noqa: E402
from test_transcode import (KEY_A, KEY_B, REC, SENTINEL, SLACK, _device_transcode, _expected_rekey, _records,  # noqa: E402
                            _rnd_rows, _sentinels_intact)

pytestmark = pytest.mark.gpu

PIECE = 65536
GCM_WAVES = 12    # k_gcm and k_rec_open: waves per workgroup, one workgroup per CU
REKEY_WAVES = 8   # k_rekey
EXTRA = 513       # records past twice the waves


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _waves():
    """W: the most waves k_gcm or k_rec_open can have on this device."""
    return GCM_WAVES * _cus()


def _nonce(dn, k):
    """Encode's rule for record k: the data nonce with its last four bytes XOR k."""
    return dn[:8] + (int.from_bytes(dn[8:], "big") ^ k).to_bytes(4, "big")


def _seal_with_row(key, row, body):
    """What libcrypto makes of Encode's sealing with this row of `random`."""
    sub, n0, dn = row[:32], row[32:44], row[44:56]
    out = bytearray(n0 + crypto_ref.gcm_seal(key, n0, sub))
    for k in range(-(-len(body) // PIECE)):
        nk = _nonce(dn, k)
        out += nk + crypto_ref.gcm_seal(sub, nk, body[k * PIECE:(k + 1) * PIECE])
    return bytes(out)


def _row(rows, i):
    return rows[56 * i:56 * i + 56]


_lz4_out = ctypes.create_string_buffer(4 * PIECE)


def _lz4f_read(frame):
    """liblz4's LZ4F_decompress of one whole frame of at most 256 KiB of
    content (crypto_ref.lz4f_decompress with one shared output buffer: that
    one allocates 4 MiB per call, too slow for thousands of small frames)."""
    L = crypto_ref.lz4()
    ctx = ctypes.c_void_p()
    assert L.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100) == 0
    try:
        src = ctypes.create_string_buffer(bytes(frame), len(frame))
        pos, out = 0, bytearray()
        while True:
            dst_n, src_n = ctypes.c_size_t(len(_lz4_out)), ctypes.c_size_t(len(frame) - pos)
            r = L.LZ4F_decompress(ctx, ctypes.addressof(_lz4_out), ctypes.byref(dst_n), ctypes.addressof(src) + pos,
                                  ctypes.byref(src_n), None)
            if L.LZ4F_isError(r):
                raise ValueError("LZ4F: " + L.LZ4F_getErrorName(r).decode())
            out += ctypes.string_at(_lz4_out, dst_n.value)
            pos += src_n.value
            if r == 0:
                break
            if src_n.value == 0 and dst_n.value == 0:
                raise ValueError("LZ4F: truncated frame")
        if pos != len(frame):
            raise ValueError(f"LZ4F: {len(frame) - pos} trailing bytes")
        return bytes(out)
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


# ---- 1. more records than waves ---------------------------------------------------------------
def _length(i):
    if i % 64 == 7:
        return PIECE + (37 * i) % 3000     # a full record and a short tail
    if i % 64 == 39:
        return 2 * PIECE                   # two full records
    if i % 97 == 0:
        return 0                           # the 60-byte envelope alone: it shares its rec0 with its neighbour
    return 1 + (131 * i) % 2100


@functools.lru_cache(None)
def _contents(w):
    """Blobs until they hold 2 w + 513 pieces of 64 KiB.  Each has its own
    seed; a third of the small ones is text, so that a compressed frame differs
    in length from its content, and the two-piece blobs are random, so that no
    form has fewer records than this count."""
    out, pieces, i = [], 0, 0
    while pieces < 2 * w + EXTRA:
        n = _length(i)
        out.append(ir.text(n, i) if n < PIECE and i % 3 == 1 else dr.rnd(n, 20_000 + i))
        pieces += -(-n // PIECE)
        i += 1
    assert sum(1 for c in out if not c) >= len(out) // 100   # every 97th, but for those that are two-piece blobs
    return out


@functools.lru_cache(None)
def _stored(w, form):
    """The batch as a repository stores it, sealed by libcrypto under KEY_A
    with a subkey and nonces of each blob's own: "raw" seals the contents,
    "lz4" the frames that liblz4 makes of them."""
    bodies = _contents(w)
    if form == "lz4":
        bodies = [dr.lz4f_compress(c) if c else b"" for c in bodies]
    return [dr.seal_stream(KEY_A, b, 40_000 + i) for i, b in enumerate(bodies)]


def _rec0(blobs):
    """rec0 of every blob, and the record count after the last."""
    return np.concatenate([[0], np.cumsum([len(_records(b)) for b in blobs])])


def _premise(records, w):
    """More than two records per wave: at least w + 513 of them are taken by a
    wave that has already had one, whatever the scheduling."""
    print(f"{_cus()} CUs, W = {w} waves, {records} records")
    assert records >= 2 * w + EXTRA and records > 2 * w, (records, w, _cus())


@functools.lru_cache(None)
def _rows(w):
    return _rnd_rows(len(_contents(w)), 91)


@functools.lru_cache(None)
def _rekeyed(w):
    """The expected re-key of every blob of the raw-sealed batch."""
    rows = _rows(w)
    return [_expected_rekey(b, KEY_A, KEY_B, _row(rows, i)) for i, b in enumerate(_stored(w, "raw"))]


def test_rekey_more_records_than_waves():
    w = _waves()
    blobs, rows, want = _stored(w, "raw"), _rows(w), _rekeyed(w)
    _premise(int(_rec0(blobs)[-1]), w)
    total = sum(len(b) for b in blobs)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (KEY_B, "LZ4"), cap=total + 333, random=rows)
    assert not st.any(), [(int(i), int(st[i])) for i in np.flatnonzero(st)[:10]]
    assert list(oo) == list(np.concatenate([[0], np.cumsum([len(b) for b in blobs])])), "out_offsets"
    bad = [i for i, (g, x) in enumerate(zip(got, want)) if g != x]
    assert not bad, f"{len(bad)} blobs differ from libcrypto's re-key, the first: {bad[:10]}"
    _sentinels_intact(host, cap, total)


def _kept_base():
    return REKEY_WAVES * _cus() + 1


@functools.lru_cache(None)
def _one_record_blobs(n):
    """n blobs of one record each, 16 to 300 bytes, and their expected re-key."""
    blobs = [dr.seal_stream(KEY_A, dr.rnd(16 + (53 * i) % 285, 60_000 + i), 70_000 + i) for i in range(n)]
    rows = _rnd_rows(n, 92)
    return blobs, rows, [_expected_rekey(b, KEY_A, KEY_B, _row(rows, i)) for i, b in enumerate(blobs)]


@pytest.mark.parametrize("count", ["CUs-1", "CUs", "CUs+1", "8CUs", "8CUs+1"])
def test_rekey_kept_waves(count):
    """k_rekey keeps ceil(records / workgroups) waves of each workgroup: one
    at the first two counts, two at CUs + 1, all eight at 8 CUs, and at
    8 CUs + 1 all eight with one record left for a second round."""
    cus = _cus()
    n = {"CUs-1": cus - 1, "CUs": cus, "CUs+1": cus + 1, "8CUs": REKEY_WAVES * cus, "8CUs+1": REKEY_WAVES * cus + 1}[count]
    blobs, rows, want = _one_record_blobs(_kept_base())
    blobs, rows, want = blobs[:n], rows[:56 * n], want[:n]
    assert all(len(_records(b)) == 1 and 16 + 88 <= len(b) <= 300 + 88 for b in blobs)
    total = sum(len(b) for b in blobs)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (KEY_B, "LZ4"), cap=total + 333, random=rows)
    assert not st.any(), [(int(i), int(st[i])) for i in np.flatnonzero(st)[:10]]
    assert list(oo) == list(np.concatenate([[0], np.cumsum([len(b) for b in blobs])])), "out_offsets"
    bad = [i for i, (g, x) in enumerate(zip(got, want)) if g != x]
    assert not bad, f"{len(bad)} of {n} blobs differ from libcrypto's re-key, the first: {bad[:10]}"
    _sentinels_intact(host, cap, total)


def _encode_rows(blobs, compress, rows, key=KEY_A):
    """One cdc_encode_device call with `random` given, over the blobs laid back
    to back after one odd byte, into the middle of a sentinel-filled buffer:
    the encoded blobs.  Nothing outside the returned offsets may be written."""
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = 1 + np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"\xEE" + b"".join(blobs) + b"\xEE", dtype=np.uint8).copy()).cuda()
    cap = sum(encode.encode_bound(len(b), compress, True) for b in blobs)
    buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(base, offs[:-1], lens, buf[SLACK:SLACK + cap], key=key, compress=compress, random=rows)
    host = buf.cpu().numpy()
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + int(oo[-1]):] == SENTINEL).all(), "bytes past the last output offset were written"
    assert oo[0] == 0 and (np.diff(oo) >= 0).all()
    return [host[SLACK + oo[i]:SLACK + oo[i + 1]].tobytes() for i in range(len(blobs))]


def test_encode_raw_sealed_more_records_than_waves():
    """With `random` given the sealed output is determined: libcrypto's, byte for byte."""
    w = _waves()
    contents, rows = _contents(w), _rows(w)
    _premise(sum(-(-len(c) // PIECE) for c in contents), w)
    got = _encode_rows(contents, False, rows)
    bad = [i for i, (g, c) in enumerate(zip(got, contents)) if g != _seal_with_row(KEY_A, _row(rows, i), c)]
    assert not bad, f"{len(bad)} blobs differ from libcrypto's sealing, the first: {bad[:10]}"


@pytest.mark.parametrize("form", [True, "GZIP"], ids=["lz4-sealed", "gzip-sealed"])
def test_encode_compressed_sealed_more_records_than_waves(form):
    """The frame is the device's own, so the check is structural: the header
    sealed from the row, record k under the data nonce XOR k, every record
    opened by libcrypto, the frame read back by liblz4 / zlib."""
    w = _waves()
    contents, rows = _contents(w), _rows(w)
    got = _encode_rows(contents, form, rows)
    records = shrunk = 0
    for i, (g, c) in enumerate(zip(got, contents)):
        sub, n0, dn = _row(rows, i)[:32], _row(rows, i)[32:44], _row(rows, i)[44:56]
        assert g[:60] == n0 + crypto_ref.gcm_seal(KEY_A, n0, sub), f"blob {i}: header"
        frame = bytearray()
        for k, (nonce, sealed) in enumerate(_records(g)):
            assert nonce == _nonce(dn, k), f"blob {i} record {k}: nonce"
            try:
                frame += crypto_ref.gcm_open(sub, nonce, sealed)
            except ValueError:
                raise AssertionError(f"blob {i} ({len(c)} bytes) record {k}: GCM tag mismatch") from None
            records += 1
        assert len(g) == 60 + len(frame) + 28 * (-(-len(frame) // PIECE)), f"blob {i}: sealed length"
        if not c:
            assert not frame, f"blob {i}: an empty blob is an empty stream"
        elif form == "GZIP":
            assert zlib.decompress(bytes(frame), 31) == c, f"blob {i} ({len(c)} bytes): zlib"
        else:
            assert _lz4f_read(frame) == c, f"blob {i} ({len(c)} bytes): liblz4"
        shrunk += len(c) >= 1000 and len(frame) < len(c)
    _premise(records, w)
    # a sixth of the blobs is 1,000 bytes or more of text from sixteen words, which any LZ77 coder shortens
    assert shrunk > len(contents) // 10, "the text blobs' frames are shorter than their contents"


DECODE_FORMS = [("raw", False), ("lz4", True)]
DECODE_IDS = ["raw-sealed", "lz4-sealed"]


@pytest.mark.parametrize("form", DECODE_FORMS, ids=DECODE_IDS)
def test_decode_more_records_than_waves(form):
    """Raw-sealed: k_rec_open's hash pass, then its pass into d_out.
    LZ4-sealed: its one pass into the frame slots, liblz4's frames after it."""
    name, compressed = form
    w = _waves()
    blobs, want = _stored(w, name), _contents(w)
    _premise(int(_rec0(blobs)[-1]), w)
    st, oo, host = _decode(blobs, KEY_A, sum(len(c) for c in want), compressed=compressed)
    assert not st.any(), [(int(i), int(st[i])) for i in np.flatnonzero(st)[:10]]
    assert list(oo) == list(np.concatenate([[0], np.cumsum([len(c) for c in want])])), "out_offsets"
    _whole_buffer(host, want)


@pytest.mark.parametrize("form", DECODE_FORMS, ids=DECODE_IDS)
def test_decode_more_records_than_waves_three_tampered(form):
    """A tag bit in an early blob, in a two-record blob whose records lie past
    ticket W and in the last blob with a record: those three are CDC_E_AUTH,
    the others come out packed, and nothing is written after them (d_out holds
    the survivors exactly)."""
    name, compressed = form
    w = _waves()
    blobs, want = list(_stored(w, name)), list(_contents(w))
    rec0 = _rec0(blobs)
    n = len(blobs)
    past = next(i for i in range(n) if rec0[i] > w and rec0[i + 1] - rec0[i] >= 2)
    last = max(i for i in range(n) if rec0[i + 1] > rec0[i])
    assert 5 < past < last and rec0[6] > rec0[5] and rec0[5] < w
    status = [0] * n
    for i in (5, past, last):
        blobs[i] = dr.flip(blobs[i], len(blobs[i]) - 1)   # the last record's tag
        status[i], want[i] = CDC_E_AUTH, None
    st, oo, host = _decode(blobs, KEY_A, sum(len(c) for c in want if c is not None), compressed=compressed)
    bad = [i for i in range(n) if st[i] != status[i]]
    assert not bad, [(i, int(st[i]), status[i]) for i in bad[:10]]
    sizes = [0 if c is None else len(c) for c in want]
    assert list(oo) == list(np.concatenate([[0], np.cumsum(sizes)])), "out_offsets"
    _whole_buffer(host, want)


def test_check_finds_the_one_wrong_checksum_past_the_waves():
    w = _waves()
    blobs, contents = _stored(w, "lz4"), _contents(w)
    sums = [hashlib.sha256(c).digest() for c in contents]
    at = next(i for i in range(w + 101, len(blobs)) if contents[i])
    sums[at] = dr.flip(sums[at], 31, 7)
    st = decode.check_blobs(blobs, sums, key=KEY_A, compressed=True)
    assert st[at] == CDC_E_MISMATCH and list(np.flatnonzero(st)) == [at]


# ---- 2. k_tc_compact when the move overlaps -----------------------------------------------------
def _compacted(payloads, damage, seed):
    """One re-key call over blobs of these payload lengths, sealed under
    KEY_A, blob i damaged by damage[i] = (offset, bit) (a negative offset
    counts from the blob's end).  Holds the call to: CDC_E_AUTH for exactly
    the damaged blobs, out_offsets the running sum of the survivors' lengths,
    every survivor libcrypto's re-key under its own row, nothing written
    outside d_out (d_out[out_offsets[n], out_cap) is scratch after a failure).
    Returns the blobs' stored lengths."""
    good = [dr.seal_stream(KEY_A, dr.rnd(p, seed + i), seed + 500 + i) for i, p in enumerate(payloads)]
    assert [len(g) for g in good] == [60 + p + 28 * (-(-p // PIECE)) for p in payloads]
    blobs = list(good)
    for i, (at, bit) in damage.items():
        blobs[i] = dr.flip(good[i], at if at >= 0 else len(good[i]) + at, bit)
    n = len(blobs)
    rows = _rnd_rows(n, seed)
    total = sum(len(b) for b in blobs)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (KEY_B, "LZ4"), cap=total, random=rows)
    assert list(st) == [CDC_E_AUTH if i in damage else 0 for i in range(n)]
    assert list(oo) == list(np.concatenate([[0], np.cumsum([0 if i in damage else len(b) for i, b in enumerate(blobs)])]))
    for i in range(n):
        if i not in damage:
            assert got[i] == _expected_rekey(good[i], KEY_A, KEY_B, _row(rows, i)), \
                f"blob {i} ({len(good[i])} stored bytes, moved down by {sum(len(blobs[j]) for j in damage if j < i)})"
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + cap:] == SENTINEL).all(), "bytes past out_cap were written"
    return [len(b) for b in blobs]


SUBKEY = (20, 1)               # a bit of the sealed subkey: k_tc_keys reports it
TAG = (-5, 6)                  # a bit of the last record's tag: k_rekey reports it
MIDDLE = (60 + REC + 12 + 4000, 3)   # a ciphertext bit in record 1


def test_compact_moves_that_overlap_by_less_than_a_piece():
    """Every survivor's new place overlaps its old one.  The shifts: 89 (no
    multiple of 4, less than a 4-KiB piece) under a three-record blob, then
    149 under stored lengths that end in the tail byte loop, fill a piece's
    256 lanes exactly and cross the piece boundary, then more under two
    failures side by side, a three-record blob that failed in its middle
    record after the others were written, and a failed last blob."""
    payloads = [1, 3 * PIECE - 19,                      # 0 fails; a three-record survivor directly after it
                0, 4007, 4008, 4009, 8104, 8105,        # 2 fails
                300, PIECE + 4464, 5000,                # 8 and 9 fail side by side
                3 * PIECE - 100, 2 * PIECE + 1, 777,    # 11 fails in its middle record
                1234]                                   # the last one fails
    damage = {0: TAG, 2: SUBKEY, 8: SUBKEY, 9: MIDDLE, 11: MIDDLE, 14: TAG}
    lens = _compacted(payloads, damage, 5000)
    assert lens[0] == 89 and lens[2] == 60 and lens[3:8] == [4095, 4096, 4097, 8192, 8193]
    assert (lens[1] - 60) // REC == 2 and (lens[11] - 60) // REC == 2, "three records each"


def test_compact_moves_by_exactly_one_piece():
    """The first failure has 4,096 stored bytes, so the blobs after it move
    down by one whole piece; later a middle-record failure and a failed last
    blob with a tampered subkey."""
    payloads = [100, 4008, 3 * PIECE + 7, 4009, 3 * PIECE - 1, 2 * PIECE, 0]
    damage = {1: TAG, 4: MIDDLE, 6: SUBKEY}
    lens = _compacted(payloads, damage, 6000)
    assert lens[1] == 4096


def test_compact_moves_every_blob_of_the_large_batch():
    """Blob 3's tag fails: the thousands of blobs after it move down by its
    length, each move overlapping."""
    w = _waves()
    blobs, rows, want = list(_stored(w, "raw")), _rows(w), _rekeyed(w)
    n = len(blobs)
    assert 88 < len(blobs[3]) < 4096
    blobs[3] = dr.flip(blobs[3], len(blobs[3]) - 5, 6)
    total = sum(len(b) for b in blobs)
    got, st, oo, host, cap = _device_transcode(blobs, (KEY_A, "LZ4"), (KEY_B, "LZ4"), cap=total, random=rows)
    assert list(np.flatnonzero(st)) == [3] and st[3] == CDC_E_AUTH
    assert list(oo) == list(np.concatenate([[0], np.cumsum([0 if i == 3 else len(b) for i, b in enumerate(blobs)])]))
    bad = [i for i in range(n) if i != 3 and got[i] != want[i]]
    assert not bad, f"{len(bad)} of {n - 1} survivors differ from libcrypto's re-key, the first: {bad[:10]}"
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + cap:] == SENTINEL).all(), "bytes past out_cap were written"


# ---- 3. k past 255 ---------------------------------------------------------------------------------
BIG = 257 * PIECE + 5   # 258 records


@functools.lru_cache(None)
def _big():
    """(content, the blob sealed by libcrypto under KEY_A, one row of random)."""
    content = dr.rnd(BIG, 80_000)
    return content, dr.seal_stream(KEY_A, content, 80_001), _rnd_rows(1, 93)


def _nonces_past_255(blob, dn):
    """Records 255, 256 and 257 carry the data nonce XOR k: k = 255 changes
    byte 11 alone, 256 byte 10 alone, 257 both.  (Bytes 0 to 9 never change.)"""
    recs = _records(blob)
    assert len(recs) == 258
    for k in (255, 256, 257):
        nonce = recs[k][0]
        assert nonce == _nonce(dn, k), f"record {k}: nonce"
        assert nonce[:10] == dn[:10]
        assert (nonce[10] != dn[10]) == (k >= 256) and (nonce[11] != dn[11]) == (k != 256), f"record {k}"
    assert recs[257][0][10] == dn[10] ^ 1 and recs[257][0][11] == dn[11] ^ 1
    assert recs[256][0][10] == dn[10] ^ 1 and recs[255][0][11] == dn[11] ^ 0xFF


def test_rekey_of_258_records():
    _, blob, row = _big()
    got, st, oo, host, cap = _device_transcode([blob], (KEY_A, "LZ4"), (KEY_B, "LZ4"), cap=len(blob) + 333, random=row)
    assert list(st) == [0] and list(oo) == [0, len(blob)]
    _nonces_past_255(got[0], row[44:56])
    assert got[0] == _expected_rekey(blob, KEY_A, KEY_B, row)
    _sentinels_intact(host, cap, len(blob))


def test_encode_raw_sealed_of_258_records():
    content, _, row = _big()
    (got,) = _encode_rows([content], False, row)
    _nonces_past_255(got, row[44:56])
    assert got == _seal_with_row(KEY_A, row, content)


def test_decode_raw_sealed_of_258_records():
    content, blob, _ = _big()
    st, oo, host = _decode([blob], KEY_A, len(content), compressed=False)
    assert list(st) == [0] and list(oo) == [0, len(content)]
    _whole_buffer(host, [content])
