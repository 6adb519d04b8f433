"""Encode, Decode and the blob check over more blobs than one tile of their
plan kernels: k_enc_plan scans 1,024 blobs per tile and carries the output
offset and the GCM piece base into the next, k_dec_plan gives each of its
1,024 threads ceil(n / 1024) blobs, k_dec_compact moves the survivors of a late
failure down.  Batches of 1,024, 1,025 and 2,049 small blobs, every output
through the host references (crypto_ref, zlib, liblz4), every decode into a
sentinel-filled buffer that is compared as a whole."""
import functools
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
import inflate_ref as ir  # noqa: E402
from plakar_amd import decode, encode  # noqa: E402
from plakar_amd._lib import CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_MISMATCH  # noqa: E402
from test_decode_gzip import _decode, _whole_buffer  # noqa: E402
from test_encode_gzip import KEY, _encode  # noqa: E402
from test_encode_gzip_large import PIECE, _hold  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 1024
COUNTS = (1024, 1025, 2049)
BIG_AT, BIG = 1030, 70_001     # a stream of two GCM pieces, whatever the form, past the first tile
# (name, the compress selector, sealed)
FORMS = [("gzip-sealed", "GZIP", True), ("gzip-plain", "GZIP", False), ("lz4-sealed", True, True),
         ("raw-sealed", False, True)]
DECODE_FORMS = [("gzip-plain", "GZIP", False), ("gzip-sealed", "GZIP", True), ("lz4-plain", True, False),
                ("lz4-sealed", True, True)]


@functools.lru_cache(None)
def _batch(n):
    """Blob i: (37 * i) % 301 bytes of zeros, text or random in turn; every
    97th is empty; the large one is random, so that no form shrinks it."""
    out = []
    for i in range(n):
        ln = 0 if i % 97 == 0 else (37 * i) % 301
        out.append(bytes(ln) if i % 3 == 0 else ir.text(ln, i) if i % 3 == 1 else ir.rnd(ln, i))
    if n > BIG_AT:
        out[BIG_AT] = ir.rnd(BIG, BIG_AT)
    assert sum(1 for b in out if not b) >= n // 97
    return out


@functools.lru_cache(None)
def _encoded(n, compress, sealed):
    """One cdc_encode_device call into a sentinel-filled buffer (_encode holds
    the margins and out_offsets: from 0, monotone, nothing written past the
    last one)."""
    return _encode(_batch(n), key=KEY if sealed else None, compress=compress)[0]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_encode_past_one_tile(form, n):
    _, compress, sealed = form
    blobs = _batch(n)
    enc = _encoded(n, compress, sealed)
    assert len(enc) == n
    frames = enc
    if sealed:
        frames = []
        for i, (e, b) in enumerate(zip(enc, blobs)):
            f = crypto_ref.decrypt_stream(KEY, e)[0]
            # a wrong piece base puts a stream's pieces, or their count, in another stream's place
            assert len(e) == 60 + len(f) + 28 * (-(-len(f) // PIECE)), f"blob {i}: sealed length"
            assert len(e) <= encode.encode_bound(len(b), compress, True), f"blob {i}: bound"
            frames.append(f)
        if n > BIG_AT:
            assert len(frames[BIG_AT]) > PIECE, "the large blob is a stream of two pieces"
    if compress == "GZIP":
        _hold(frames, blobs, form[0])
    else:
        for i, (f, b) in enumerate(zip(frames, blobs)):
            assert crypto_ref.decode(f, None, compress) == b, f"blob {i} ({len(b)} bytes)"
    assert n == TILE or frames[TILE:], "blobs of the second tile were read"


def _expect(blobs, want, status, key, compressed, scratch):
    """test_decode_gzip._expect with the selector: exact statuses, out_offsets
    the cumulative sizes of the survivors, the survivors back to back and
    byte-identical, nothing else written but the scratch of late failures."""
    total = sum(len(w) for w in want if w is not None)
    st, oo, host = _decode(blobs, key, total + scratch, compressed=compressed)
    bad = [i for i in range(len(blobs)) if st[i] != status[i]]
    assert not bad, [(i, int(st[i]), status[i]) for i in bad[:10]]
    sizes = [0 if w is None else len(w) for w in want]
    assert list(oo) == list(np.concatenate([[0], np.cumsum(sizes)])), "out_offsets"
    _whole_buffer(host, want, scratch)


@pytest.mark.parametrize("form", DECODE_FORMS, ids=[f[0] for f in DECODE_FORMS])
def test_decode_past_one_tile_with_failures(form):
    _, compress, sealed = form
    n = COUNTS[-1]
    blobs = list(_encoded(n, compress, sealed))
    want = list(_batch(n))
    status = [0] * n
    scratch = 0
    assert all(want[i] for i in (5, TILE, n - 1))
    if sealed:
        for i in (5, TILE, n - 1):          # a bit of the last record's tag
            blobs[i] = dr.flip(blobs[i], len(blobs[i]) - 1)
            status[i], want[i] = CDC_E_AUTH, None
    else:
        for i in (5, n - 1):                # refused while sizing: a header byte
            blobs[i] = dr.flip(blobs[i], 1)
            status[i], want[i] = CDC_E_CORRUPT, None
        # refused after its bytes were written: the CRC-32 of the trailer, the frame's content checksum
        at = len(blobs[TILE]) - 8 if compress == "GZIP" else len(blobs[TILE]) - 2
        blobs[TILE] = dr.flip(blobs[TILE], at, 3)
        scratch = len(want[TILE])
        status[TILE], want[TILE] = CDC_E_CORRUPT, None
    _expect(blobs, want, status, KEY if sealed else None, compress, scratch)


def test_decode_past_one_tile_whole():
    """Nothing damaged: 1,025 and 2,049 blobs, every form Decode reads."""
    for n in COUNTS[1:]:
        for _, compress, sealed in DECODE_FORMS + [("raw-sealed", False, True)]:
            _expect(list(_encoded(n, compress, sealed)), list(_batch(n)), [0] * n, KEY if sealed else None, compress, 0)


@pytest.mark.parametrize("form", [DECODE_FORMS[1], DECODE_FORMS[2]], ids=["gzip-sealed", "lz4-plain"])
def test_check_finds_the_one_wrong_checksum_past_one_tile(form):
    _, compress, sealed = form
    n = COUNTS[-1]
    sums = [hashlib.sha256(b).digest() for b in _batch(n)]
    sums[1500] = dr.flip(sums[1500], 31, 7)
    st = decode.check_blobs(list(_encoded(n, compress, sealed)), sums, key=KEY if sealed else None, compressed=compress)
    assert st[1500] == CDC_E_MISMATCH and list(np.flatnonzero(st)) == [1500]
