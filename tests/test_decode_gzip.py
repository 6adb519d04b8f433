"""GZIP Decode on the device (cdc_decode_device / cdc_check_device with
compressed = CDC_COMPRESS_GZIP) against zlib and inflate_ref: what zlib writes,
the hand-made fixtures, the named corruptions, seeded mutations, the CRC-32's
slice boundaries, space and late failures, the blob check and the selector.
Every call decodes into a sentinel-filled buffer that is compared as a whole."""
import functools
import hashlib
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import decode_ref as dr  # noqa: E402
import inflate_ref as ir  # noqa: E402
from plakar_amd import _lib, decode  # noqa: E402
from plakar_amd._lib import CDC_E_AUTH, CDC_E_CORRUPT, CDC_E_MISMATCH, CDC_E_NOSPACE, CDC_E_UNSUPPORTED  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))
SENTINEL = 0xA5
SLACK = 4096


def _decode(blobs, key=None, cap=0, compressed="GZIP"):
    """One cdc_decode_device call into the middle of a sentinel-filled buffer:
    (status, out_offsets, the whole buffer on the host)."""
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8).copy()).cuda()
    buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo, st = decode.decode_device(base, offs[:-1], lens, buf[SLACK:SLACK + cap], key=key, compressed=compressed)
    return st, oo, buf.cpu().numpy()


def _whole_buffer(host, want, scratch=0):
    """The margins, the outputs back to back, and nothing after them but the
    `scratch` bytes that late failures may leave overwritten."""
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    body = b"".join(w for w in want if w is not None)
    got = host[SLACK:SLACK + len(body)].tobytes()
    assert got == body, "the outputs differ" if len(got) == len(body) else "short buffer"
    assert (host[SLACK + len(body) + scratch:] == SENTINEL).all(), "bytes past the outputs were written"


def _expect(blobs, want, status, key=None, scratch=0, slack_cap=0):
    """Decode and hold everything against want (None: failed) and status."""
    total = sum(len(w) for w in want if w is not None)
    st, oo, host = _decode(blobs, key, total + scratch + slack_cap)
    bad = [i for i in range(len(blobs)) if st[i] != status[i]]
    assert not bad, [(i, int(st[i]), status[i]) for i in bad[:10]]
    sizes = [0 if w is None else len(w) for w in want]
    assert list(oo) == list(np.concatenate([[0], np.cumsum(sizes)])), "out_offsets"
    _whole_buffer(host, want, scratch)


@functools.lru_cache(None)
def _big():
    t = ir.text(1 << 20, 77)
    mix = ir.rnd(300_000, 78) + ir.text(400_000, 79) + bytes(200_000) + ir.rnd(48_576, 80) + ir.text(100_000, 81)
    assert len(mix) == 1 << 20
    z = bytes(4 << 20)
    zz = ir.member(ir.raw_deflate(z, level=9), z)
    assert len(z) / len(zz) > 1000
    return [(ir.gz(t), t), (zz, z), (ir.gz(mix), mix)]


@pytest.mark.parametrize("sealed", [False, True], ids=["plain", "sealed"])
def test_written_by_zlib(sealed):
    zs = ir.zlib_streams()
    # the runs of lengths 0..300 one after the other: their starts are triangular numbers, every residue mod 16
    order = sorted(zs, key=lambda k: (k.startswith("text-") and k[5:].isdigit(), k.startswith("zeros-")))
    pairs = [zs[k] for k in order] + _big()
    blobs = [p[0] for p in pairs]
    want = [p[1] for p in pairs]
    status = [0] * len(pairs)
    if sealed:
        assert max(len(b) for b in blobs) > 65536, "a stream that spans records"
        blobs = [dr.seal_stream(KEY, b, 500 + i) for i, b in enumerate(blobs)]
        blobs.append(dr.flip(blobs[7], len(blobs[7]) - 1))  # a record's tag
        want.append(None)
        status.append(CDC_E_AUTH)
    starts = np.cumsum([0] + [len(w) for w in want if w is not None])
    assert {int(s) % 16 for s in starts} == set(range(16)), "outputs start at every residue"
    _expect(blobs, want, status, key=KEY if sealed else None)


def test_handmade_fixtures():
    pairs = list(ir.handmade().values())
    for s, c in pairs:
        assert ir.status_of(s) == (0, c)
    _expect([p[0] for p in pairs], [p[1] for p in pairs], [0] * len(pairs))


def test_named_corruptions_are_reported_and_contained():
    cases = ir.corruptions()
    names = sorted(cases)
    assert {s for _, s in cases.values()} == {CDC_E_CORRUPT, CDC_E_UNSUPPORTED}
    blobs, want, status, scratch = [], [], [], 0
    for i, n in enumerate(names):
        good = ir.text(1001 + 2 * i, 300 + i)      # odd-length neighbours
        blobs += [ir.gz(good), cases[n][0]]
        want += [good, None]
        status += [0, cases[n][1]]
        st, c = ir.claim(cases[n][0])
        scratch += c if st == 0 else 0              # refused only while emitting: its planned range is scratch
    blobs.append(ir.gz(b"the last neighbour"))
    want.append(b"the last neighbour")
    status.append(0)
    assert ir.claim(cases["isize-1GiB-in-30-bytes"][0])[0] == CDC_E_CORRUPT
    assert scratch < 50_000, "no corruption makes the call ask for more than its own few bytes"
    # the capacity is what the good blobs and those few claims need: a sizing pass
    # that believed the 1-GiB ISIZE would answer CDC_E_NOSPACE here
    _expect(blobs, want, status, scratch=scratch)


def test_corruptions_sealed():
    cases = ir.corruptions()
    names = sorted(cases)
    good = ir.text(777, 1)
    blobs = [dr.seal_stream(KEY, ir.gz(good), 600)] + [dr.seal_stream(KEY, cases[n][0], 601 + i)
                                                        for i, n in enumerate(names)]
    scratch = sum(c for st, c in (ir.claim(cases[n][0]) for n in names) if st == 0)
    _expect(blobs, [good] + [None] * len(names), [0] + [cases[n][1] for n in names], key=KEY, scratch=scratch)


def test_mutations_equal_inflate_ref():
    blobs = list(ir.mutations())
    ref = ir.mutation_refs()
    scratch = sum(c for (st, c), r in zip((ir.claim(b) for b in blobs), ref) if st == 0 and r[0] != 0)
    assert sum(1 for r in ref if r[0]) > 50 and sum(1 for r in ref if not r[0]) > 50
    _expect(blobs, [r[1] for r in ref], [r[0] for r in ref], scratch=scratch)


def test_crc32_slice_boundaries():
    contents = ir.crc_boundary_contents()
    blobs = [ir.stored_member(c) for c in contents]
    for b, c in zip(blobs[::37], contents[::37]):
        assert zlib.decompress(b, 31) == c
    _expect(blobs, contents, [0] * len(blobs))
    # and a wrong CRC-32 at each of the larger sizes is seen
    bad = [dr.flip(b, len(b) - 6, 5) for b in blobs[300:]]
    _expect(bad, [None] * len(bad), [CDC_E_CORRUPT] * len(bad), scratch=sum(len(c) for c in contents[300:]))


def test_nospace_reports_the_size_and_writes_nothing():
    pairs = [ir.handmade()[n] for n in ("distance-32768", "15-bit-code", "three-blocks-beyond-32k")]
    pairs.append(ir.zlib_streams()["mix-level6"])
    blobs, want = [p[0] for p in pairs], [p[1] for p in pairs]
    total = sum(len(w) for w in want)
    with pytest.raises(_lib.CdcError) as e:
        _decode(blobs, None, total - 1)
    assert e.value.status == CDC_E_NOSPACE and e.value.needed == total
    # the same call by hand, to look at the buffer afterwards
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    buf = torch.full((total + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.CdcError):
        decode.decode_device(base, offs[:-1], lens, buf[:total - 1], compressed="GZIP")
    assert (buf.cpu().numpy() == SENTINEL).all(), "nothing is written when the capacity is short"
    _expect(blobs, want, [0] * len(blobs))   # the retry with `needed`
    # decode_blobs starts from 4x and retries: the 1024 : 1 stream comes out
    zz, z = _big()[1]
    assert decode.decode_blobs([zz, blobs[1]], compressed="GZIP") == [z, want[1]]


def test_late_failure_moves_the_later_blobs_down():
    (big, text), _, _ = _big()
    first = ir.text(50_001, 90)
    bad = ir.member(ir.raw_deflate(first), first, crc=zlib.crc32(first) ^ 0x10)
    blobs = [bad] + [big] * 8 + [ir.gz(b"tail")]
    want = [None] + [text] * 8 + [b"tail"]
    _expect(blobs, want, [CDC_E_CORRUPT] + [0] * 9, scratch=len(first))


def test_check_blobs():
    hm = ir.handmade()
    names = ["all-lengths-all-distances", "15-bit-code", "member-all-fields", "single-distance-code"]
    blobs = [dr.seal_stream(KEY, hm[n][0], 700 + i) for i, n in enumerate(names)]
    blobs.append(dr.seal_stream(KEY, b"", 710))    # the empty stream is the empty blob
    sums = [hashlib.sha256(hm[n][1]).digest() for n in names] + [hashlib.sha256(b"").digest()]
    assert (decode.check_blobs(blobs, sums, key=KEY, compressed="GZIP") == 0).all()
    bad_sums = list(sums)
    bad_sums[1] = dr.flip(sums[1], 0)
    d = decode.DeviceDecoder(key=KEY, compression="GZIP")
    assert list(d.check_many(blobs, bad_sums)) == [0, CDC_E_MISMATCH, 0, 0, 0]
    plain = [hm[n][0] for n in names]
    plain[2] = ir.corruptions()["symbol-286"][0]
    assert list(decode.check_blobs(plain, sums[:4], compressed="GZIP")) == [0, 0, CDC_E_CORRUPT, 0]
    assert d(blobs[0]) == hm[names[0]][1]
    assert decode.DeviceDecoder(compression="GZIP").decode_many(plain[:2]) == [hm[n][1] for n in names[:2]]


def test_the_selector_selects():
    content = ir.text(5000, 3)
    gzs = ir.gz(content)
    frame, lz4_content = dr.fixture_frames()["mixed"]
    st, oo, host = _decode([gzs, frame], None, len(lz4_content) + 100, compressed=True)
    assert list(st) == [CDC_E_CORRUPT, 0] and host[SLACK:SLACK + oo[-1]].tobytes() == lz4_content
    st, oo, host = _decode([gzs, frame], None, len(content) + 100, compressed="GZIP")
    assert list(st) == [0, CDC_E_CORRUPT] and host[SLACK:SLACK + oo[-1]].tobytes() == content
    # every other non-zero value still means LZ4 at the C boundary
    L = _lib.lib()
    import ctypes
    blob = torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).cuda()
    out = torch.empty(len(lz4_content), dtype=torch.uint8, device="cuda")
    offs, lens = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(len(frame))
    oo2, st2 = (ctypes.c_uint64 * 2)(), (ctypes.c_int32 * 1)()
    rc = L.cdc_decode_device(0, ctypes.c_void_p(blob.data_ptr()), offs, lens, 1, 7, None,
                             ctypes.c_void_p(out.data_ptr()), out.numel(), oo2, st2,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert (rc, st2[0], oo2[1]) == (0, 0, len(lz4_content)) and out.cpu().numpy().tobytes() == lz4_content
