"""The level-1 match search (k_lz_seq_wide) on contents with planted repeats
(tests/planted.py): the backward extension to the byte, the window load at
every source residue and history size, LZ4's end of block behind a history,
seeded batches, more than 1,024 blobs in a call, stream and zip pieces that
must see nothing before them, and the size on planted content against the
zlib level 1 yardstick of tests/test_encode_wide.py.  Every blob is read by
the independent readers (liblz4 and the strict walker, or zlib and the Python
inflater up to 70,000 bytes) and by the device's decoder."""
import functools
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import inflate_ref as ir  # noqa: E402
import lz4_ref  # noqa: E402
import planted  # noqa: E402
from plakar_amd import archive, decode, encode  # noqa: E402
from test_encode_wide import (BLOCK, IDS, KEY, SEG, SELECTORS, WALK_MAX, WINDOW, _gz_matches, _inflate_any,  # noqa: E402
                              _local_header, _lz4_matches, _period7, _tokens, _zlib1_segments)

pytestmark = pytest.mark.gpu


def _device_encode(buf, offs, lens, sel, level=1, key=None):
    """encode.encode_device over the bytes `buf` as one device buffer: the encoded blobs."""
    base = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).cuda()
    assert base.data_ptr() % 16 == 0
    cap = sum(encode.encode_bound(n, sel, key is not None) for n in lens)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(base, offs, lens, out, key=key, compress=sel, level=level)
    host = out[:int(oo[-1])].cpu().numpy()
    return [host[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(len(lens))]


def _read(sel, e, c, what):
    """The independent readers of one unsealed blob."""
    assert len(e) <= encode.encode_bound(len(c), sel, False), f"{what}: bound"
    assert _inflate_any(sel, e) == c, f"{what} ({len(c)} bytes)"
    if not c:
        assert e == b""
    elif sel == "GZIP":
        assert struct.unpack("<II", e[-8:]) == (zlib.crc32(c), len(c) & 0xFFFFFFFF)
        if len(c) <= WALK_MAX:
            assert ir.status_of(e) == (0, c), f"{what} ({len(c)} bytes): the walker"
    else:
        assert lz4_ref.content(lz4_ref.walk_frame(e)) == c, f"{what} ({len(c)} bytes): the strict walker"


def _in_window(toks, what, floor=0):
    """Every token's source lies in the 32 KiB before it, in its 4-MiB block and after `floor`."""
    for p, ln, d in toks:
        assert 1 <= d <= min(WINDOW, p % BLOCK, p - floor), f"{what}: token ({p}, {ln}, {d})"


def _assert_copy(sel, toks, pos, length, dist, what):
    """The copy is one LZ4 match, or DEFLATE's pieces of at most 258 that start
    at pos, touch and add up to length."""
    if sel != "GZIP":
        assert (pos, length, dist) in toks, f"{what}: {[t for t in toks if t[0] + t[1] > pos and t[0] < pos + length]}"
        return
    ts = sorted(t for t in toks if t[2] == dist)
    assert ts and ts[0][0] == pos, f"{what}: {ts[:3]}"
    assert all(a[0] + a[1] == b[0] for a, b in zip(ts, ts[1:])) and all(3 <= ln <= 258 for _, ln, _ in ts), f"{what}: {ts}"
    assert sum(ln for _, ln, _ in ts) == length, f"{what}: {ts}"


# ---- 2. the backward extension, to the byte ------------------------------------------------------
def _exact(variant):
    """The blob (or the two) of a variant and the copies expected, the seed
    chosen so that every copy stops where it was planted."""
    for s in range(900, 1000, 3):
        R = bytearray(ir.rnd(24576, s))
        L = ir.rnd(4000, s + 1)
        tail = ir.rnd(1192, s + 2)
        T = bytes(R[5000:8000])
        if variant == "one":
            blob = bytes(R) + L + T + tail
            want = [(28576, 3000, 23576)]
            ok = L[-1] != R[4999] and tail[0] != R[8000]
        elif variant == "two":
            R[11900:12000] = R[7900:8000]       # what precedes the second source is the first copy's tail
            T2 = bytes(R[12000:13000])
            blob = bytes(R) + L + T + T2 + tail[:192]
            want = [(28576, 3000, 23576), (31576, 1000, 19576)]
            ok = L[-1] != R[4999] and T2[0] != R[8000] and tail[0] != R[13000]
        else:
            first = ir.rnd(20001, s + 3)
            T = bytes(R[:3000])
            second = T + bytes(R[3000:12200]) + first[-100:] + T + tail[:1084]
            blob = (first, second)
            want = [(12300, 3000, 12300)]
            ok = tail[0] != R[3000]
        if ok:
            return blob, want
    raise AssertionError("no seed")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_backward_extension_exact(sel):
    """A copy of 3,000 bytes begins at 28,576, after 4,000 literals of the
    fourth segment (stride 63): the probe that hits lies somewhere inside it,
    and the first `for (;;)` of k_lz_seq_wide walks back, 64 bytes a turn, to
    the planted byte.  Without that loop, or with one turn only (`if (back <
    64) break` taken early), the token starts late; a loop that runs past a
    mismatch gives a blob that does not decode."""
    blob, want = _exact("one")
    assert len(blob) == 32768 and blob[28576:31576] == blob[5000:8000]
    assert blob[28575] != blob[4999] and blob[31576] != blob[8000], "the copy is 3,000 bytes, not one more either way"
    (e,) = _device_encode(blob, [0], [len(blob)], sel)
    _read(sel, e, blob, "blob")
    assert decode.decode_blobs([e], compressed=sel) == [blob]
    out, toks = _tokens(sel, e)
    assert out == blob
    _in_window(toks, "blob")
    _assert_copy(sel, toks, *want[0], "the copy")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_backward_extension_stops_at_the_match_before(sel):
    """Variant (a): a second copy follows the first at once, and the bytes
    before its source equal the first copy's last 100.  `room = min(q -
    anchor, cq)`: without `q - anchor` the second match would walk back into
    the first one's bytes."""
    blob, want = _exact("two")
    assert len(blob) == 32768 and blob[31576:32576] == blob[12000:13000] and blob[31476:31576] == blob[11900:12000]
    assert blob[28575] != blob[4999] and blob[31576] != blob[8000] and blob[32576] != blob[13000]
    (e,) = _device_encode(blob, [0], [len(blob)], sel)
    _read(sel, e, blob, "blob")
    assert decode.decode_blobs([e], compressed=sel) == [blob]
    out, toks = _tokens(sel, e)
    assert out == blob
    _in_window(toks, "blob")
    for w in want:
        _assert_copy(sel, toks, *w, f"the copy at {w[0]}")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_backward_extension_stops_at_the_blob(sel):
    """Variant (b): the copy's twin is the blob's first bytes, and the 100
    bytes before the copy equal the 100 bytes before the blob in device memory
    (the blob in front of it).  The copy begins 4,108 bytes into the second
    segment, so the probe that hits lies some hundred bytes inside it and the
    walk back ends on the twin's first byte, the window's first (hist is 8,192
    here).  `room = min(q - anchor, cq)`: without `cq` it would go on before
    the window, and the match would reach before the blob."""
    (first, second), want = _exact("blob")
    assert len(second) == 16384 and second[12300:15300] == second[:3000] and second[12200:12300] == first[-100:]
    assert second[15300] != second[3000]
    encs = _device_encode(first + second, [0, len(first)], [len(first), len(second)], sel)
    for e, c in zip(encs, (first, second)):
        _read(sel, e, c, "blob")
    assert decode.decode_blobs(encs, compressed=sel) == [first, second]
    out, toks = _tokens(sel, encs[1])
    assert out == second
    _in_window(toks, "the second blob")
    _assert_copy(sel, toks, *want[0], "the copy")


# ---- 3. the window load ------------------------------------------------------------------------------
@functools.lru_cache(None)
def _window_buffer():
    blobs = planted.window_blobs()
    buf = bytearray(blobs[0][0][:4096])       # in front of the first blob: its own first bytes, 4,096 back
    offs = []
    for i, (c, _) in enumerate(blobs):
        fill = ir.rnd(16, 640 + i)
        while len(buf) % 16 != i:
            buf += fill[len(buf) % 16:][:1]
        offs.append(len(buf))
        buf += c
    buf += ir.rnd(64, 639)
    return bytes(buf), offs, blobs


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_window_load_at_every_residue(sel):
    """Sixteen blobs of k * 8192 + r bytes at source residues 0..15 (mod 16) in
    one buffer: the window load of k_lz_seq_wide with hist 8, 16, 24 and 32
    KiB (`nbulk`), a last segment of 0, 1, 255 or 511 whole 16-byte pieces
    (the short-segment loop) and `tail` 0, 1, 15.  A piece loaded from `win`
    rounded down to 16, a tail stored at a wrong LDS byte or left out, or
    `nbulk` that drops the last bulk turn gives a window that is not the
    source: a verified match then copies other bytes than the decoder will,
    and the blob does not read back.  Every blob ends in a copy of 600 bytes,
    and a token must end 5 bytes before the blob's end (LZ4's rule, which the
    search keeps for DEFLATE too): the forward extension compared the last
    segment's bytes, the tail's among them, so they stand in their places.
    (Where the last segment has 15-17 bytes, only its first 3-5 positions are
    probed; the seeds of planted.window_blobs are such that one of them finds
    its twin still in the table.)"""
    buf, offs, blobs = _window_buffer()
    assert [o % 16 for o in offs] == list(range(16)) and offs[0] == 4096
    assert buf[:4096] == blobs[0][0][:4096], "the decoy"
    lens = [len(c) for c, _ in blobs]
    encs = _device_encode(buf, offs, lens, sel)
    for i, (e, (c, _)) in enumerate(zip(encs, blobs)):
        _read(sel, e, c, f"blob {i}")
        out, toks = _tokens(sel, e)
        assert out == c
        _in_window(toks, f"blob {i}")
        if len(c) > 2 * SEG:
            assert any(d > SEG for _, _, d in toks), f"blob {i} ({len(c)} bytes): no match from past 8,192"
        assert any(p + ln == len(c) - 5 for p, ln, _ in toks), f"blob {i} ({len(c)} bytes): {toks[-1:]}"
    assert decode.decode_blobs(encs, compressed=sel) == [c for c, _ in blobs]


# ---- 4. the end of a block behind a history ----------------------------------------------------------
@functools.lru_cache(None)
def _end_contents():
    out = []
    for k in (1, 4, 5):
        for d in range(17):
            out += [_period7(k * SEG + d), ir.text(k * SEG + d, 40 + d)]
    for d in (5, 13):
        out.append(_period7(BLOCK + d))
    for d in (1, 12):
        out.append(ir.text(BLOCK + d, 60 + d))
    return out


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_end_of_block_with_a_history(sel):
    """Repetitive blobs that end 0..16 bytes past a segment edge, the last
    segment behind 8 or 32 KiB of history, and 1, 5, 12, 13 bytes past a 4-MiB
    block.  `start_lim` / `end_lim` of k_lz_seq_wide are window positions:
    without `hist +` no match is found in such a segment at all, and with
    `S.len` in the place of `S.rem` a match begins in the block's last 12
    bytes or covers its last 5, which the strict walker refuses.  `S.hist =
    seg_hist(level, g * kSegLZ)` counts g from the block: counted from the
    blob, the 13 bytes of period-7's second block would copy from the first,
    which the walker refuses for LZ4 and the token rule below for GZIP."""
    contents = _end_contents()
    encs = encode.encode_blobs(contents, compress=sel, level=1)
    for i, (e, c) in enumerate(zip(encs, contents)):
        _read(sel, e, c, f"blob {i}")
        if sel == "GZIP" and (len(c) > WALK_MAX and c[:7] != b"abcdefg"):
            continue                         # 4 MiB of text is too long for the Python inflater: zlib read it
        out, toks = _tokens(sel, e)
        assert out == c
        _in_window(toks, f"blob {i}")
        if len(c) % SEG > 12 and len(c) < BLOCK and c[:7] == b"abcdefg":
            assert toks[-1][0] + toks[-1][1] > len(c) - len(c) % SEG, f"blob {i}: the last segment has a match"
    assert decode.decode_blobs(encs, compressed=sel) == contents


# ---- 5. seeded batches --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", planted.BATCH_SEEDS)
def test_seeded_batches_at_level_1(seed):
    """planted.seeded_batch: 1-120 blobs and one past 4 MiB, LZ4 for even
    seeds and GZIP for odd ones, sealed unless seed % 3 == 2."""
    sel = SELECTORS[seed % 2]
    key = KEY if seed % 3 != 2 else None
    contents = [c for c, _ in planted.seeded_batch(seed)]
    encs = encode.encode_blobs(contents, key=key, compress=sel, level=1)
    for i, (e, c) in enumerate(zip(encs, contents)):
        what = f"seed {seed} blob {i}"
        assert len(e) <= encode.encode_bound(len(c), sel, key is not None), f"{what}: bound"
        if key is not None:
            if len(c) <= WALK_MAX:       # the host's AES-GCM is slow
                _read(sel, crypto_ref.decrypt_stream(KEY, e)[0], c, what)
            continue
        _read(sel, e, c, what)
        if c:
            out, toks = _tokens(sel, e)
            assert out == c
            _in_window(toks, what)
    assert decode.decode_blobs(encs, key=key, compressed=sel) == contents


# ---- 6. past one tile -------------------------------------------------------------------------------
@pytest.mark.parametrize("sel,sealed", [("GZIP", True), (True, False)], ids=["gzip-sealed", "lz4"])
def test_1500_blobs_at_level_1(sel, sealed):
    contents = [c for c, _ in planted.tile_blobs()]
    key = KEY if sealed else None
    e0 = encode.encode_blobs(contents, key=key, compress=sel, level=0)
    e1 = encode.encode_blobs(contents, key=key, compress=sel, level=1)
    assert decode.decode_blobs(e1, key=key, compressed=sel) == contents
    for i in range(0, len(contents), 50):
        _read(sel, crypto_ref.decrypt_stream(KEY, e1[i])[0] if sealed else e1[i], contents[i], f"blob {i}")
    t0, t1 = sum(map(len, e0)), sum(map(len, e1))
    print(f"{len(contents)} blobs, {sum(map(len, contents))} bytes: level 0 {t0}, level 1 {t1}")
    assert t1 < t0


# ---- 7. a piece sees nothing before it ----------------------------------------------------------------
def _stream(src, pieces):
    """One level-1 gzip member from (offset, length) pieces of the device tensor src."""
    with archive.GzipStream(level=1) as s:
        member = b""
        for i, (off, n) in enumerate(pieces):
            out = torch.empty(archive.gzip_stream_bound(n), dtype=torch.uint8, device="cuda")
            got = s.piece_device(src[off:], n, out, last=i == len(pieces) - 1)
            member += out[:got].cpu().numpy().tobytes()
    return member


def _one_member(member, content):
    d = zlib.decompressobj(31)
    assert d.decompress(member) == content and d.eof and d.unused_data == b"", "one member"
    assert struct.unpack("<II", member[-8:]) == (zlib.crc32(content), len(content))


def test_a_stream_piece_sees_nothing_before_it():
    """Device memory holds A + B + A and the stream is B, then the second A:
    what lies 40,000 bytes of memory before the second piece is not what lies
    before it in the stream.  cdc_gzip_stream_piece plans `G.src` from the
    piece and `G.hist = seg_hist(level, g * kSegLZ)` from the piece's first
    segment: a hist above 0 there (or one counted from the stream) lets the
    second piece's first segments copy A's bytes out of memory, and the member
    either inflates to something else or becomes smaller than 0.99 of its
    random content.  There the twin lies 40,000 bytes back, which the
    search's own compare refuses whatever the plan says; so the same stream is
    written again from memory A + A + B, where the second piece's own bytes
    lie 20,000 before it.

    The other way round a repeat inside one piece is found: memory B + A + A,
    pieces B and then A + A.  (With pieces A and B + A of A + B + A the twin
    would lie 40,000 bytes back and in another piece: no DEFLATE writer
    reaches it.  The sizes, the two pieces and the 0.80 are kept.)"""
    A, B = ir.rnd(20000, 81), ir.rnd(20000, 82)
    for memory, pieces in ((A + B + A, [(20000, 20000), (40000, 20000)]), (A + A + B, [(40000, 20000), (20000, 20000)])):
        src = torch.from_numpy(np.frombuffer(memory, dtype=np.uint8).copy()).cuda()
        member = _stream(src, pieces)
        _one_member(member, B + A)
        assert ir.status_of(member) == (0, B + A)
        print(f"B, A: {len(member)} of 40000")
        assert len(member) > 0.99 * 40000
    src = torch.from_numpy(np.frombuffer(B + A + A, dtype=np.uint8).copy()).cuda()
    member = _stream(src, [(0, 20000), (20000, 40000)])
    _one_member(member, B + A + A)
    assert ir.status_of(member) == (0, B + A + A)
    _, toks = _gz_matches(member)
    print(f"B, A + A: {len(member)} of 60000")
    assert all(p >= 40000 and d == 20000 for p, _, d in toks), "only the second A copies, from the first"
    assert len(member) < 0.80 * 60000


def _zip_entry(p1, before, p2, name=b"split.bin"):
    """One zip entry from two pieces (p1; then p2, which `before` precedes in
    device memory), each its own call: (the zip file, the two deflate_len)."""
    hdr = _local_header(name)
    src = torch.from_numpy(np.frombuffer(p1 + before + p2, dtype=np.uint8).copy()).cuda()
    out = torch.empty(archive.zip_piece_bound(max(len(p1), len(p2)), len(hdr)), dtype=torch.uint8, device="cuda")
    t1, (o1,) = archive.zip_pieces_device(src, [dict(off=0, len=len(p1), first=True, last=False, hdr_off=0, hdr_len=len(hdr))],
                                          hdr, out, level=1)
    data = out[:t1].cpu().numpy().tobytes()
    t2, (o2,) = archive.zip_pieces_device(src, [dict(off=len(p1) + len(before), len=len(p2), first=False, last=True,
                                                     crc_reg=zlib.crc32(p1) ^ 0xFFFFFFFF, csize_before=o1["deflate_len"],
                                                     usize_before=len(p1))], b"", out, level=1)
    data += out[:t2].cpu().numpy().tobytes()
    body = p1 + p2
    csize = o1["deflate_len"] + o2["deflate_len"]
    assert data[-16:] == struct.pack("<IIII", 0x08074B50, zlib.crc32(body), csize, len(body)), "the descriptor"
    directory = struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 0x0314, 20, 0x8, 8, 0, 0x21, zlib.crc32(body), csize, len(body),
                            len(name), 0, 0, 0, 0, 0o100644 << 16, 0) + name
    end = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 1, 1, len(directory), len(data), 0)
    return data + directory + end, (o1["deflate_len"], o2["deflate_len"])


def test_a_zip_piece_sees_nothing_before_it():
    """An entry in two pieces; the second is Z + Z (Z random, 12,000 bytes)
    and a copy of it lies right before it in device memory.  cdc_zip.hip
    plans `G.hist = seg_hist(level, g * kSegLZ)` with g from the piece: a
    hist above 0 on the piece's first segment would copy the first Z from the
    decoy, and the entry would shrink with the decoy there and not with random
    bytes in its place (or not inflate).  The second Z is found inside the
    piece either way."""
    p1, Z = ir.rnd(20000, 83), ir.rnd(12000, 84)
    p2 = Z + Z
    sizes = []
    for before in (p2, ir.rnd(len(p2), 85)):
        data, lens = _zip_entry(p1, before, p2)
        z = zipfile.ZipFile(io.BytesIO(data))
        assert z.testzip() is None and z.read("split.bin") == p1 + p2
        sizes.append(lens)
    print(f"deflate_len of the two pieces: {sizes[0]}")
    assert sizes[0] == sizes[1], "the decoy changes nothing"
    assert sizes[0][0] > 0.99 * len(p1) and 0.99 * len(Z) < sizes[0][1] < 0.60 * len(p2)


# ---- 8. the size on planted content --------------------------------------------------------------------
@pytest.mark.parametrize("name,n,seed,mode", planted.SIZE_CASES, ids=[c[0] for c in planted.SIZE_CASES])
def test_size_on_planted_content(name, n, seed, mode):
    """The rule of test_size_on_text on 1 MiB of planted content.  zlib level
    1 per 8-KiB segment, alone -> with the 32 KiB before it as dictionary:
    far (seed 800) 950,917 -> 332,753, g1 0.650; free (seed 803) 411,954 ->
    326,943, g1 0.206.  Measured on an MI355X: DESIGN.md 5.17 has the table."""
    data, _ = planted.planted(n, seed, mode)
    alone, with_dict = _zlib1_segments(data, False), _zlib1_segments(data, True)
    g1 = 1 - with_dict / alone
    sizes = {}
    for sel in SELECTORS:
        e0, e1 = (encode.encode_blobs([data], compress=sel, level=lv)[0] for lv in (0, 1))
        assert _inflate_any(sel, e1) == data
        sizes[sel] = (len(e0), len(e1))
    g0, g1_dev = sizes["GZIP"]
    l0, l1 = sizes[True]
    print(f"{name}: {len(data)} bytes; zlib 1 segments {alone} -> {with_dict} (g1 {g1:.4f}); "
          f"GZIP level 0 {g0}, level 1 {g1_dev} (gain {1 - g1_dev / g0:.4f}); LZ4 level 0 {l0}, level 1 {l1}")
    assert g1 > 0.03, "the yardstick itself gains from the window"
    assert 1 - g1_dev / g0 >= g1 / 2
    assert l1 < l0
