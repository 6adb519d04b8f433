"""Compression level 9 (CDC_LEVEL_BEST: k_lz_seq_deep, four candidates per hash
bucket and a one-position lazy look) on the device, GZIP and LZ4 alike: every
reader reads it, the ways are used (a repeat behind one to three decoys that
share its first six bytes comes out whole), the lazy look moves a match by one
byte when the later one is longer, the sizes on text and on the source tree
against zlib yardsticks computed here, the layers that pass the level on, and
levels 0 and 1 writing the bytes they wrote before (tests/golden)."""
import functools
import hashlib
import io
import json
import os
import struct
import tarfile
import zipfile
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import inflate_ref as ir  # noqa: E402
import lz4_ref  # noqa: E402
import planted  # noqa: E402
from plakar_amd import _lib, archive, decode, encode, restore, snapshot, sync  # noqa: E402
from plakar_amd.archive import ArchiveEntry  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402
from test_encode_wide import (BLOCK, IDS, KEY, ROOT, SEG, SELECTORS, SPAN, WALK_MAX, WINDOW, _encode_level_ctypes,  # noqa: E402
                              _inflate_any, _kinds, _local_header, _period7, _text_sets, _text_sizes, _today_batch,
                              _tokens)

pytestmark = pytest.mark.gpu

TOKENS_MAX = 300_000   # the Python walkers list a blob's tokens up to this size


def _enc9(blobs, sel, key=None):
    return encode.encode_blobs(blobs, key=key, compress=sel, level=9)


def _read(sel, e, c, what):
    """The independent readers of one unsealed blob: zlib or the system's liblz4, and the strict walkers."""
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


def _in_window(toks, what):
    """Every token's source lies in the 32 KiB before it and in its 4-MiB block."""
    for p, ln, d in toks:
        assert 1 <= d <= min(WINDOW, p % BLOCK), f"{what}: token ({p}, {ln}, {d})"


# ---- 1. every reader reads level 9 -----------------------------------------------------------------
@functools.lru_cache(None)
def _contents():
    out = []
    for i, n in enumerate((SEG - 13, SEG, SEG + 13, SPAN - 1, SPAN, SPAN + 1, 65535, 65536, 65537, 70001)):
        out += _kinds(n, 900 + i)
    out.append(_text_sets()["text"])
    # all 64 lanes of a step meet one bucket
    out += [bytes(70001), (b"ab" * 35001)[:70001], (b"abc" * 23334)[:70001], _period7(70001)]
    # the history starts again at the 4-MiB block
    out += [ir.text(BLOCK + d, 950 + d) for d in (1, 5, 12, 13)]
    return out


@functools.lru_cache(None)
def _encoded(sel, sealed):
    return _enc9(_contents(), sel, KEY if sealed else None)


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_independent_readers_read_level_9(sel):
    contents = _contents()
    for i, (e, c) in enumerate(zip(_encoded(sel, False), contents)):
        _read(sel, e, c, f"blob {i}")
        if len(c) <= TOKENS_MAX and (sel != "GZIP" or len(c) <= WALK_MAX):
            out, toks = _tokens(sel, e)
            assert out == c
            _in_window(toks, f"blob {i}")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_the_device_reads_level_9_plain_and_sealed(sel):
    contents = _contents()
    assert decode.decode_blobs(_encoded(sel, False), compressed=sel) == contents
    sealed = _encoded(sel, True)
    for i, (e, c) in enumerate(zip(sealed, contents)):
        assert len(e) <= encode.encode_bound(len(c), sel, True), f"blob {i}: bound"
        if len(c) <= WALK_MAX:   # the host's AES-GCM is slow: the large blobs go through the device below
            _read(sel, crypto_ref.decrypt_stream(KEY, e)[0], c, f"blob {i}")
    assert decode.decode_blobs(sealed, key=KEY, compressed=sel) == contents


@pytest.mark.parametrize("seed", planted.BATCH_SEEDS)
def test_seeded_batches_at_level_9(seed):
    """planted.seeded_batch: 1-120 blobs and one past 4 MiB, LZ4 for even
    seeds and GZIP for odd ones, sealed unless seed % 3 == 2."""
    sel = SELECTORS[seed % 2]
    key = KEY if seed % 3 != 2 else None
    contents = [c for c, _ in planted.seeded_batch(seed)]
    encs = _enc9(contents, sel, key)
    for i, (e, c) in enumerate(zip(encs, contents)):
        what = f"seed {seed} blob {i}"
        assert len(e) <= encode.encode_bound(len(c), sel, key is not None), f"{what}: bound"
        if key is not None:
            if len(c) <= WALK_MAX:       # the host's AES-GCM is slow
                _read(sel, crypto_ref.decrypt_stream(KEY, e)[0], c, what)
            continue
        _read(sel, e, c, what)
        if c and len(c) <= TOKENS_MAX and (sel != "GZIP" or len(c) <= WALK_MAX):
            out, toks = _tokens(sel, e)
            assert out == c
            _in_window(toks, what)
    assert decode.decode_blobs(encs, key=key, compressed=sel) == contents


# ---- 2. the ways --------------------------------------------------------------------------------------
# One blob under 40 KiB.  Its fifth segment starts at S0 = 32,768 behind a full
# history, so every history position is in the table; inside the segment a
# position is in the table when a step probed it, which holds for the 64 bytes
# behind a match (stride 1) and for a segment's first 64.  Q0, Q1, ... are
# 64-byte random runs at the history's end, and a copy of one of them in front
# of a planted run makes the search arrive at that run's first byte at stride 1.
S0 = 4 * SEG
RUN = 200
BUCKET_BITS = 12
QGAP = 80


def _bucket(b, p):
    """The bucket of the four bytes at p: k_lz_seq_deep's hash (layouts are
    chosen so that no unrelated position shares a planted run's bucket and
    pushes a way out; any hash spreads them, this one says where)."""
    return ((struct.unpack_from("<I", b, p)[0] * 2654435761) & 0xFFFFFFFF) >> (32 - BUCKET_BITS)


def _alone_in_its_bucket(blob, at, upto, known=()):
    """No position of [at - 64, upto) but `at` and `known` falls into at's bucket."""
    h = _bucket(blob, at)
    return not [p for p in range(max(at - 64, 0), upto) if p != at and p not in known and _bucket(blob, p) == h]


def _ways_blob(k, a_in_history, seed):
    """(blob, A, B, decoy positions, clean): R at A, k decoys (R's first 6
    bytes, then other bytes), R again at B right behind a copy of a Q; clean:
    every copy ends where it was planted."""
    R = ir.rnd(RUN, seed)
    nq = k + 2
    qs = [ir.rnd(64, seed + 1 + i) for i in range(nq)]
    decoys = [R[:6] + ir.rnd(34, seed + 100 + i) for i in range(k)]
    planted_hist = (RUN + 40 * k) if a_in_history else 0
    body = bytearray(ir.rnd(S0, seed + 50))
    qpos = [S0 - planted_hist - QGAP * (i + 1) for i in range(nq)]
    for q, at in zip(qs, qpos):
        body[at:at + 64] = q
    dpos, copies = [], []   # copies: (position, source, length) of each Q copy
    seg = bytearray()
    if a_in_history:
        A = at = S0 - planted_hist
        body[at:at + RUN] = R
        at += RUN
        for d in decoys:
            dpos.append(at)
            body[at:at + 40] = d
            at += 40
        assert at == S0
        copies.append((S0, qpos[0], 64))
        seg += qs[0]
    else:
        copies.append((S0, qpos[0], 64))
        seg += qs[0]
        A = S0 + len(seg)
        seg += R
        for i, d in enumerate(decoys):
            copies.append((S0 + len(seg), qpos[1 + i], 64))
            seg += qs[1 + i]
            dpos.append(S0 + len(seg))
            seg += d
        copies.append((S0 + len(seg), qpos[k + 1], 64))
        seg += qs[k + 1]
    B = S0 + len(seg)
    seg += R + ir.rnd(300, seed + 60)
    blob = bytes(body) + bytes(seg)
    clean = (_alone_in_its_bucket(blob, A, B, dpos) and blob[A + RUN] != blob[B + RUN] and blob[A - 1] != blob[B - 1]
             and all(blob[p + 6] != R[6] and blob[p - 1] != blob[B - 1] for p in dpos)
             and all(blob[c + n] != blob[src + n] and _alone_in_its_bucket(blob, src, c) for c, src, n in copies))
    return blob, A, B, dpos, clean


def _ways_case(k, a_in_history):
    for seed in range(2000, 2700, 7):
        blob, A, B, _, clean = _ways_blob(k, a_in_history, seed)
        assert len(blob) < 40 * 1024 and blob[A:A + RUN] == blob[B:B + RUN] and S0 <= B and (A < S0) == a_in_history
        if clean:
            return blob, A, B
    raise AssertionError("no seed")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
@pytest.mark.parametrize("where", ["history", "segment"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_repeat_behind_decoys_is_taken_whole(k, where, sel):
    """k decoys stand between R and its repeat in R's bucket.  With one
    candidate per bucket the latest decoy is what a probe of the repeat meets:
    6 bytes.  With four ways R itself is still there, and the longest is taken."""
    blob, A, B = _ways_case(k, where == "history")
    e1 = encode.encode_blobs([blob], compress=sel, level=1)[0]
    (e9,) = _enc9([blob], sel)
    _read(sel, e9, blob, "blob")
    assert decode.decode_blobs([e9], compressed=sel) == [blob]
    out, toks = _tokens(sel, e9)
    assert out == blob
    _in_window(toks, "blob")
    _, toks1 = _tokens(sel, e1)
    print(f"k {k}, A in the {where}: level 1 covers the repeat with {[t for t in toks1 if B <= t[0] < B + RUN]}, "
          f"level 9 with {[t for t in toks if B <= t[0] < B + RUN]}; {len(e1)} -> {len(e9)} bytes")
    assert (B, RUN, B - A) in toks


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
@pytest.mark.parametrize("where", ["history", "segment"])
@pytest.mark.parametrize("k", [4, 9])
def test_more_decoys_than_ways_round_trip(k, where, sel):
    blob, A, B, _, _ = _ways_blob(k, where == "history", 2500 + k)
    (e9,) = _enc9([blob], sel)
    _read(sel, e9, blob, "blob")
    assert decode.decode_blobs([e9], compressed=sel) == [blob]
    out, toks = _tokens(sel, e9)
    assert out == blob
    _in_window(toks, "blob")


def _out_of_reach():
    """R at 24 and again 33,000 later: out of reach by 232 bytes, though inside
    the repeat's window in LDS.  A twin of R's first 40 bytes, 2,000 before
    the segment, is in reach.  Everything else is zero, so nothing shares R's
    bucket (both ways are still in it when the repeat is probed) and the run
    of zeros in front of the repeat is the copy that leaves the stride at 1."""
    for seed in range(2600, 2900, 7):
        R = ir.rnd(RUN, seed)
        A, T, B = 24, S0 - 2000, S0 + 256
        blob = bytearray(B + RUN + 300)
        blob[A:A + RUN] = R
        blob[T:T + 40] = R[:40]
        blob[B:B + RUN] = R
        blob[B + RUN:] = ir.rnd(300, seed + 4)
        blob = bytes(blob)
        grams = {blob[p:p + 4] for p in range(B) if p not in (A, T)}
        if 0 not in R[:41] and R[:4] not in grams and _alone_in_its_bucket(blob, A, B, (T,)) and blob[B + RUN] != 0:
            return blob, A, T, B
    raise AssertionError("no seed")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_a_way_out_of_reach_is_refused_and_the_twin_used(sel):
    blob, A, T, B = _out_of_reach()
    assert B - A == 33_000 and len(blob) < 40 * 1024
    (e9,) = _enc9([blob], sel)
    _read(sel, e9, blob, "blob")
    assert decode.decode_blobs([e9], compressed=sel) == [blob]
    out, toks = _tokens(sel, e9)
    assert out == blob
    _in_window(toks, "blob")
    assert all(d <= min(WINDOW, p) for p, _, d in toks)
    assert (B, 40, B - T) in toks, [t for t in toks if t[0] >= B - 64]


# ---- 3. the lazy look ------------------------------------------------------------------------------------
S1, S2 = SEG - 900, SEG - 600   # the two sources, at the first segment's end


def _lazy_blob(seed, at, tail_len):
    """Source 1 `wxyz` + noise and source 2 `xyz` + L in the first segment
    (random bytes); the target `wxyz` + L at `at` behind a run of zeros from
    the segment's start (the copy that leaves the stride at 1); then tail_len
    random bytes."""
    L = ir.rnd(RUN, seed)
    w, x, y, z = ir.rnd(4, seed + 1)
    body = bytearray(ir.rnd(SEG, seed + 3))
    body[S1:S1 + 4] = bytes([w, x, y, z])
    body[S2:S2 + 3] = bytes([x, y, z])
    body[S2 + 3:S2 + 3 + RUN] = L
    tail = ir.rnd(tail_len, seed + 4)
    blob = bytes(body) + bytes(at - SEG) + bytes([w, x, y, z]) + L + tail
    ok = (0 not in (w, x, y, z) and len({w, x, y, z}) == 4 and blob[S1 + 4] != L[0] and blob[S2 - 1] != w
          and blob[S2 + 3 + RUN] != (tail + b"\0")[0] and blob[S1 - 1] != 0
          and _alone_in_its_bucket(blob, S1, at) and _alone_in_its_bucket(blob, S2, at, (at + 1,)))
    return blob, ok


def _lazy_case(at, tail_len):
    for seed in range(3000, 3700, 7):
        blob, ok = _lazy_blob(seed, at, tail_len)
        if ok:
            return blob
    raise AssertionError("no seed")


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_the_lazy_look_takes_the_longer_match(sel):
    """At the target's `w` the only match is source 1's four bytes; one byte on,
    source 2 gives 203.  The look leaves `w` a literal."""
    at = SEG + 3000
    blob = _lazy_case(at, 300)
    e1 = encode.encode_blobs([blob], compress=sel, level=1)[0]
    (e9,) = _enc9([blob], sel)
    _read(sel, e9, blob, "blob")
    assert decode.decode_blobs([e9], compressed=sel) == [blob]
    out, toks = _tokens(sel, e9)
    assert out == blob
    _in_window(toks, "blob")
    _, toks1 = _tokens(sel, e1)
    print(f"level 1: {[t for t in toks1 if at <= t[0] < at + 4 + RUN]}, level 9: {[t for t in toks if at <= t[0] < at + 4 + RUN]}")
    assert (at + 1, RUN + 3, at + 1 - S2) in toks
    assert not any(p <= at < p + ln for p, ln, _ in toks), "w is a literal"


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_no_look_from_a_segments_last_searchable_position(sel):
    """`w` stands on the second segment's last position that starts a match
    (its end - 4): q + 1 is not searched, so no look happens, and source 1's
    four bytes are the token."""
    at = 2 * SEG - 4
    blob = _lazy_case(at, 300)
    (e9,) = _enc9([blob], sel)
    _read(sel, e9, blob, "blob")
    assert decode.decode_blobs([e9], compressed=sel) == [blob]
    out, toks = _tokens(sel, e9)
    assert out == blob
    _in_window(toks, "blob")
    assert all(p // SEG == (p + ln - 1) // SEG for p, ln, _ in toks), "a token stays in its segment"
    assert (at, 4, at - S1) in toks


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_a_lazily_moved_match_at_the_end_of_a_blob(sel):
    """Blobs that end 0-16 bytes after the target: LZ4's last five bytes are
    literals and no match starts in the last twelve, also when the look has
    moved the match; liblz4 and the strict walker decode each."""
    at = SEG + 3000
    blobs = [_lazy_case(at, d) for d in range(17)]
    encs = _enc9(blobs, sel)
    for d, (e, c) in enumerate(zip(encs, blobs)):
        _read(sel, e, c, f"{d} bytes after the target")
        out, toks = _tokens(sel, e)
        assert out == c
        _in_window(toks, f"{d} bytes after the target")
        moved = [t for t in toks if t[0] == at + 1 and t[2] == at + 1 - S2]
        assert moved and (sel == "GZIP" or moved[0][1] == min(RUN + 3, RUN + 3 + d - 5)), f"{d}: {toks[-3:]}"
    assert decode.decode_blobs(encs, compressed=sel) == blobs


# ---- 4. sizes, against zlib alone --------------------------------------------------------------------------
def _zlib_segments(data, level):
    """zlib at `level`, raw deflate, each 8-KiB segment with the 32 KiB before
    it as preset dictionary: the shape the device compresses in."""
    total = 0
    for a in range(0, len(data), SEG):
        d = data[max(0, a - WINDOW):a]
        z = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=d) if d else zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(z.compress(data[a:a + SEG]) + z.flush())
    return total


@functools.lru_cache(None)
def _best_sizes(name, sel):
    data = _text_sets()[name]
    (e9,) = _enc9([data], sel)
    assert _inflate_any(sel, e9) == data
    return len(e9)


@pytest.mark.parametrize("name", ["text", "tree"])
def test_size_at_level_9(name):
    """The GZIP member at level 9 is at most the midpoint of zlib 1 and zlib 4
    (its first lazy level, chain 16), both per segment with dictionary, and
    strictly below level 1's; LZ4 at level 9 is strictly below level 1's.
    Measured on an MI355X (DESIGN.md 5.18 has the table)."""
    data = _text_sets()[name]
    z1, z4 = _zlib_segments(data, 1), _zlib_segments(data, 4)
    z6 = len(zlib.compress(data, 6))
    g0, g1 = _text_sizes(name, "GZIP")
    l0, l1 = _text_sizes(name, True)
    g9, l9 = _best_sizes(name, "GZIP"), _best_sizes(name, True)
    print(f"{name}: {len(data)} bytes; zlib segments with dictionary: level 1 {z1}, level 4 {z4}, midpoint {(z1 + z4) / 2}; "
          f"zlib 6 whole {z6}; GZIP level 0 {g0}, level 1 {g1}, level 9 {g9}; LZ4 level 0 {l0}, level 1 {l1}, level 9 {l9}")
    assert z4 < z1
    assert g9 <= (z1 + z4) / 2
    assert g9 < g1
    assert l9 < l1


# ---- 5. the layers -----------------------------------------------------------------------------------------------
LEVELS = (0, 1, 9)


def test_gzip_stream_at_level_9():
    text = _text_sets()["text"]
    pieces = [text[:400_000], text[400_000:400_001], text[400_001:]]
    sizes = {}
    for level in (1, 9):
        with archive.GzipStream(level=level) as s:
            member = b"".join(s.piece(p, last=i == 2) for i, p in enumerate(pieces))
        d = zlib.decompressobj(31)
        assert d.decompress(member) == text and d.eof and d.unused_data == b"", "one member"
        assert struct.unpack("<II", member[-8:]) == (zlib.crc32(text), len(text))
        sizes[level] = len(member)
    print(f"gzip stream of three pieces: {sizes}")
    assert sizes[9] <= sizes[1]


def test_zip_pieces_at_level_9():
    body = _text_sets()["text"][:300_000]
    names = [b"first.txt", b"second.txt"]
    hdrs = [_local_header(n) for n in names]
    src = torch.from_numpy(np.frombuffer(body + body, dtype=np.uint8).copy()).cuda()
    pieces, at = [], 0
    for i, h in enumerate(hdrs):
        pieces.append(dict(off=i * len(body), len=len(body), first=True, last=True, hdr_off=at, hdr_len=len(h)))
        at += len(h)
    cap = sum(archive.zip_piece_bound(len(body), len(h)) for h in hdrs)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    totals = {}
    for level in (1, 9):
        total, outs = archive.zip_pieces_device(src, pieces, b"".join(hdrs), out, level=level)
        data = out[:total].cpu().numpy().tobytes()
        directory = b""
        for n, o in zip(names, outs):
            directory += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 0x0314, 20, 0x8, 8, 0, 0x21, zlib.crc32(body),
                                     o["deflate_len"], len(body), len(n), 0, 0, 0, 0, 0o100644 << 16, o["out_off"]) + n
        end = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 2, 2, len(directory), len(data), 0)
        z = zipfile.ZipFile(io.BytesIO(data + directory + end))
        assert z.testzip() is None and [z.read(n.decode()) for n in names] == [body, body]
        assert outs[0]["deflate_len"] == outs[1]["deflate_len"], "an entry sees nothing of the one before it"
        totals[level] = total
    print(f"zip batch of two entries: {totals}")
    assert totals[9] <= totals[1]


@pytest.fixture(scope="module")
def text_backup(tmp_path_factory):
    """The text set backed up through BackupSession(level=9): (files, objects, packfiles, stored bytes per level)."""
    d = tmp_path_factory.mktemp("best_in")
    files = [_text_sets()["text"], b"", ir.rnd(5000, 72)]
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i}"
        p.write_bytes(b)
        paths.append(str(p))
    res = {}
    for level in (1, 9):
        repo = Repository(Configuration("FASTCDC", 16384, 65536, 262144))
        with snapshot.BackupSession(repo=repo, key=KEY, compression="GZIP", max_size=2 << 20, timestamp=5, level=level) as s:
            objs, packs, _ = s.run(paths)
        res[level] = (objs, packs)
    return files, res


def test_backup_session_at_level_9_restores(text_backup):
    files, res = text_backup
    stored = {}
    for level, (objs, packs) in res.items():
        contents, statuses, _ = restore.restore_files(objs, packs, key=KEY, compression="GZIP")
        assert list(statuses) == [0] * len(files) and [bytes(c) for c in contents] == files
        stored[level] = sum(len(p) for p in packs)
    print(f"stored bytes: {stored}")
    assert stored[9] <= stored[1]


def test_archives_at_level_9(text_backup):
    files, res = text_backup
    objs, packs = res[9]
    ents = [ArchiveEntry(f"dir/f{i}", o, mtime=1_700_000_000 + i) for i, o in enumerate(objs)]
    sizes = {}
    for level in (1, 9):
        data, statuses, _ = archive.archive_files(ents, packs, key=KEY, compression="GZIP", format="tarball", level=level)
        assert statuses == [0] * len(files)
        with tarfile.open(fileobj=io.BytesIO(data), mode="r:gz") as t:
            assert [t.extractfile(m).read() for m in t.getmembers() if m.isfile()] == files
        zdata, statuses, _ = archive.zip_files(ents, packs, key=KEY, compression="GZIP", level=level)
        assert statuses == [0] * len(files)
        z = zipfile.ZipFile(io.BytesIO(zdata))
        assert z.testzip() is None and [z.read(f"dir/f{i}") for i in range(len(files))] == files
        sizes[level] = (len(data), len(zdata))
    print(f"tar.gz and zip: {sizes}")
    assert sizes[9][0] <= sizes[1][0] and sizes[9][1] <= sizes[1][1]


def test_transcode_lz4_to_gzip_at_every_level():
    text = _text_sets()["text"]
    plains = [text[i:i + 150_000] for i in range(0, len(text), 150_000)] + [b"", ir.rnd(3000, 5)]
    stored = encode.encode_blobs(plains, compress=True)
    sums = [hashlib.sha256(p).digest() for p in plains]
    sizes = {}
    for level in LEVELS:
        outs = sync.transcode_blobs(stored, src=(None, "LZ4"), dst=(None, "GZIP"), checksums=sums, level=level)
        assert [_inflate_any("GZIP", o) for o in outs] == plains, level
        sizes[level] = sum(map(len, outs))
    print(f"transcode LZ4 -> GZIP: {sizes}")
    assert sizes[9] < sizes[1] < sizes[0]
    assert sync.transcode_blobs(stored, src=(None, "LZ4"), dst=(None, "GZIP"), checksums=sums) == \
        encode.encode_blobs(plains, compress="GZIP"), "without a level it is level 0"
    # the paths that keep the compression ignore the level
    sealed = sync.transcode_blobs(stored, src=(None, "LZ4"), dst=(KEY, "LZ4"), level=9)
    assert decode.decode_blobs(sealed, key=KEY, compressed=True) == plains


def test_backup_files_runs_at_the_level(tmp_path):
    """snapshot.backup_files goes through cdc_backup_run_level."""
    p = tmp_path / "text"
    p.write_bytes(_text_sets()["text"])
    stored = {}
    for level in (0, 1):
        repo = Repository(Configuration("FASTCDC", 16384, 65536, 262144))
        o, pk, _ = snapshot.backup_files([str(p)], repo=repo, key=None, compression="GZIP", timestamp=5, level=level)
        stored[level] = sum(len(x) for x in pk)
        c, st, _ = restore.restore_files(o, pk, key=None, compression="GZIP")
        assert list(st) == [0] and bytes(c[0]) == _text_sets()["text"]
    print(f"stored bytes: {stored}")
    assert stored[1] < stored[0]


# ---- 6. levels 0 and 1 are what they were -----------------------------------------------------------------------------
@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
@pytest.mark.parametrize("level", [0, 1])
def test_levels_0_and_1_write_the_bytes_they_wrote(level, sel):
    """tests/golden/encode_levels_sha256.json: the SHA-256 of every encoded blob
    of test_encode_wide._today_batch(), compress-only, written by the build
    before level 9 existed."""
    with open(os.path.join(ROOT, "tests", "golden", "encode_levels_sha256.json")) as f:
        want = json.load(f)[f"{'gzip' if sel == 'GZIP' else 'lz4'}_level{level}"]
    got = [hashlib.sha256(e).hexdigest() for e in _encode_level_ctypes(_today_batch(), sel, level)]
    assert len(want) == 40 and got == want
