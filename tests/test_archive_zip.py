"""The zip format of the archive path on the device (cdc_archive_new_zip,
plakar_amd.archive.ZipSession) and its batched raw-DEFLATE pass
(cdc_zip_pieces_device).  Python's zipfile lists the same names, modes, times
and contents; read by hand, every local header, raw stream, data descriptor,
directory record and the end record is where and what it has to be; the
contents do not depend on the batch budget; an entry written in one piece is
Encode's GZIP member without its header and trailer; an entry with a blob in
no packfile is left out whole, and a damaged blob ends the run and leaves no
file."""
import hashlib
import io
import os
import struct
import time
import types
import zipfile
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pack_loss  # noqa: E402
from datagen import low_entropy, random_bytes, text_like  # noqa: E402
from plakar_amd import _lib, archive, encode, restore, snapshot  # noqa: E402
from plakar_amd.archive import ArchiveEntry  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))
SPAN = 32768
BLOCK = 4 << 20
SIZES = [0, 1, SPAN - 1, SPAN, SPAN + 1, 300_000, BLOCK + 1]   # the span boundary; a block whose last span is short
CONFIGS = [(None, None), (KEY, "LZ4"), (KEY, "GZIP")]
IDS = ["plain", "lz4-sealed", "gzip-sealed"]
NON_ASCII = "café/naïve.txt"
SMALL_BATCH = 64 << 10
EMPTY_STREAM = b"\x01\x00\x00\xff\xff"
END_RECORD = b"PK\x05\x06" + bytes(18)
SENTINEL, SLACK = 0x5A, 4096


def _bound(n):
    """A piece's deflate bytes: n, 5 per span (a stored block's header at worst), 6 for the longest joiner."""
    return n + 5 * (-(-n // SPAN)) + 6


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("zip_in")
    files = [b"" if n == 0 else random_bytes(n, 70 + i).tobytes() if i % 2 == 0 else low_entropy(n, 70 + i).tobytes()
             for i, n in enumerate(SIZES)]
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i}"
        p.write_bytes(b)
        paths.append(str(p))
    return paths, files


@pytest.fixture(scope="module")
def backups(corpus):
    paths, _ = corpus
    made = {}

    def get(key, compression):
        if (key, compression) not in made:
            repo = Repository(Configuration("FASTCDC", 4096, 16384, 65536))
            objs, packs, _ = snapshot.backup_files(paths, repo=repo, key=key, compression=compression, max_size=2 << 20,
                                                   timestamp=11)
            assert len(objs[5].Chunks) > 3, "the 300,000-byte file is several chunks"
            made[(key, compression)] = (objs, packs)
        return made[(key, compression)]
    return get


def _entries(objs):
    """(ArchiveEntry, content index or None for a directory) in archive order."""
    names = ["empty", "one", "dir/span-1", "/abs/span", "dir/sub/span+1", "big.bin", "block.bin"]
    out = [(ArchiveEntry("dir", directory=True, mode=0o750, mtime=1_600_000_000), None)]
    out += [(ArchiveEntry(n, objs[i], mode=0o600 + i, mtime=1_700_000_000 + 2 * i), i) for i, n in enumerate(names)]
    out.append((ArchiveEntry("again/big.bin", objs[5], mode=0o444, mtime=1_700_000_101), 5))   # twice; read-only; odd second
    out.append((ArchiveEntry(NON_ASCII, objs[2], mode=0o640, mtime=100), 2))                    # before 1980
    return out


def _date_time(mtime):
    t = time.gmtime(mtime)
    return (1980, 1, 1, 0, 0, 0) if t.tm_year < 1980 else (t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min, t.tm_sec & ~1)


def _zip(objs, packs, key, compression, **kw):
    ents = _entries(objs)
    data, statuses, st = archive.zip_files([e for e, _ in ents], packs, key=key, compression=compression, **kw)
    assert statuses == [0] * len(ents), "a directory is accepted and reported as done"
    return data, st, [(e, i) for e, i in ents if not e.directory]


def _by_hand(data):
    """The archive read with struct alone: per entry a dict of the directory
    record, the local header, the raw stream and the descriptor."""
    end = len(data) - 22
    sig, d0, d1, n0, n1, dsize, doff, clen = struct.unpack_from("<IHHHHIIH", data, end)
    assert (sig, d0, d1, clen) == (0x06054B50, 0, 0, 0) and n0 == n1
    assert doff + dsize == end, "the end record follows the directory at once (no zip64 records for a small archive)"
    out, p = [], doff
    for _ in range(n0):
        (sig, creator, reader, flags, method, t, d, crc, cs, us, nlen, xlen, clen, disk, iattr, xattr,
         off) = struct.unpack_from("<IHHHHHHIIIHHHHHII", data, p)
        assert (sig, creator, reader, method, clen, disk, iattr) == (0x02014B50, 0x0314, 20, 8, 0, 0, 0)
        name, extra = data[p + 46:p + 46 + nlen], data[p + 46 + nlen:p + 46 + nlen + xlen]
        p += 46 + nlen + xlen
        lsig, lver, lflags, lmethod, lt, ld, lcrc, lcs, lus, lnlen, lxlen = struct.unpack_from("<IHHHHHIIIHH", data, off)
        assert (lsig, lver, lmethod) == (0x04034B50, 20, 8), "the directory's offset points at a local header"
        assert (lcrc, lcs, lus) == (0, 0, 0), "CRC-32 and sizes are in the descriptor"
        assert (lflags, lt, ld, lnlen) == (flags, t, d, nlen) and data[off + 30:off + 30 + nlen] == name
        assert data[off + 30 + nlen:off + 30 + nlen + lxlen] == extra, "the same extra in both headers"
        s0 = off + 30 + nlen + lxlen
        desc = data[s0 + cs:s0 + cs + 16]
        out.append(dict(name=name, extra=extra, flags=flags, crc=crc, cs=cs, us=us, xattr=xattr, off=off, raw=data[s0:s0 + cs],
                        desc=desc, end=s0 + cs + 16))
    assert p == end
    at = 0
    for r in out:       # local entries back to back from offset 0 to the directory
        assert r["off"] == at
        at = r["end"]
    assert at == doff
    return out


def _check_zip(data, ents, files):
    z = zipfile.ZipFile(io.BytesIO(data))
    assert z.testzip() is None
    assert z.namelist() == [e.name.decode().lstrip("/") for e, _ in ents]
    hand = _by_hand(data)
    assert len(hand) == len(ents)
    for info, r, (e, i) in zip(z.infolist(), hand, ents):
        content = files[i]
        assert z.read(info) == content, info.filename
        assert info.compress_type == 8 and info.flag_bits & 0x8
        assert bool(info.flag_bits & 0x800) == (e.name.decode() == NON_ASCII)
        assert info.external_attr == ((0o100000 | e.mode) << 16) | (0 if e.mode & 0o200 else 1)
        assert info.create_system == 3 and info.date_time == _date_time(e.mtime)
        assert info.CRC == zlib.crc32(content) and info.file_size == len(content)
        # by hand
        assert r["desc"] == struct.pack("<IIII", 0x08074B50, zlib.crc32(content), r["cs"], len(content))
        assert (r["crc"], r["us"]) == (zlib.crc32(content), len(content))
        d = zlib.decompressobj(-15)
        assert d.decompress(r["raw"]) == content and d.eof and d.unused_data == b"", "one raw stream, and all of it"
        assert r["extra"] == b"UT\x05\x00\x01" + struct.pack("<I", e.mtime & 0xFFFFFFFF)
    return hand


@pytest.fixture(scope="module")
def one_batch(backups):
    made = {}

    def get(key, compression):
        if (key, compression) not in made:
            made[(key, compression)] = _zip(*backups(key, compression), key, compression)
        return made[(key, compression)]
    return get


@pytest.mark.parametrize("key,compression", CONFIGS, ids=IDS)
def test_zip_lists_the_entries_with_equal_contents(corpus, one_batch, key, compression):
    _, files = corpus
    data, st, ents = one_batch(key, compression)
    hand = _check_zip(data, ents, files)
    assert st["batches"] == 1 and st["entries"] == len(ents) == 9 and st["skipped_entries"] == 0
    assert st["output_bytes"] == len(data)
    assert st["stream_bytes"] == sum(len(files[i]) + 30 + len(r["name"]) + 9 for r, (_, i) in zip(hand, ents))
    for r, (_, i) in zip(hand, ents):
        assert r["cs"] <= _bound(len(files[i]))
    assert hand[0]["raw"] == EMPTY_STREAM and hand[0]["crc"] == 0, "an entry with no bytes: the final empty stored block"


def test_every_configuration_gives_the_same_zip(one_batch):
    assert one_batch(*CONFIGS[0])[0] == one_batch(*CONFIGS[1])[0] == one_batch(*CONFIGS[2])[0]


def test_an_entry_in_one_piece_is_encodes_member_without_header_and_trailer(corpus, one_batch):
    """Both plan the same spans, and the choice between stored, fixed and dynamic depends on the
    bit position only mod 8: the member's 80 header bits change nothing.  (Encode writes no
    member at all for an empty blob, so the empty entry is held to its five bytes above.)"""
    _, files = corpus
    data, _, ents = one_batch(None, None)
    hand = _by_hand(data)
    members = encode.encode_blobs([files[i] for _, i in ents if files[i]], compress="GZIP", key=None)
    for r, m in zip([r for r, (_, i) in zip(hand, ents) if files[i]], members):
        assert r["raw"] == m[10:-8], r["name"]


@pytest.mark.parametrize("key,compression", CONFIGS[:2], ids=IDS[:2])
def test_contents_do_not_depend_on_the_batch_budget(corpus, backups, one_batch, key, compression):
    _, files = corpus
    want, st1, _ = one_batch(key, compression)
    data, st, ents = _zip(*backups(key, compression), key, compression, batch_bytes=SMALL_BATCH)
    many, one = _check_zip(data, ents, files), _by_hand(want)
    assert st["batches"] > 60 and st["decoded_blobs"] >= st1["decoded_blobs"]
    for a, b, (_, i) in zip(one, many, ents):
        assert a["cs"] <= b["cs"], "a joiner per piece costs bytes, never saves them"
        if len(files[i]) > SMALL_BATCH:
            assert b["raw"].count(b"\x00\x00\xff\xff") >= len(files[i]) // SMALL_BATCH - 1, "many pieces, a joiner each"
        elif len(files[i]) < 4096:
            assert a["raw"] == b["raw"]


def test_the_sinks_agree(backups, tmp_path):
    objs, packs = backups(KEY, "LZ4")
    ents = [e for e, _ in _entries(objs)]
    path = str(tmp_path / "out.zip")
    pieces = []
    with archive.ZipSession(key=KEY, batch_bytes=SMALL_BATCH) as s:
        for p in packs:
            s.add_packfile(p)
        none, statuses, st = s.run(ents, path=path)
        assert none is None and statuses == [0] * len(ents)
        none, statuses, st2 = s.run(ents, on_data=pieces.append)         # the same session, a second run
        assert none is None and statuses == [0] * len(ents)
        data, statuses, st3 = s.run(ents)
    with open(path, "rb") as f:
        on_disk = f.read()
    assert len(pieces) == st2["batches"] + 1, "a write per batch and one for the directory"
    assert b"".join(pieces) == on_disk == data
    assert st["output_bytes"] == st2["output_bytes"] == st3["output_bytes"] == len(on_disk)
    assert zipfile.ZipFile(path).testzip() is None


# ---- cdc_zip_pieces_device directly -------------------------------------------------------------------
POLY = 0xEDB88320


def _crc_mul(a, b):
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def _crc_shift(nbytes):
    e, r, b = (8 * nbytes) % 0xFFFFFFFF, 0x80000000, 0x40000000
    while e:
        if e & 1:
            r = _crc_mul(r, b)
        b = _crc_mul(b, b)
        e >>= 1
    return r


def _direct_plan():
    """65 pieces in entries of one to three pieces: (content, headers, pieces)."""
    lens = [0, 1, SPAN, SPAN + 1, 5, 0, 70_001, 3 * SPAN, 17, SPAN - 1]
    shapes = [1, 2, 3, 1, 2]                 # pieces per entry, in turn
    content, pieces, headers = bytearray(), [], bytearray()
    k, e = 0, 0
    while len(pieces) < 65:
        n = min(shapes[e % len(shapes)], 65 - len(pieces))
        before = b""
        for j in range(n):
            ln = lens[k % len(lens)]
            body = bytes(text_like(ln, 200 + k) if k % 3 == 0 else random_bytes(ln, 200 + k).tobytes() if k % 3 == 1
                         else low_entropy(ln, 200 + k).tobytes())
            assert len(body) == ln
            content += b"\xEE" * (k % 3)      # gaps: pieces need not be back to back in the source
            p = dict(off=len(content), len=ln, first=j == 0, last=j == n - 1, crc_reg=zlib.crc32(before) ^ 0xFFFFFFFF,
                     csize_before=1000 * j, usize_before=len(before), entry=e, body=body)
            if j == 0:
                h = bytes((7 * e + i) & 255 for i in range(31 + e % 5))
                p.update(hdr_off=len(headers), hdr_len=len(h), hdr=h)
                headers += h
            content += body
            before += body
            pieces.append(p)
            k += 1
        e += 1
    return bytes(content), bytes(headers), pieces


@pytest.fixture(scope="module")
def direct():
    content, headers, pieces = _direct_plan()
    src = torch.from_numpy(np.frombuffer(content, dtype=np.uint8).copy()).cuda()
    cap = sum(archive.zip_piece_bound(p["len"], p.get("hdr_len", 0)) for p in pieces)
    buf = torch.full((SLACK + cap + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    total, outs = archive.zip_pieces_device(src, pieces, headers, buf[SLACK:SLACK + cap])
    host = buf.cpu().numpy()
    assert (host[:SLACK] == SENTINEL).all(), "bytes before d_out were written"
    assert (host[SLACK + total:] == SENTINEL).all(), "bytes past the total were written"
    return src, headers, pieces, total, outs, host[SLACK:SLACK + total].tobytes()


def test_pieces_lie_back_to_back_and_add_up(direct):
    _, _, pieces, total, outs, _ = direct
    assert len(pieces) == 65 and {0, 1, SPAN, SPAN + 1} <= {p["len"] for p in pieces}
    assert {(p["first"], p["last"]) for p in pieces} == {(True, True), (True, False), (False, False), (False, True)}
    at = 0
    for p, o in zip(pieces, outs):
        assert o["out_off"] == at
        desc = (24 if o["zip64"] else 16) if p["last"] else 0
        assert o["out_len"] == (p["hdr_len"] if p["first"] else 0) + o["deflate_len"] + desc
        assert o["deflate_len"] <= _bound(p["len"])
        at += o["out_len"]
    assert at == total


def test_pieces_inflate_and_their_registers_combine(direct):
    _, _, pieces, total, outs, data = direct
    raw, body, reg = b"", b"", None
    for p, o in zip(pieces, outs):
        at = o["out_off"]
        if p["first"]:
            assert data[at:at + p["hdr_len"]] == p["hdr"], "the local header from the arena"
            at += p["hdr_len"]
            raw, body, reg = b"", b"", 0xFFFFFFFF
        d = data[at:at + o["deflate_len"]]
        assert o["crc_reg"] == zlib.crc32(p["body"]) ^ zlib.crc32(bytes(p["len"])), "the register from 0, not inverted"
        reg = _crc_mul(reg, _crc_shift(p["len"])) ^ o["crc_reg"]
        raw += d
        body += p["body"]
        assert reg ^ 0xFFFFFFFF == zlib.crc32(body), "the host's running register"
        if not p["last"]:
            assert d.endswith(b"\x00\x00\xff\xff") if p["len"] else d == b"", "the joiner; an empty piece writes nothing"
            continue
        if not body:
            assert raw == EMPTY_STREAM
        assert o["zip64"] == 0
        desc = data[at + o["deflate_len"]:at + o["deflate_len"] + 16]
        assert desc == struct.pack("<IIII", 0x08074B50, zlib.crc32(body), p["csize_before"] + o["deflate_len"], len(body))
        z = zlib.decompressobj(-15)
        assert z.decompress(raw) == body and z.eof and z.unused_data == b""


def test_a_short_out_cap_writes_nothing_and_names_the_total(direct):
    src, headers, pieces, total, _, _ = direct
    for short in (total - 1, total // 2, 0):
        buf = torch.full((SLACK + total + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.CdcError) as e:
            archive.zip_pieces_device(src, pieces, headers, buf[SLACK:], out_cap=short)
        assert e.value.status == _lib.CDC_E_NOSPACE and e.value.total == total
        assert (buf.cpu().numpy() == SENTINEL).all(), "nothing is written when the pieces do not fit"
    buf = torch.full((SLACK + total + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")
    got, _ = archive.zip_pieces_device(src, pieces, headers, buf[SLACK:], out_cap=total)       # exactly enough
    host = buf.cpu().numpy()
    assert got == total and host[SLACK:SLACK + total].tobytes() == direct[5] and (host[SLACK + total:] == SENTINEL).all()


def test_the_descriptor_takes_the_zip64_form_when_a_total_needs_it():
    body = random_bytes(SPAN, 9).tobytes()
    src = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).cuda()
    out = torch.empty(archive.zip_piece_bound(SPAN, 0), dtype=torch.uint8, device="cuda")
    reg = zlib.crc32(b"before") ^ 0xFFFFFFFF
    want_crc = zlib.crc32(body, zlib.crc32(b"before"))
    cases = [(0xFFFFFFF0, 6, True), (0, 6, False), (0, 0xFFFFFFFF - SPAN, True), (0, 0xFFFFFFFE - SPAN, False)]
    for cs0, us0, z64 in cases:
        p = dict(off=0, len=SPAN, first=False, last=True, crc_reg=reg, csize_before=cs0, usize_before=us0)
        total, (o,) = archive.zip_pieces_device(src, [p], b"", out)
        d = out[:total].cpu().numpy().tobytes()
        assert o["zip64"] == int(z64) and total == o["deflate_len"] + (24 if z64 else 16)
        desc = d[o["deflate_len"]:]
        cs, us = cs0 + o["deflate_len"], us0 + SPAN
        assert desc == struct.pack("<IIQQ" if z64 else "<IIII", 0x08074B50, want_crc, cs, us)
    # 0xFFFFFFFF itself is already the 64-bit form (archive/zip's isZip64)
    p = dict(off=0, len=SPAN, first=False, last=True, crc_reg=reg, csize_before=0, usize_before=0)
    _, (o,) = archive.zip_pieces_device(src, [p], b"", out)
    p["csize_before"] = 0xFFFFFFFF - o["deflate_len"]
    assert archive.zip_pieces_device(src, [p], b"", out)[1][0]["zip64"] == 1
    p["csize_before"] -= 1
    assert archive.zip_pieces_device(src, [p], b"", out)[1][0]["zip64"] == 0


def test_encode_is_untouched(direct):
    src, headers, pieces, total, _, data = direct
    blobs = [text_like(70001, 3), random_bytes(SPAN + 5, 4).tobytes(), b"\x07" * 300]
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    before = encode.encode_blobs(blobs, compress="GZIP")
    archive.zip_pieces_device(src, pieces, headers, out)
    during = encode.encode_blobs(blobs, compress="GZIP")
    archive.zip_pieces_device(src, pieces, headers, out)
    after = encode.encode_blobs(blobs, compress="GZIP")
    assert before == during == after
    assert [zlib.decompress(m, 31) for m in after] == blobs
    assert out.cpu().numpy().tobytes() == data, "and the pass gives the same bytes again"


# ---- failures -------------------------------------------------------------------------------------------
def _obj(chunks):
    return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in chunks])


def test_a_missing_blob_leaves_its_entry_out_and_the_archive_valid(corpus, backups):
    _, files = corpus
    objs, packs = backups(None, None)
    chunks5 = [(bytes(c.Checksum), c.Length) for c in objs[5].Chunks]
    missing = _obj(chunks5[:2] + [(hashlib.sha256(b"in no packfile").digest(), 1234)] + chunks5[2:])
    ents = [ArchiveEntry("first", objs[4], mtime=1_700_000_000), ArchiveEntry("lost", missing, mtime=1_700_000_002),
            ArchiveEntry("d", directory=True, mtime=3), ArchiveEntry("last", objs[5], mtime=1_700_000_004)]
    data, statuses, st = archive.zip_files(ents, packs, key=None, compression=None)
    assert statuses == [0, _lib.CDC_E_NOTFOUND, 0, 0]
    assert st["entries"] == 2 and st["skipped_entries"] == 1
    _check_zip(data, [(ents[0], 4), (ents[3], 5)], files)
    assert b"lost" not in data, "no orphan header and no directory record"


def _damage(packs, checksum):
    """The packfiles with one byte flipped in the middle of that chunk's blob."""
    out, hit = [], 0
    for p in packs:
        _, rows = restore.packfile_index(p)
        for _, c, o, n in rows:
            if c == checksum and n:
                b = bytearray(p)
                b[o + n // 2] ^= 0x10
                p = bytes(b)
                hit += 1
        out.append(p)
    assert hit == 1
    return out


def test_a_damaged_blob_ends_the_run_and_leaves_no_file(backups, tmp_path):
    objs, packs = backups(KEY, "LZ4")
    bad = _damage(packs, bytes(objs[5].Chunks[2].Checksum))
    ents = [ArchiveEntry("ok", objs[3], mtime=1), ArchiveEntry("hurt", objs[5], mtime=2), ArchiveEntry("after", objs[4])]
    path = str(tmp_path / "out.zip")
    pieces = []
    for kw in (dict(path=path), dict(on_data=pieces.append)):
        with pytest.raises(_lib.CdcError) as e:
            archive.zip_files(ents, bad, key=KEY, compression="LZ4", batch_bytes=SMALL_BATCH, **kw)
        assert e.value.status == _lib.CDC_E_AUTH and e.value.entry == 1, "the run's status names the entry"
        assert not os.path.exists(path)
    good = archive.zip_files(ents, packs, key=KEY, compression="LZ4", batch_bytes=SMALL_BATCH)[0]
    assert len(b"".join(pieces)) < len(good) and good.startswith(b"".join(pieces)), "nothing more is written after the failure"


def test_an_archive_without_files_is_the_end_record(backups):
    objs, packs = backups(None, None)
    dirs = [ArchiveEntry("d", directory=True), ArchiveEntry("d/e", directory=True, mtime=5)]
    for ents in (dirs, []):
        data, statuses, st = archive.zip_files(ents, packs, key=None, compression=None)
        assert data == END_RECORD and statuses == [0] * len(ents) and st["entries"] == 0 and st["batches"] == 0
        assert zipfile.ZipFile(io.BytesIO(data)).namelist() == []


def _three(objs, hurt=None):
    return [ArchiveEntry("ok", objs[3], mtime=1), ArchiveEntry("hurt", hurt or objs[5], mtime=2), ArchiveEntry("after", objs[4])]


@pytest.mark.parametrize("how", ["removed", "truncated"])
def test_an_unreadable_packfile_ends_the_run_and_names_the_entry(backups, tmp_path, how):
    """Registered by path, then lost before the run: CDC_E_IO, the first entry
    with a blob in the lost bytes named, no file left."""
    objs, packs = backups(KEY, "LZ4")
    ents = _three(objs)
    paths = pack_loss.write_packs(tmp_path, packs)
    path = str(tmp_path / "out.zip")
    with archive.ZipSession(key=KEY, writers=3) as s:
        for q in paths:
            s.add_packfile(q)
        used = [e.obj for e in ents]
        lost = pack_loss.lose(paths, packs, pack_loss.first_home(packs)[bytes(objs[5].Chunks[0].Checksum)][0], how, used)
        want = next(i for i, o in enumerate(used) if pack_loss.first_lost(o, lost) is not None)
        with pytest.raises(_lib.CdcError) as e:
            s.run(ents, path=path)
    assert e.value.status == _lib.CDC_E_IO and e.value.entry == want
    assert not os.path.exists(path)


@pytest.mark.parametrize("key,compression", CONFIGS[:2], ids=IDS[:2])
@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
def test_a_wrong_recorded_length_ends_the_run_and_names_the_entry(backups, tmp_path, delta, key, compression):
    objs, packs = backups(key, compression)
    chunks5 = [(bytes(c.Checksum), c.Length) for c in objs[5].Chunks]
    (c0, n0) = chunks5[0]
    ents = _three(objs, _obj([(c0, n0 + delta)] + chunks5[1:]))
    path = str(tmp_path / "out.zip")
    with pytest.raises(_lib.CdcError) as e:
        archive.zip_files(ents, packs, path=path, key=key, compression=compression)
    assert e.value.status == _lib.CDC_E_MISMATCH and e.value.entry == 1
    assert not os.path.exists(path)
    good, statuses, st = archive.zip_files(_three(objs), packs, key=key, compression=compression)
    assert statuses == [0, 0, 0] and st["batches"] == 1, "the three entries are one batch"
