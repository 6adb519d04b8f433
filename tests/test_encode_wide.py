"""The compression level (CDC_LEVEL_WIDE: k_lz_seq_wide, a match search with a
32-KiB window before each 8-KiB segment) on the device, GZIP and LZ4 alike:
level 0 writes today's bytes, every reader reads level 1, the window is used
and only the window (never past 32,768, the 4-MiB block or the blob), the
size on text against a zlib yardstick computed here, and the layers that pass
the level on (the gzip stream, the zip pieces, archives, the backup)."""
import ctypes
import functools
import glob
import io
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
from plakar_amd import _lib, archive, decode, encode, restore, snapshot  # noqa: E402
from plakar_amd.archive import ArchiveEntry  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32, 64))
SEG = 8192
SPAN = 32768
WINDOW = 32768
BLOCK = 4 << 20
WALK_MAX = 70_000
SELECTORS = [True, "GZIP"]
IDS = ["lz4", "gzip"]


def _period7(n):
    return (b"abcdefg" * (n // 7 + 1))[:n]


def _kinds(n, seed):
    return [bytes(n), ir.text(n, seed), _period7(n), ir.rnd(n, seed)]


def _inflate_any(sel, enc):
    """The content by the independent reader: liblz4 or zlib."""
    if not enc:
        return b""
    return zlib.decompress(enc, 31) if sel == "GZIP" else crypto_ref.lz4f_decompress(enc)


def _gz_matches(member):
    """Every (position, length, distance) of a gzip member, by the Python walker."""
    out, end, walk = ir.inflate(member, 10)
    assert end + 8 == len(member)
    return out, [m for b in walk for m in b["matches"]]


def _lz4_matches(frame):
    """Per block: (stored, [(position in the block, length, offset)])."""
    blocks = lz4_ref.walk_frame(frame)
    res = []
    for b in blocks:
        pos, ms = 0, []
        for ll, off, ml in b.seqs:
            pos += ll
            if ml:
                ms.append((pos, ml, off))
            pos += ml
        res.append((b.stored, ms))
    return lz4_ref.content(blocks), res


def _tokens(sel, enc):
    """(content, [(position in the blob, length, distance)])."""
    if sel == "GZIP":
        return _gz_matches(enc)
    out, blocks = _lz4_matches(enc)
    return out, [(k * BLOCK + p, ml, off) for k, (_, ms) in enumerate(blocks) for p, ml, off in ms]


# ---- 1. level 0 is today ------------------------------------------------------------------
@functools.lru_cache(None)
def _today_batch():
    out = []
    for i, n in enumerate((SEG - 13, SEG, SEG + 13, SPAN - 1, SPAN, SPAN + 1, 65535, 65536, 65537, 70001)):
        out += _kinds(n, 500 + i)
    return out


def _encode_level_ctypes(blobs, sel, level):
    """cdc_encode_device_level itself, compress-only: the encoded blobs."""
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs) + b"\0", dtype=np.uint8).copy()).cuda()
    cap = sum(encode.encode_bound(len(b), sel, False) for b in blobs)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    oo = np.zeros(len(blobs) + 1, dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    _lib.ensure_init()
    rc = _lib.lib().cdc_encode_device_level(0, ctypes.c_void_p(base.data_ptr()), offs.ctypes.data_as(u64p),
                                            lens.ctypes.data_as(u64p), len(blobs), encode._sel(sel), None, None,
                                            ctypes.c_void_p(out.data_ptr()), cap, oo.ctypes.data_as(u64p), level,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    host = out[:int(oo[-1])].cpu().numpy()
    return [host[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(len(blobs))]


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_level_0_is_today(sel):
    blobs = _today_batch()
    assert len(blobs) == 40
    today = encode.encode_blobs(blobs, compress=sel)
    assert encode.encode_blobs(blobs, compress=sel, level=0) == today
    assert _encode_level_ctypes(blobs, sel, 0) == today
    assert encode.DeviceEncoder(compression="GZIP" if sel == "GZIP" else "LZ4", level=0).encode_many(blobs[:5]) == today[:5]
    # and level 1 is not: the text blobs past one segment shrink
    wide = _encode_level_ctypes(blobs, sel, 1)
    assert wide != today and sum(map(len, wide)) < sum(map(len, today))


def test_a_level_that_does_not_exist_is_refused():
    with pytest.raises(ValueError):
        encode.encode_blobs([b"abc"], level=2)
    base = torch.zeros(64, dtype=torch.uint8, device="cuda")
    oo = (ctypes.c_uint64 * 2)()
    one = (ctypes.c_uint64 * 1)(16)
    zero = (ctypes.c_uint64 * 1)(0)
    for level in (2, -1):
        for comp in (0, 1, 2):
            rc = _lib.lib().cdc_encode_device_level(0, ctypes.c_void_p(base.data_ptr()), zero, one, 1, comp, None, None,
                                                    ctypes.c_void_p(base.data_ptr()), 64, oo, level, None)
            assert rc == _lib.CDC_E_INVALID
    # with no compression the level changes nothing
    b = [ir.text(20000, 3)]
    assert encode.encode_blobs(b, compress=False, level=1) == b


# ---- 2. every reader reads level 1 ----------------------------------------------------------
@functools.lru_cache(None)
def _contents():
    out = []
    for n in range(81):
        out += _kinds(n, n)
    for k in range(1, 6):
        for d in (-13, 13):
            out += _kinds(SEG * k + d, 100 + k)
    for n in (SPAN - 1, SPAN, SPAN + 1):
        out += _kinds(n, 200 + n % 7)
    out += [ir.text(BLOCK + 24 * 1024 + 5, 300), bytes(BLOCK + 5)]
    return out


@functools.lru_cache(None)
def _encoded(sel, sealed):
    contents = _contents()
    enc = encode.encode_blobs(contents, key=KEY if sealed else None, compress=sel, level=1)
    return enc, contents


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_independent_readers_read_level_1(sel):
    enc, contents = _encoded(sel, False)
    walked = 0
    for i, (e, c) in enumerate(zip(enc, contents)):
        assert len(e) <= encode.encode_bound(len(c), sel, False), f"blob {i}: bound"
        assert _inflate_any(sel, e) == c, f"blob {i} ({len(c)} bytes)"
        if not c:
            assert e == b""
        elif sel == "GZIP":
            assert struct.unpack("<II", e[-8:]) == (zlib.crc32(c), len(c))
            if len(c) <= WALK_MAX:
                assert ir.status_of(e) == (0, c), f"blob {i} ({len(c)} bytes): the walker"
                walked += len(c)
        else:
            assert lz4_ref.content(lz4_ref.walk_frame(e)) == c, f"blob {i} ({len(c)} bytes): the strict walker"
    assert walked < 2 << 20


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_the_device_reads_level_1_plain_and_sealed(sel):
    enc, contents = _encoded(sel, False)
    assert decode.decode_blobs(enc, compressed=sel) == contents
    sealed, _ = _encoded(sel, True)
    for i, (e, c) in enumerate(zip(sealed, contents)):
        assert len(e) <= encode.encode_bound(len(c), sel, True), f"blob {i}: bound"
        if len(c) <= WALK_MAX:   # the host's AES-GCM is slow: the two large blobs go through the device below
            assert _inflate_any(sel, crypto_ref.decrypt_stream(KEY, e)[0]) == c, f"blob {i}"
    assert decode.decode_blobs(sealed, key=KEY, compressed=sel) == contents


# ---- 3. the window is used, and only the window -----------------------------------------------
R = ir.rnd(24576, 41)
R37 = ir.rnd(37, 42)
X = ir.rnd(SEG, 43)


def _both_levels(blob, sel):
    return [encode.encode_blobs([blob], compress=sel, level=lv)[0] for lv in (0, 1)]


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
@pytest.mark.parametrize("blob", [R + R, R + R37 + R], ids=["R+R", "R+r37+R"])
def test_a_repeat_24_kib_back_is_found(sel, blob):
    e0, e1 = _both_levels(blob, sel)
    out, toks = _tokens(sel, e1)
    assert out == blob and _inflate_any(sel, e1) == blob
    print(f"level 0: {len(e0)}, level 1: {len(e1)} of {len(blob)}")
    assert any(d > SEG for _, _, d in toks), "some match reaches past 8,192"
    assert all(1 <= d <= WINDOW for _, _, d in toks)
    assert len(e1) < 0.60 * len(blob)
    assert len(e0) > 0.99 * len(blob), "without the window nothing is found"


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_the_distance_ends_at_32768(sel):
    at = X + ir.rnd(24576, 44) + X
    _, e1 = _both_levels(at, sel)
    out, toks = _tokens(sel, e1)
    assert out == at and _inflate_any(sel, e1) == at
    assert max(d for _, _, d in toks) == WINDOW, "a distance of exactly 32,768 is taken"
    assert len(e1) < 0.85 * len(at)
    past = X + ir.rnd(24577, 44) + X
    _, e1 = _both_levels(past, sel)
    out, toks = _tokens(sel, e1)
    assert out == past and _inflate_any(sel, e1) == past
    assert decode.decode_blobs([e1], compressed=sel) == [past]
    assert all(d <= WINDOW for _, _, d in toks), "32,769 is not"


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_nothing_reaches_into_the_4_mib_block_before(sel):
    blob = ir.rnd(BLOCK - len(R), 45) + R + R
    e1 = encode.encode_blobs([blob], compress=sel, level=1)[0]
    assert _inflate_any(sel, e1) == blob
    if sel == "GZIP":
        out, toks = _gz_matches(e1)
        assert out == blob
        second = [(p, ln, d) for p, ln, d in toks if p >= BLOCK]
        assert all(d <= p - BLOCK for p, _, d in second), "a token of block 2 reaches before the block"
    else:
        out, blocks = _lz4_matches(e1)     # the strict walker refuses an offset past its position in the block
        assert out == blob and len(blocks) == 2
        assert all(off <= p for _, ms in blocks for p, _, off in ms)
    assert len(e1) > 0.99 * len(blob), "the second R's twin lies in the block before: it stays"


@pytest.mark.parametrize("sel", SELECTORS, ids=IDS)
def test_nothing_outside_a_blob_is_used(sel):
    A = ir.rnd(12288, 46)
    o1 = 16 * 1024 + 1
    buf = bytearray((A + A)[-o1:])          # the bytes in front of the first blob are A's too
    offs = []
    for want in (1, 7, 15):
        while len(buf) % 16 != want:
            buf += A[-1:]
        offs.append(len(buf))
        buf += A
    buf += A[:64]
    assert [o % 16 for o in offs] == [1, 7, 15]
    base = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).cuda()
    cap = 3 * encode.encode_bound(len(A), sel, False)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(base, offs, [len(A)] * 3, out, compress=sel, level=1)
    host = out[:int(oo[-1])].cpu().numpy()
    for i in range(3):
        e = host[int(oo[i]):int(oo[i + 1])].tobytes()
        assert _inflate_any(sel, e) == A, f"blob {i} decodes on its own"
        assert len(e) > 0.99 * len(A), f"blob {i}: something outside it was used"


# ---- 4. size on text -------------------------------------------------------------------------
@functools.lru_cache(None)
def _text_sets():
    names = sorted(glob.glob(os.path.join(ROOT, "plakar_amd", "csrc", "*"))) + [os.path.join(ROOT, "DESIGN.md")]
    tree = b""
    for p in names:
        if os.path.isfile(p):
            with open(p, "rb") as f:
                tree += f.read()
    return {"text": ir.text(1 << 20, 77), "tree": tree}


def _zlib1_segments(data, with_dict):
    """zlib level 1, raw deflate, each 8-KiB segment on its own; with_dict:
    the 32 KiB before it as preset dictionary."""
    total = 0
    for a in range(0, len(data), SEG):
        d = data[max(0, a - WINDOW):a]
        z = zlib.compressobj(1, zlib.DEFLATED, -15, zdict=d) if with_dict and d else zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(z.compress(data[a:a + SEG]) + z.flush())
    return total


@functools.lru_cache(None)
def _text_sizes(name, sel):
    data = _text_sets()[name]
    e0, e1 = _both_levels(data, sel)
    assert _inflate_any(sel, e1) == data
    return len(e0), len(e1)


@pytest.mark.parametrize("name", ["text", "tree"])
def test_size_on_text(name):
    """Measured on an MI355X (DESIGN.md 5.17 has the table)."""
    data = _text_sets()[name]
    alone, with_dict = _zlib1_segments(data, False), _zlib1_segments(data, True)
    g1 = 1 - with_dict / alone
    z6 = len(zlib.compress(data, 6))
    g0, g1_dev = _text_sizes(name, "GZIP")
    l0, l1 = _text_sizes(name, True)
    print(f"{name}: {len(data)} bytes; zlib 1 segments {alone} -> {with_dict} (g1 {g1:.4f}); zlib 6 whole {z6}; "
          f"GZIP level 0 {g0}, level 1 {g1_dev} (gain {1 - g1_dev / g0:.4f}); LZ4 level 0 {l0}, level 1 {l1}")
    assert g1 > 0.03, "the yardstick itself gains from the window"
    assert 1 - g1_dev / g0 >= g1 / 2
    assert l1 < l0


# ---- 5. the layers ------------------------------------------------------------------------------
def test_gzip_stream_at_level_1():
    p1 = ir.text(40000, 61)
    pieces = [p1, p1[:1], (p1 + p1)[:70000]]
    content = b"".join(pieces)
    sizes = {}
    for level in (0, 1):
        with archive.GzipStream(level=level) as s:
            member = b"".join(s.piece(p, last=i == 2) for i, p in enumerate(pieces))
            with pytest.raises(_lib.CdcError) as ex:
                s.set_level(0)
            assert ex.value.status == _lib.CDC_E_INVALID, "a member is written at one level"
        d = zlib.decompressobj(31)
        assert d.decompress(member) == content and d.eof and d.unused_data == b"", "one member"
        assert struct.unpack("<II", member[-8:]) == (zlib.crc32(content), len(content))
        sizes[level] = len(member)
    assert sizes[1] < sizes[0]
    with archive.GzipStream() as s:
        s.set_level(1)
        s.set_level(0)          # before the first piece the level may still change
        with pytest.raises(ValueError):
            s.set_level(2)


def _local_header(name):
    return struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0x8, 8, 0, 0x21, 0, 0, 0, len(name), 0) + name


def test_zip_pieces_at_level_1():
    body = ir.text(50000, 62)
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
    for level in (0, 1):
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
    assert totals[1] < totals[0]
    with pytest.raises(ValueError):
        archive.zip_pieces_device(src, pieces, b"".join(hdrs), out, level=3)


@pytest.fixture(scope="module")
def small_backup(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_in")
    files = [ir.text(90000, 71), b"", ir.rnd(5000, 72), _period7(40000) + ir.text(30000, 73)]
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i}"
        p.write_bytes(b)
        paths.append(str(p))
    repo = Repository(Configuration("FASTCDC", 4096, 16384, 65536))
    objs, packs, _ = snapshot.backup_files(paths, repo=repo, key=KEY, compression="GZIP", max_size=2 << 20, timestamp=5,
                                           level=1)
    return files, objs, packs


def test_archives_at_level_1(small_backup):
    files, objs, packs = small_backup
    ents = [ArchiveEntry(f"dir/f{i}", o, mtime=1_700_000_000 + i) for i, o in enumerate(objs)]
    sizes = {}
    for level in (0, 1):
        data, statuses, _ = archive.archive_files(ents, packs, key=KEY, compression="GZIP", format="tarball", level=level)
        assert statuses == [0] * 4
        with tarfile.open(fileobj=io.BytesIO(data), mode="r:gz") as t:
            assert [t.extractfile(m).read() for m in t.getmembers() if m.isfile()] == files
        zdata, statuses, _ = archive.zip_files(ents, packs, key=KEY, compression="GZIP", level=level)
        assert statuses == [0] * 4
        z = zipfile.ZipFile(io.BytesIO(zdata))
        assert z.testzip() is None and [z.read(f"dir/f{i}") for i in range(4)] == files
        sizes[level] = (len(data), len(zdata))
    assert sizes[1][0] < sizes[0][0] and sizes[1][1] < sizes[0][1]
    with pytest.raises(ValueError):
        archive.ArchiveSession(level=2)


def test_backup_at_level_1_restores_and_stores_less(small_backup, tmp_path):
    files, objs, packs = small_backup
    contents, statuses, _ = restore.restore_files(objs, packs, key=KEY, compression="GZIP")
    assert list(statuses) == [0] * 4 and [bytes(c) for c in contents] == files
    p = tmp_path / "text"
    p.write_bytes(_text_sets()["text"])
    stored = {}
    for level in (0, 1):
        repo = Repository(Configuration("FASTCDC", 16384, 65536, 262144))
        o, pk, _ = snapshot.backup_files([str(p)], repo=repo, key=None, compression="GZIP", timestamp=5, level=level)
        stored[level] = sum(len(x) for x in pk)
        c, st, _ = restore.restore_files(o, pk, key=None, compression="GZIP")
        assert list(st) == [0] and bytes(c[0]) == _text_sets()["text"]
    print(f"stored bytes: level 0 {stored[0]}, level 1 {stored[1]}")
    assert stored[1] < stored[0]
