"""Restore of a GZIP repository: packfiles built here through packer.Packer.
AddBlob from blobs deflated with zlib (and sealed on the host), then
snapshot.restore_files(compression="GZIP") to callbacks and to paths."""
import hashlib
import os
import types
import zlib

import pytest

torch = pytest.importorskip("torch")

import decode_ref as dr  # noqa: E402
import inflate_ref as ir  # noqa: E402
from plakar_amd import _lib, packer, restore, snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32, 64))
CHUNK = 61_003


def _chunks(data):
    return [data[p:p + CHUNK] for p in range(0, len(data), CHUNK)] or [b""]


def _repository(files, key, level=6):
    """(objects, packfiles, {checksum: (packfile index, blob offset, length)}):
    every distinct chunk deflated once, sealed when there is a key, and packed
    into packfiles of about 100 KB."""
    objs, packs, where, seen = [], [], {}, set()
    pk = packer.Packer(max_size=100_000, timestamp=1)
    off = 0
    for data in files:
        rows = []
        for c in _chunks(data):
            sum_ = hashlib.sha256(c).digest()
            rows.append(types.SimpleNamespace(Checksum=sum_, Length=len(c)))
            if sum_ in seen:
                continue
            seen.add(sum_)
            blob = ir.member(ir.raw_deflate(c, level=level), c)
            if key is not None:
                blob = dr.seal_stream(key, blob, len(seen))
            where[sum_] = (len(packs), off, len(blob))
            off += len(blob)
            if pk.AddBlob(packer.TYPE_CHUNK, sum_, blob):
                packs.append(pk.Serialize())
                pk.Reset()
                off = 0
        objs.append(types.SimpleNamespace(Chunks=rows))
    if pk.Count():
        packs.append(pk.Serialize())
    pk.close()
    return objs, packs, where


@pytest.fixture(scope="module")
def files():
    shared = ir.text(400_000, 40)
    return [b"", ir.text(1000, 41), ir.rnd(150_001, 42), shared + ir.rnd(777, 43), bytes(900_000),
            shared + ir.text(300_000, 44), ir.rnd(20_000, 45) + bytes(100_000) + ir.text(50_000, 46)]


@pytest.mark.parametrize("key", [None, KEY], ids=["plain", "key"])
def test_gzip_repository_restores_byte_for_byte(files, key, tmp_path):
    objs, packs, _ = _repository(files, key)
    assert len(packs) > 1
    contents, statuses, st = snapshot.restore_files(objs, packs, key=key, compression="GZIP")
    assert statuses == [0] * len(files)
    assert contents == files
    assert st["bytes"] == sum(len(f) for f in files) and st["failed_files"] == 0
    dests = [str(tmp_path / f"out{i}") for i in range(len(files))]
    contents, statuses, _ = snapshot.restore_files(objs, packs, dests, key=key, compression="GZIP")
    assert statuses == [0] * len(files) and contents == [None] * len(files)
    for d, want in zip(dests, files):
        with open(d, "rb") as f:
            assert f.read() == want


def test_a_file_listed_twice_decodes_its_blobs_once(files):
    objs, packs, _ = _repository(files[1:3], None)
    twice = [objs[1], objs[0], objs[1]]
    contents, statuses, st = snapshot.restore_files(twice, packs, compression="GZIP")
    assert statuses == [0, 0, 0] and contents == [files[2], files[1], files[2]]
    distinct = len({c.Checksum for o in objs for c in o.Chunks})
    assert st["batches"] == 1 and st["decoded_blobs"] == st["distinct_blobs"] == distinct < st["segments"]


def test_a_file_spans_batches(files):
    objs, packs, _ = _repository([files[4], files[5]], KEY)
    with restore.RestoreSession(key=KEY, compression="GZIP", batch_bytes=256 << 10) as s:
        for p in packs:
            s.add_packfile(p)
        contents, statuses, st = s.run(objs)
    assert statuses == [0, 0] and contents == [files[4], files[5]]
    assert st["batches"] >= 4 and st["pieces"] > 2


@pytest.mark.parametrize("key,status", [(None, _lib.CDC_E_CORRUPT), (KEY, _lib.CDC_E_AUTH)], ids=["plain", "key"])
def test_one_damaged_blob_fails_exactly_the_files_that_use_it(files, key, status):
    objs, packs, where = _repository(files, key)
    victim = objs[3].Chunks[2].Checksum           # in the 400,000 bytes that files 3 and 5 share
    users = [i for i, o in enumerate(objs) if any(c.Checksum == victim for c in o.Chunks)]
    assert users == [3, 5]
    pi, off, n = where[victim]
    _, rows = restore.packfile_index(packs[pi])
    (row,) = [r for r in rows if r[1] == victim]
    assert (row[2], row[3]) == (off, n)
    bad = bytearray(packs[pi])
    bad[off + n // 2] ^= 0x04
    bad_packs = packs[:pi] + [bytes(bad)] + packs[pi + 1:]
    contents, statuses, st = snapshot.restore_files(objs, bad_packs, key=key, compression="GZIP")
    assert statuses == [status if i in users else 0 for i in range(len(files))]
    assert st["failed_files"] == 2
    assert [c for i, c in enumerate(contents) if i not in users] == [f for i, f in enumerate(files) if i not in users]


def test_a_wrong_length_is_a_mismatch(files, tmp_path):
    objs, packs, _ = _repository(files[:4], None)
    ch = [(c.Checksum, c.Length) for c in objs[2].Chunks]

    def obj(rows):
        return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in rows])

    longer, shorter = obj([(ch[0][0], ch[0][1] + 1)] + ch[1:]), obj([(ch[0][0], ch[0][1] - 1)] + ch[1:])
    todo = list(objs) + [longer, shorter]
    contents, statuses, st = snapshot.restore_files(todo, packs, compression="GZIP")
    assert statuses == [0, 0, 0, 0, _lib.CDC_E_MISMATCH, _lib.CDC_E_MISMATCH]
    assert contents[:4] == files[:4] and contents[4:] == [None, None] and st["failed_files"] == 2
    dests = [str(tmp_path / f"o{i}") for i in range(len(todo))]
    _, statuses, _ = snapshot.restore_files(todo, packs, dests, compression="GZIP")
    assert [os.path.exists(d) for d in dests] == [True] * 4 + [False] * 2


def test_blobs_of_this_test_are_what_zlib_reads(files):
    _, packs, where = _repository(files[1:2], None)
    (pi, off, n), = where.values()
    assert zlib.decompress(packs[pi][off:off + n], 31) == files[1]
