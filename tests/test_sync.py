"""Sync end to end (sync.SyncSession): packfiles of one repository in,
packfiles of another out, read back with restore_files and with libcrypto."""
import hashlib

import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, decode, packer, restore, snapshot, sync  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_A = bytes(range(32, 64))
KEY_B = bytes(range(200, 232))


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    """Three small files backed up under key A / LZ4 (test_restore.py's backup
    settings): empty, about 100 KiB, and about 1.5 MiB with a repeated region."""
    d = tmp_path_factory.mktemp("sync")
    region = random_bytes(300_000, 21).tobytes()
    files = [b"", random_bytes(100_003, 20).tobytes(),
             region + random_bytes(500_000, 22).tobytes() + region + random_bytes(400_001, 23).tobytes()]
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i}"
        p.write_bytes(b)
        paths.append(str(p))
    objs, packs, _ = snapshot.backup_files(paths, key=KEY_A, compression="LZ4", max_size=2 << 20, batch_bytes=8 << 20,
                                           timestamp=11)
    return files, objs, packs


def _rows(packs):
    out = []
    for p in packs:
        _, rows = restore.packfile_index(p)
        out += [(t, c, p[o:o + n]) for t, c, o, n in rows]
    return out


def test_round_trip_to_another_key_and_compression(source):
    files, objs, packs = source
    s = sync.SyncSession(src_key=KEY_A, src_compression="LZ4", dst_key=KEY_B, dst_compression="GZIP", timestamp=12)
    for p in packs:
        s.add_packfile(p)
    out, failures, stats = s.run()
    assert failures == {} and stats["failed"] == 0 and stats["path"] == "reencode"
    assert stats["blobs"] == len(_rows(packs)) == len(_rows(out)) and stats["skipped"] == 0
    assert stats["bytes_in"] == sum(len(b) for _, _, b in _rows(packs))
    assert stats["bytes_out"] == sum(len(b) for _, _, b in _rows(out))
    assert stats["batches"] == 1 and stats["packfiles"] == len(out) >= 1
    contents, statuses, _ = snapshot.restore_files(objs, out, key=KEY_B, compression="GZIP", verify=True)
    assert statuses == [0] * len(files) and contents == files
    _, statuses, _ = snapshot.restore_files(objs, out, key=KEY_A, compression="GZIP", verify=True)
    assert statuses == [_lib.CDC_E_AUTH] * len(files)  # the empty file too: its one empty chunk is a sealed blob


def test_rekey_carries_the_compressed_frame_over(source):
    files, objs, packs = source
    s = sync.SyncSession(src_key=KEY_A, dst_key=KEY_B, timestamp=12)
    for p in packs:
        s.add_packfile(p)
    out, failures, stats = s.run()
    assert failures == {} and stats["path"] == "rekey" and stats["bytes_in"] == stats["bytes_out"]
    src_rows, dst_rows = _rows(packs), _rows(out)
    assert [(t, c) for t, c, _ in src_rows] == [(t, c) for t, c, _ in dst_rows]
    for (_, c, a), (_, _, b) in zip(src_rows, dst_rows):
        frame = crypto_ref.decrypt_stream(KEY_A, a)[0]
        assert crypto_ref.decrypt_stream(KEY_B, b)[0] == frame and a != b
        assert hashlib.sha256(crypto_ref.decode(a, KEY_A, True)).digest() == c
    contents, statuses, _ = snapshot.restore_files(objs, out, key=KEY_B, compression="LZ4", verify=True)
    assert statuses == [0] * len(files) and contents == files


def test_known_blobs_are_skipped(source):
    _, _, packs = source
    known = {(t, c) for t, c, _ in _rows(packs)}
    s = sync.SyncSession(src_key=KEY_A, dst_key=KEY_B, known=known)
    for p in packs:
        s.add_packfile(p)
    out, failures, stats = s.run()
    assert out == [] and failures == {}
    assert stats["blobs"] == 0 and stats["skipped"] == len(_rows(packs)) and stats["batches"] == 0
    # `wanted` narrows the run to the pairs it names
    some = sorted(known)[:2]
    s = sync.SyncSession(src_key=KEY_A, dst_key=KEY_B)
    for p in packs:
        s.add_packfile(p)
    out, failures, stats = s.run(wanted=some)
    assert sorted((t, c) for t, c, _ in _rows(out)) == some and stats["blobs"] == 2


def _typed_packfile():
    """Blobs of types 1 to 5 under key A / LZ4, one checksum under two types,
    and one row whose bytes are damaged."""
    pk = packer.Packer(timestamp=5)
    rows = []
    for i, t in enumerate([1, 2, 3, 4, 5, 3, 1]):
        content = dr.rnd(1000 + 700 * i, 900 + i) if i != 5 else dr.rnd(1000, 900)  # row 5: row 0's content again
        blob = dr.seal_stream(KEY_A, dr.lz4f_compress(content), 910 + i)
        if i == 6:
            blob = dr.flip(blob, 100)
        c = hashlib.sha256(content).digest()
        pk.AddBlob(t, c, blob)
        rows.append((t, c, content))
    raw = pk.Serialize()
    pk.close()
    return raw, rows


def test_every_blob_type_is_carried_and_a_failed_blob_is_reported():
    raw, rows = _typed_packfile()
    assert rows[0][1] == rows[5][1] and rows[0][0] != rows[5][0]
    s = sync.SyncSession(src_key=KEY_A, dst_key=KEY_B, dst_compression="GZIP", timestamp=6)
    s.add_packfile(raw)
    s.add_packfile(raw)  # every row a second time: already taken in this run
    out, failures, stats = s.run()
    assert failures == {(1, rows[6][1]): _lib.CDC_E_AUTH}
    assert stats["blobs"] == 7 and stats["failed"] == 1 and stats["skipped"] == 7
    got = _rows(out)
    assert [(t, c) for t, c, _ in got] == [(t, c) for t, c, _ in rows[:6]]  # in order, the duplicate checksum twice
    plains = decode.decode_blobs([b for _, _, b in got], key=KEY_B, compressed="GZIP")
    assert plains == [content for _, _, content in rows[:6]]


def test_a_small_max_size_flushes_several_packfiles(source):
    files, objs, packs = source
    s = sync.SyncSession(src_key=KEY_A, dst_key=KEY_B, max_size=256 << 10, batch_bytes=1 << 20, timestamp=12)
    for p in packs:
        s.add_packfile(p)
    out, failures, stats = s.run()
    assert failures == {} and len(out) > 1 and stats["batches"] > 1
    n = 0
    for p in out:
        footer, rows = restore.packfile_index(p)
        assert footer["count"] == len(rows) >= 1 and footer["timestamp"] == 12
        n += len(rows)
    assert n == len(_rows(packs))
    contents, statuses, _ = snapshot.restore_files(objs, out, key=KEY_B, compression="LZ4", verify=True)
    assert statuses == [0] * len(files) and contents == files
