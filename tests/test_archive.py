"""The archive path on the device (cdc_archive_run, plakar_amd.archive): a
backed-up corpus written as tar and as tarball.  Python's tarfile lists the
same names, types, sizes, modes and mtimes with equal contents, the bytes do
not depend on the batch budget, the tarball is one gzip member of exactly the
tar stream, the two sinks agree, an entry with a blob in no packfile is left
out whole, and a damaged blob ends the run and leaves no file."""
import hashlib
import io
import os
import tarfile
import types
import zlib

import pytest

torch = pytest.importorskip("torch")

import pack_loss  # noqa: E402
from datagen import low_entropy, random_bytes  # noqa: E402
from plakar_amd import _lib, archive, restore, snapshot  # noqa: E402
from plakar_amd.archive import ArchiveEntry  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))
SIZES = [0, 1, 511, 512, 513, 300_000]
LONG_SPLIT = "d" * 154 + "/" + "f" * 100            # 255 bytes: prefix and name
LONG_PAX = "p" * 150 + "/" + "n" * 104              # no valid split: a PAX path
OVER_255 = "q" * 200 + "/" + "r" * 99               # 300 bytes
NON_ASCII = "café/naïve.txt"
CONFIGS = [(None, None), (KEY, "LZ4")]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("archive_in")
    files = [b"" if n == 0 else random_bytes(n, 40 + i).tobytes() if i % 2 == 0 else low_entropy(n, 40 + i).tobytes()
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
    """(ArchiveEntry, content index or None) in archive order."""
    names = ["empty", "one", "dir/511", "dir/512", "dir/sub/513", "big.bin"]
    out = [(ArchiveEntry("dir", directory=True, mode=0o750, mtime=1_600_000_000), None)]
    out += [(ArchiveEntry(n, objs[i], mode=0o600 + i, mtime=1_700_000_000 + i), i) for i, n in enumerate(names)]
    out.append((ArchiveEntry("dir/sub", directory=True, mtime=5), None))
    out.append((ArchiveEntry("again/big.bin", objs[5], mtime=6), 5))                 # the same file twice
    out.append((ArchiveEntry("a" * 100, objs[1], mtime=7), 1))
    out.append((ArchiveEntry("dir/" + "b" * 97, objs[2], mtime=8), 2))               # 101 bytes
    out.append((ArchiveEntry(LONG_SPLIT, objs[3], mtime=9), 3))
    out.append((ArchiveEntry(LONG_PAX, objs[4], mtime=10), 4))
    out.append((ArchiveEntry(OVER_255, objs[5], mtime=11), 5))
    out.append((ArchiveEntry(NON_ASCII, objs[2], mtime=-1), 2))                       # PAX path and mtime
    return out


def _tar(objs, packs, key, compression, fmt="tar", **kw):
    ents = _entries(objs)
    data, statuses, st = archive.archive_files([e for e, _ in ents], packs, key=key, compression=compression, format=fmt,
                                               **kw)
    assert statuses == [0] * len(ents)
    return data, st, ents


def _check_tar(data, ents, files):
    assert len(data) % 512 == 0 and data.endswith(bytes(1024))
    t = tarfile.open(fileobj=io.BytesIO(data), mode="r:")
    members = t.getmembers()
    assert [m.name for m in members] == [e.name.decode().rstrip("/") for e, _ in ents]
    end = 0
    for m, (e, i) in zip(members, ents):
        assert m.isdir() == e.directory and m.isfile() == (not e.directory)
        assert (m.mode, m.mtime, m.uid, m.gid) == (e.mode, e.mtime, 0, 0)
        assert m.size == (0 if i is None else len(files[i]))
        if i is not None:
            assert t.extractfile(m).read() == files[i], m.name
        end = m.offset_data + -(-m.size // 512) * 512
    assert end + 1024 == len(data), "1,024 zeros after the last entry and no blocking-factor padding"


@pytest.fixture(scope="module")
def one_batch(corpus, backups):
    """The tar stream of each configuration in one batch, made once."""
    made = {}

    def get(key, compression):
        if (key, compression) not in made:
            made[(key, compression)] = _tar(*backups(key, compression), key, compression)
        return made[(key, compression)]
    return get


@pytest.mark.parametrize("key,compression", CONFIGS, ids=["plain", "lz4-sealed"])
def test_tar_lists_the_entries_with_equal_contents(corpus, one_batch, key, compression):
    _, files = corpus
    data, st, ents = one_batch(key, compression)
    _check_tar(data, ents, files)
    assert st["batches"] == 1 and st["entries"] == len(ents) and st["skipped_entries"] == 0
    assert st["stream_bytes"] == st["output_bytes"] == len(data)
    chunks = [(bytes(c.Checksum), c.Length) for e, _ in ents if e.obj is not None for c in e.obj.Chunks if c.Length]
    assert st["decoded_blobs"] == len(set(chunks)) < len(chunks), "a blob used three times is decoded once"


def test_both_configurations_give_the_same_tar(one_batch):
    assert one_batch(*CONFIGS[0])[0] == one_batch(*CONFIGS[1])[0]


@pytest.mark.parametrize("key,compression", CONFIGS, ids=["plain", "lz4-sealed"])
@pytest.mark.parametrize("budget", [64 << 10, 4096 + 512])
def test_tar_does_not_depend_on_the_batch_budget(backups, one_batch, key, compression, budget):
    want, st1, _ = one_batch(key, compression)
    data, st, _ = _tar(*backups(key, compression), key, compression, batch_bytes=budget)
    assert data == want
    assert st["batches"] > 4 and st["stream_bytes"] == len(want)
    assert st["decoded_blobs"] > st1["decoded_blobs"], "a blob is decoded again in every batch that uses it"


@pytest.mark.parametrize("key,compression", CONFIGS, ids=["plain", "lz4-sealed"])
@pytest.mark.parametrize("budget", [archive.DEFAULT_BATCH_BYTES, 64 << 10])
def test_tarball_inflates_as_one_member_to_the_tar_stream(backups, one_batch, key, compression, budget):
    want, _, _ = one_batch(key, compression)
    data, st, _ = _tar(*backups(key, compression), key, compression, fmt="tarball", batch_bytes=budget)
    d = zlib.decompressobj(31)
    assert d.decompress(data) == want and d.eof and d.unused_data == b""
    assert st["stream_bytes"] == len(want) and st["output_bytes"] == len(data) < len(want)
    assert st["batches"] == 1 if budget > 1 << 20 else st["batches"] > 4
    assert data[:10] == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF]) and data.count(data[:10]) == 1
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:gz") as t:
        assert len(t.getmembers()) == len(_entries(backups(key, compression)[0]))


@pytest.mark.parametrize("fmt", ["tar", "tarball"])
def test_the_sinks_agree(backups, tmp_path, fmt):
    objs, packs = backups(KEY, "LZ4")
    ents = [e for e, _ in _entries(objs)]
    path = str(tmp_path / ("out." + fmt))
    pieces = []
    with archive.ArchiveSession(key=KEY, format=fmt, batch_bytes=64 << 10) as s:
        for p in packs:
            s.add_packfile(p)
        none, statuses, st = s.run(ents, path=path)
        assert none is None and statuses == [0] * len(ents)
        none, statuses, st2 = s.run(ents, on_data=pieces.append)         # the same session, a second run
        assert none is None and statuses == [0] * len(ents)
    with open(path, "rb") as f:
        on_disk = f.read()
    assert len(pieces) == st2["batches"] > 4 and b"".join(pieces) == on_disk
    assert st["output_bytes"] == st2["output_bytes"] == len(on_disk)
    if fmt == "tar":
        assert on_disk == _tar(objs, packs, KEY, "LZ4")[0]
    else:
        assert zlib.decompress(on_disk, 31) == _tar(objs, packs, KEY, "LZ4")[0]
    # packfiles by path
    pack_paths = []
    for i, p in enumerate(packs):
        q = tmp_path / f"pack{i}"
        q.write_bytes(p)
        pack_paths.append(str(q))
    data, statuses, _ = archive.archive_files(ents, pack_paths, key=KEY, format=fmt, batch_bytes=64 << 10)
    assert data == on_disk


def _obj(chunks):
    return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in chunks])


@pytest.mark.parametrize("fmt", ["tar", "tarball"])
def test_a_missing_blob_leaves_its_entry_out_and_the_archive_valid(corpus, backups, fmt):
    _, files = corpus
    objs, packs = backups(None, None)
    chunks5 = [(bytes(c.Checksum), c.Length) for c in objs[5].Chunks]
    missing = _obj(chunks5[:2] + [(hashlib.sha256(b"in no packfile").digest(), 1234)] + chunks5[2:])
    ents = [ArchiveEntry("first", objs[4], mtime=1), ArchiveEntry("lost", missing, mtime=2),
            ArchiveEntry("d", directory=True, mtime=3), ArchiveEntry("last", objs[5], mtime=4)]
    data, statuses, st = archive.archive_files(ents, packs, key=None, compression=None, format=fmt)
    assert statuses == [0, _lib.CDC_E_NOTFOUND, 0, 0]
    assert st["entries"] == 3 and st["skipped_entries"] == 1
    tar = zlib.decompress(data, 31) if fmt == "tarball" else data
    _check_tar(tar, [(ents[0], 4), (ents[2], None), (ents[3], 5)], files)
    assert b"lost" not in tar, "no orphan header"


def _damage(packs, checksum, where):
    """The packfiles with one bit flipped in that chunk's blob: in its last 16 bytes (a tag) or its middle."""
    out, hit = [], 0
    for p in packs:
        _, rows = restore.packfile_index(p)
        for _, c, o, n in rows:
            if c == checksum and n:
                b = bytearray(p)
                b[o + (n - 3 if where == "tag" else n // 2)] ^= 0x10
                p = bytes(b)
                hit += 1
        out.append(p)
    assert hit == 1
    return out


@pytest.mark.parametrize("key,compression,where,status", [(KEY, "LZ4", "tag", _lib.CDC_E_AUTH),
                                                          (None, None, "frame", _lib.CDC_E_MISMATCH)],
                         ids=["a-tag-bit", "a-frame-bit-no-key"])
@pytest.mark.parametrize("fmt", ["tar", "tarball"])
def test_a_damaged_blob_ends_the_run_and_leaves_no_file(backups, tmp_path, key, compression, where, status, fmt):
    objs, packs = backups(key, compression)
    victim = bytes(objs[5].Chunks[2].Checksum)
    bad = _damage(packs, victim, where)
    ents = [ArchiveEntry("ok", objs[3], mtime=1), ArchiveEntry("hurt", objs[5], mtime=2), ArchiveEntry("after", objs[4])]
    path = str(tmp_path / "out")
    pieces = []
    for kw in (dict(path=path), dict(on_data=pieces.append)):
        with pytest.raises(_lib.CdcError) as e:
            archive.archive_files(ents, bad, key=key, compression=compression, format=fmt, batch_bytes=64 << 10, **kw)
        assert e.value.status == status and e.value.entry == 1, "the run's status names the entry"
        assert not os.path.exists(path)
    good = archive.archive_files(ents, packs, key=key, compression=compression, format=fmt, batch_bytes=64 << 10)[0]
    assert len(b"".join(pieces)) < len(good), "nothing more is written after the failure"
    assert good.startswith(b"".join(pieces))


def _three(objs, hurt=None):
    return [ArchiveEntry("ok", objs[3], mtime=1), ArchiveEntry("hurt", hurt or objs[5], mtime=2), ArchiveEntry("after", objs[4])]


@pytest.mark.parametrize("how", ["removed", "truncated"])
@pytest.mark.parametrize("fmt", ["tar", "tarball"])
def test_an_unreadable_packfile_ends_the_run_and_names_the_entry(backups, tmp_path, fmt, how):
    """Registered by path, then lost before the run: CDC_E_IO, the first entry
    with a blob in the lost bytes named, no file left."""
    objs, packs = backups(KEY, "LZ4")
    ents = _three(objs)
    paths = pack_loss.write_packs(tmp_path, packs)
    path = str(tmp_path / "out")
    with archive.ArchiveSession(key=KEY, format=fmt, writers=3) as s:
        for q in paths:
            s.add_packfile(q)
        used = [e.obj for e in ents]
        lost = pack_loss.lose(paths, packs, pack_loss.first_home(packs)[bytes(objs[5].Chunks[0].Checksum)][0], how, used)
        want = next(i for i, o in enumerate(used) if pack_loss.first_lost(o, lost) is not None)
        with pytest.raises(_lib.CdcError) as e:
            s.run(ents, path=path)
    assert e.value.status == _lib.CDC_E_IO and e.value.entry == want
    assert not os.path.exists(path)


@pytest.mark.parametrize("key,compression", CONFIGS, ids=["plain", "lz4-sealed"])
@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
@pytest.mark.parametrize("fmt", ["tar", "tarball"])
def test_a_wrong_recorded_length_ends_the_run_and_names_the_entry(backups, tmp_path, fmt, delta, key, compression):
    objs, packs = backups(key, compression)
    chunks5 = [(bytes(c.Checksum), c.Length) for c in objs[5].Chunks]
    (c0, n0) = chunks5[0]
    ents = _three(objs, _obj([(c0, n0 + delta)] + chunks5[1:]))
    path = str(tmp_path / "out")
    with pytest.raises(_lib.CdcError) as e:
        archive.archive_files(ents, packs, path=path, key=key, compression=compression, format=fmt)
    assert e.value.status == _lib.CDC_E_MISMATCH and e.value.entry == 1
    assert not os.path.exists(path)
    good, statuses, st = archive.archive_files(_three(objs), packs, key=key, compression=compression, format=fmt)
    assert statuses == [0, 0, 0] and st["batches"] == 1, "the three entries are one batch"


@pytest.mark.parametrize("key,compression", CONFIGS, ids=["plain", "lz4-sealed"])
def test_two_wrong_lengths_in_one_batch_name_the_first_entry(backups, key, compression):
    """One blob decodes shorter than its recorded Length, a later one longer
    (by more, so the batch overflows its plaintext room and is decoded one by
    one): the run names the first wrong entry, as it does when nothing
    overflows."""
    objs, packs = backups(key, compression)
    bad = []
    for i, delta in ((5, 1), (2, -2)):
        chunks = [(bytes(c.Checksum), c.Length) for c in objs[i].Chunks]
        (c0, n0) = chunks[0]
        bad.append(_obj([(c0, n0 + delta)] + chunks[1:]))
    ents = [ArchiveEntry("ok", objs[3], mtime=1), ArchiveEntry("short", bad[0], mtime=2),
            ArchiveEntry("long", bad[1], mtime=3), ArchiveEntry("after", objs[4])]
    for order in (ents, [ents[0], ents[2], ents[1], ents[3]]):
        with pytest.raises(_lib.CdcError) as e:
            archive.archive_files(order, packs, key=key, compression=compression, format="tar")
        assert e.value.status == _lib.CDC_E_MISMATCH and e.value.entry == 1
