"""Byte ranges of files on the device (cdc_restore_ranges, snapshot.read_ranges,
restore.SnapshotFile): every range against a slice of the source file, the
work counters against the chunk lists, per-range failures, and the file object
with VFilep's rules."""
import io
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pack_loss  # noqa: E402
from datagen import low_entropy, random_bytes  # noqa: E402
from plakar_amd import _lib, restore, snapshot  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32, 64))
MIB = 1 << 20
REPOS = [(KEY, "LZ4"), (KEY, "GZIP"), (None, None)]
IDS = ["lz4-key", "gzip-key", "none"]
SMALL = 256 << 10


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("ranges")
    block = random_bytes(150_000, 5).tobytes()
    mixed = low_entropy(MIB, 3).tobytes() + random_bytes(MIB, 4).tobytes() + low_entropy(MIB + 17, 6).tobytes()
    files = [b"",                                   # empty
             random_bytes(1, 1).tobytes(),          # one byte
             low_entropy(9000, 2).tobytes(),        # under MinSize: one chunk, no CDC
             mixed,                                 # multi-chunk
             random_bytes(2 * MIB + 5, 7).tobytes(),  # multi-chunk
             mixed,                                 # a duplicate
             block * 12]                            # repeats its chunks
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
            repo = Repository(Configuration("FASTCDC", 16384, 65536, 262144))
            objs, packs, _ = snapshot.backup_files(paths, repo=repo, key=key, compression=compression,
                                                   max_size=1 << 20, batch_bytes=8 << 20, timestamp=5)
            made[(key, compression)] = (objs, packs)
        return made[(key, compression)]
    return get


def _starts(obj):
    return np.concatenate([[0], np.cumsum([c.Length for c in obj.Chunks])]).astype(np.int64)


def _ranges(objs):
    """Every chunk boundary +- 1 as a start and as an end, the edge cases, whole
    files; in an order that is not the files'."""
    rs = []
    for fi in (3, 4):
        s = _starts(objs[fi])
        size = int(s[-1])
        assert len(s) > 24, "dozens of chunks"
        for b in s[1:-1]:
            for d in (-1, 0, 1):
                at = int(b) + d
                rs.append((fi, at, 5000))                        # begins there
                rs.append((fi, max(at - 70_000, 0), min(at, 70_000)))  # ends there, a chunk or two before
        rs += [(fi, size, 10), (fi, 100, 0), (fi, size - 10, 1000), (fi, 0, size), (fi, 0, size + 99)]
    rs += [(3, 1000, 200_000), (3, 50_000, 200_000), (3, 1000, 200_000)]    # overlapping, and one twice
    rs += [(0, 0, 10), (0, 0, 0), (1, 0, 1), (1, 0, 100), (1, 1, 5), (2, 10, 100), (2, 0, 9000), (2, 8999, 1)]
    rs += [(5, 12345, 300_000), (6, 149_999, 150_002), (6, 0, 1_800_000), (6, 1_000_000, 1)]
    order = np.random.default_rng(8).permutation(len(rs))
    return [rs[i] for i in order]


def _plan(objs, ranges, budget):
    """read_plan.h's rule restated: per batch, {(checksum, recorded length): upto}."""
    batches, cur, out, dec = [], {}, 0, 0
    for fi, off, ln in ranges:
        s = _starts(objs[fi])
        size = int(s[-1])
        if off > size:
            continue
        end = off + min(ln, size - off)
        for c, ch in enumerate(objs[fi].Chunks):
            lo, hi = max(int(s[c]), off), min(int(s[c + 1]), end)
            if hi <= lo:
                continue
            k = (bytes(ch.Checksum), int(ch.Length))
            in_hi = hi - int(s[c])
            grow = max(0, in_hi - cur.get(k, 0))
            if (out or dec) and (out + hi - lo > budget or dec + grow > budget):
                batches.append(cur)
                cur, out, dec, grow = {}, 0, 0, in_hi
            cur[k] = max(cur.get(k, 0), in_hi)
            out += hi - lo
            dec += grow
    if cur:
        batches.append(cur)
    return batches


def _counters(plan):
    blobs = [(k, u) for b in plan for k, u in b.items()]
    return dict(decoded_bytes=sum(u for _, u in blobs), whole_blobs=sum(1 for k, u in blobs if u == k[1]),
                prefix_blobs=sum(1 for k, u in blobs if u < k[1]),
                skipped_bytes=sum(k[1] - u for k, u in blobs), batches=len(plan))


def _hold(files, ranges, contents, statuses):
    for i, ((fi, off, ln), got, st) in enumerate(zip(ranges, contents, statuses)):
        assert st == 0, (i, ranges[i], st)
        assert got == files[fi][off:off + ln], f"range {i}: {ranges[i]}"


@pytest.mark.parametrize("key,compression", REPOS, ids=IDS)
def test_ranges_are_slices_and_the_counters_follow_the_chunk_lists(corpus, backups, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    assert len(packs) > 2
    ranges = _ranges(objs)
    got = {}
    for budget in (restore.DEFAULT_BATCH_BYTES, SMALL):
        contents, statuses, st = snapshot.read_ranges(objs, ranges, packs, key=key, compression=compression,
                                                      batch_bytes=budget)
        _hold(files, ranges, contents, statuses)
        want = _counters(_plan(objs, ranges, budget))
        for k, v in want.items():
            assert st[k] == v, (k, st[k], v, budget)
        assert st["verified_blobs"] == st["whole_blobs"] and st["failed_ranges"] == 0 and st["ranges"] == len(ranges)
        assert st["bytes"] == sum(len(c) for c in contents)
        got[budget] = contents
    assert got[SMALL] == got[restore.DEFAULT_BATCH_BYTES]
    assert _counters(_plan(objs, ranges, SMALL))["batches"] > 10, "ranges were cut into pieces, batches multiplied"


@pytest.mark.parametrize("key,compression", REPOS, ids=IDS)
def test_the_first_4k_of_every_file_costs_4k_each(corpus, backups, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    ranges = [(i, 0, 4096) for i in range(len(files))]
    contents, statuses, st = snapshot.read_ranges(objs, ranges, packs, key=key, compression=compression, verify=False)
    _hold(files, ranges, contents, statuses)
    assert st["decoded_bytes"] <= 4096 * len(files) and st["verified_blobs"] == 0
    assert st["decoded_bytes"] == _counters(_plan(objs, ranges, restore.DEFAULT_BATCH_BYTES))["decoded_bytes"]
    assert st["skipped_bytes"] > 100_000 and st["prefix_blobs"] >= 3


def test_an_offset_past_the_size_fails_that_range_only(corpus, backups):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    ranges = [(3, 10, 100), (3, len(files[3]) + 1, 1), (7, 0, 1), (0, 1, 0), (3, len(files[3]), 5), (4, 5, 5)]
    contents, statuses, st = snapshot.read_ranges(objs, ranges, packs, key=KEY)
    E = _lib.CDC_E_INVALID
    assert statuses == [0, E, E, E, 0, 0] and st["failed_ranges"] == 3
    assert contents == [files[3][10:110], None, None, None, b"", files[4][5:10]]


def _touch(objs, r, sums):
    fi, off, ln = r
    s = _starts(objs[fi])
    end = min(off + ln, int(s[-1]))
    return any(bytes(ch.Checksum) in sums and max(int(s[c]), off) < min(int(s[c + 1]), end)
               for c, ch in enumerate(objs[fi].Chunks))


def test_a_packfile_left_out_fails_exactly_the_ranges_that_touch_it(corpus, backups):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    in3 = {bytes(c.Checksum) for c in objs[3].Chunks}
    rows = [{c for _, c, _, _ in restore.packfile_index(p)[1]} for p in packs]
    k = next(i for i, r in enumerate(rows) if 0 < len(r & in3) < len(in3))
    gone = rows[k] - set().union(*(r for i, r in enumerate(rows) if i != k))
    assert gone & in3
    ranges = _ranges(objs)
    contents, statuses, st = snapshot.read_ranges(objs, ranges, packs[:k] + packs[k + 1:], key=KEY)
    want = [_lib.CDC_E_NOTFOUND if _touch(objs, r, gone) else 0 for r in ranges]
    assert statuses == want
    hit3 = [w for r, w in zip(ranges, want) if r[0] == 3]
    assert 0 in hit3 and _lib.CDC_E_NOTFOUND in hit3, "ranges of the same file on both sides"
    for (fi, off, ln), got, w in zip(ranges, contents, want):
        assert got == (None if w else files[fi][off:off + ln])
    assert st["failed_ranges"] == sum(1 for w in want if w)


@pytest.mark.parametrize("key,compression", REPOS[:2], ids=IDS[:2])
@pytest.mark.parametrize("budget", [restore.DEFAULT_BATCH_BYTES, SMALL])
def test_a_damaged_blob_fails_exactly_its_ranges(corpus, backups, key, compression, budget):
    _, files = corpus
    objs, packs = backups(key, compression)
    victim = bytes(objs[4].Chunks[len(objs[4].Chunks) // 2].Checksum)
    bad, hit = [], 0
    for p in packs:
        for _, c, o, n in restore.packfile_index(p)[1]:
            if c == victim:
                b = bytearray(p)
                b[o + n // 2] ^= 0x10
                p = bytes(b)
                hit += 1
        bad.append(p)
    assert hit == 1
    ranges = _ranges(objs)
    contents, statuses, _ = snapshot.read_ranges(objs, ranges, bad, key=key, compression=compression,
                                                 batch_bytes=budget)
    want = [_lib.CDC_E_AUTH if _touch(objs, r, {victim}) else 0 for r in ranges]
    assert statuses == want and 5 < sum(1 for w in want if w) < len(want) // 2
    for (fi, off, ln), got, w in zip(ranges, contents, want):
        assert got == (None if w else files[fi][off:off + ln])


@pytest.mark.parametrize("key,compression", REPOS, ids=IDS)
def test_snapshot_file(corpus, backups, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    with restore.RestoreSession(key=key, compression=compression) as s:
        for p in packs:
            s.add_packfile(p)
        for i in (0, 1, 2, 3, 6):
            calls = {}
            for ra in (0, 4 << 20):
                f = restore.SnapshotFile(s, objs[i], readahead=ra)
                assert f.readable() and f.seekable() and not f.writable() and f.size == len(files[i])
                parts = []
                while True:
                    b = f.read(32768)
                    if not b:
                        break
                    parts.append(b)
                assert b"".join(parts) == files[i], (i, ra)
                assert f.read() == b"" and f.read(10) == b"" and f.tell() == len(files[i])
                calls[ra] = f.device_calls
            n = len(files[i])
            assert calls[0] == -(-n // 32768) and calls[4 << 20] == -(-n // (4 << 20))
        want = files[3]
        f = restore.SnapshotFile(s, objs[3])
        assert f.seek(100_000) == 100_000 and f.read(10) == want[100_000:100_010]
        assert f.seek(-5, io.SEEK_CUR) == 100_005 and f.read(70_000) == want[100_005:170_005]
        assert f.seek(-3, io.SEEK_END) == len(want) - 3 and f.read() == want[-3:]
        assert f.seek(0, io.SEEK_END) == len(want) and f.read(1) == b""
        assert f.seek(0) == 0
        buf = bytearray(1000)
        assert f.readinto(buf) == 1000 and bytes(buf) == want[:1000]
        with pytest.raises(OSError):
            f.seek(len(want) + 1)
        with pytest.raises(OSError):
            f.seek(1, io.SEEK_END)
        with pytest.raises(OSError):
            f.seek(-1)
        assert f.tell() == 1000
        assert io.BufferedReader(restore.SnapshotFile(s, objs[6])).read() == files[6]
        f.close()
        with pytest.raises(ValueError):
            f.read(1)


@pytest.mark.parametrize("how", ["removed", "truncated"])
def test_an_unreadable_packfile_fails_exactly_the_ranges_that_touch_it(corpus, backups, tmp_path, how):
    """Registered by path, then lost before the run: CDC_E_IO for the ranges
    that touch a blob in the lost bytes, every other range's bytes."""
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    paths = pack_loss.write_packs(tmp_path, packs)
    ranges = _ranges(objs)
    with restore.RestoreSession(key=KEY, writers=3) as s:
        for q in paths:
            s.add_packfile(q)
        k = pack_loss.first_home(packs)[bytes(objs[3].Chunks[len(objs[3].Chunks) // 2].Checksum)][0]
        lost = pack_loss.lose(paths, packs, k, how, objs)
        contents, statuses, st = s.read_ranges(objs, ranges)
    want = [_lib.CDC_E_IO if _touch(objs, r, lost) else 0 for r in ranges]
    assert statuses == want and 0 in want and _lib.CDC_E_IO in want
    for (fi, off, ln), got, w in zip(ranges, contents, want):
        assert got == (None if w else files[fi][off:off + ln])
    assert st["failed_ranges"] == sum(1 for w in want if w)


@pytest.mark.parametrize("key,compression", [REPOS[0], REPOS[2]], ids=[IDS[0], IDS[2]])
@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
def test_a_wrong_recorded_length_fails_its_ranges_alone(corpus, backups, key, compression, delta):
    """The first chunk's recorded Length one byte off and a range over that
    whole chunk, so the blob is decoded whole: CDC_E_MISMATCH for that range,
    the ranges of the same batch get their bytes."""
    _, files = corpus
    objs, packs = backups(key, compression)
    chunks = [(bytes(c.Checksum), c.Length) for c in objs[4].Chunks]
    (c0, n0) = chunks[0]
    bad = types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in [(c0, n0 + delta)] + chunks[1:]])
    n = len(objs)
    ranges = [(3, 10, 100_000), (n, 0, n0 + delta + 10), (4, 0, n0 + 10), (n, n0 + delta, 5), (6, 1000, 5)]
    contents, statuses, st = snapshot.read_ranges(list(objs) + [bad], ranges, packs, key=key, compression=compression)
    M = _lib.CDC_E_MISMATCH
    assert statuses == [0, M, 0, 0, 0] and st["failed_ranges"] == 1 and st["batches"] == 1
    assert contents[0] == files[3][10:100_010] and contents[1] is None and contents[2] == files[4][:n0 + 10]
    assert contents[3] == files[4][n0:n0 + 5] and contents[4] == files[6][1000:1005]
