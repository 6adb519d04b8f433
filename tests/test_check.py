"""Check on the device: k_object_digest through check.object_digests_device
against hashlib over the bytes put together in Python (bit-exact, every case),
and backup -> check runs through cdc_check_files (snapshot.check_files):
verdicts, computed object checksums, the device/host split and the counters."""
import ctypes
import hashlib
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pack_loss  # noqa: E402
from datagen import low_entropy, random_bytes  # noqa: E402
from plakar_amd import _lib, check, restore, snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32, 64))
MIB = 1 << 20
SRC_LEN = 3 * MIB + 5  # odd
TOTALS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 4095, 4096, 4097, 65535, 65536, 65537, MIB + 3]
U64_MAX = 2 ** 64 - 1


# ---------------------------------------------------------------- k_object_digest
@pytest.fixture(scope="module")
def src():
    a = random_bytes(SRC_LEN, 91)
    return a, torch.from_numpy(a).to(torch.device("cuda", 0))


def _want(a, segs):
    return hashlib.sha256(b"".join(a[o:o + n].tobytes() for o, n in segs)).digest()


def _run(src, objects):
    a, t = src
    got = check.object_digests_device(t, objects).cpu().numpy()
    assert got.shape == (len(objects), 32)
    bad = [i for i, segs in enumerate(objects) if got[i].tobytes() != _want(a, segs)]
    assert not bad, f"{len(bad)} of {len(objects)} digests differ, first object {bad[0]}: {objects[bad[0]][:6]}"


def test_one_segment_objects_every_total_and_residue(src):
    """Padding in one block and in two, the funnel shift at every source
    residue and the clamped last dword; a segment from offset 0 and one that
    ends on the buffer's last byte per total.  One object per lane: no queue."""
    rng = np.random.default_rng(1)
    objects = []
    for t in TOTALS:
        for r in range(4):
            objects.append([(4 * int(rng.integers(0, (SRC_LEN - t - 8) // 4)) + r, t)])
        objects.append([(0, t)])
        objects.append([(SRC_LEN - t, t)])
    _run(src, objects)


def test_two_segment_objects_every_seam_phase(src):
    """A first segment of every length 0..130 before one of 200 bytes, at all
    16 pairs of source residues: every seam phase on both sides of the first
    two block boundaries.  2,096 objects: one per lane, no queue."""
    rng = np.random.default_rng(2)
    objects = []
    for a in range(131):
        for r0 in range(4):
            for r1 in range(4):
                objects.append([(4 * int(rng.integers(0, 700000)) + r0, a), (4 * int(rng.integers(0, 700000)) + r1, 200)])
    _run(src, objects)


def test_several_boundaries_in_one_block(src):
    """Three- and four-segment objects whose first segments sum to less than
    64 bytes: several seam parts land in one block.  No queue."""
    rng = np.random.default_rng(3)
    lens = [0, 1, 5, 7, 31, 32]
    at = lambda n: (int(rng.integers(0, SRC_LEN - n)), n)  # noqa: E731
    objects = []
    for a in lens:
        for b in lens:
            if a + b < 64:
                objects.append([at(a), at(b), at(150)])
                objects.append([at(a), at(b), at(3)])
            for c in lens:
                if a + b + c < 64:
                    objects.append([at(a), at(b), at(c), at(150)])
                    objects.append([at(a), at(b), at(c), at(0)])
    _run(src, objects)


def test_seams_everywhere_and_nowhere(src):
    """500 segments of 1-200 bytes; segments of 63 bytes only (every block a
    seam); multiples of 64 only (no block a seam).  No queue."""
    rng = np.random.default_rng(4)
    tiny = [(int(rng.integers(0, SRC_LEN - 200)), int(rng.integers(1, 201))) for _ in range(500)]
    all63 = [(int(rng.integers(0, SRC_LEN - 63)), 63) for _ in range(300)]
    all64 = [(int(rng.integers(0, SRC_LEN - 512)), 64 * int(rng.integers(1, 9))) for _ in range(100)]
    _run(src, [tiny, all63, all64])


def test_shared_and_overlapping_sources(src):
    """One 1-MiB segment in 20 objects, and segments that overlap by half.  No queue."""
    objects = [[(12345, MIB)]] + [[(12345, MIB), (7 * i, i)] for i in range(1, 20)]
    objects.append([(100 + i * 32768, 65536) for i in range(20)])
    _run(src, objects)


def test_empty_objects(src):
    """No segments, empty segments only (one of them at the buffer's end), an
    empty list of objects and an empty source: SHA-256("") from one padding
    block.  No queue."""
    a, t = src
    objects = [[], [(5, 0)], [(0, 0), (SRC_LEN, 0), (77, 0)], [(3, 1)], []]
    _run(src, objects)
    got = check.object_digests_device(t, objects).cpu().numpy()
    assert got[0].tobytes() == got[2].tobytes() == hashlib.sha256(b"").digest()
    assert check.object_digests_device(t, []).shape == (0, 32)
    empty = torch.zeros(0, dtype=torch.uint8, device=t.device)
    assert check.object_digests_device(empty, [[], [(0, 0)]]).cpu().numpy()[1].tobytes() == hashlib.sha256(b"").digest()


@pytest.mark.parametrize("lanes", [1, 128, 700])
def test_object_queue_order(src, lanes):
    """1,500 objects of 0-40,000 bytes in 1-4 segments with fewer lanes than
    objects (test_gpu_digest_queue_order's shape).  lanes 1 and 128: one
    workgroup takes all 1,500, more than kSortCap, so the queue hands them out
    in list order; lanes 700: three objects per lane, four workgroups of at
    most 384 objects each, sorted longest first by the bitonic network."""
    rng = np.random.default_rng(5)
    objects = []
    for _ in range(1500):
        total = int(rng.integers(0, 40001)) if rng.random() < 0.9 else 0
        k = int(rng.integers(1, 5))
        cuts = sorted(int(x) for x in rng.integers(0, total + 1, size=k - 1))
        parts = [b - a for a, b in zip([0] + cuts, cuts + [total])]
        objects.append([(int(rng.integers(0, SRC_LEN - n)), n) for n in parts])
    L = _lib.lib()
    try:
        assert L.cdc_debug_set_digest_lanes(lanes) == 0
        _run(src, objects)
    finally:
        L.cdc_debug_set_digest_lanes(0)


def test_object_digests_rejects_on_the_host(src):
    a, t = src
    sentinel = torch.full((2, 32), 0xA7, dtype=torch.uint8, device=t.device)
    p64 = ctypes.POINTER(ctypes.c_uint64)

    def call(off, ln, seg0, n=2, data=True, dig=True):
        arr = [np.asarray(x, dtype=np.uint64) if x is not None else None for x in (off, ln, seg0)]
        ptr = [x.ctypes.data_as(p64) if x is not None else None for x in arr]
        return _lib.lib().cdc_object_digests_device(
            0, ctypes.c_void_p(t.data_ptr()) if data else None, SRC_LEN, ptr[0], ptr[1], len(off) if off is not None else 3,
            ptr[2], n, ctypes.c_void_p(sentinel.data_ptr()) if dig else None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    good = ([0, 100, SRC_LEN - 96], [100, 50, 96], [0, 2, 3])
    for off, ln, seg0 in ([good[0], [100, 50, 97], good[2]],            # one byte past the end
                          [[0, SRC_LEN + 1, 5], good[1], good[2]],      # an offset past the end
                          [good[0], [100, 2 ** 64 - 50, 96], good[2]],  # offset + length wraps
                          [good[0], good[1], [0, 2, 2]],                # does not reach nsegs
                          [good[0], good[1], [0, 2, 4]],                # passes nsegs
                          [good[0], good[1], [2, 1, 3]],                # descends
                          [None, good[1], good[2]], [good[0], None, good[2]], [good[0], good[1], None]):
        assert call(off, ln, seg0) == _lib.CDC_E_INVALID, (off, ln, seg0)
    assert call(*good, data=False) == _lib.CDC_E_INVALID
    assert call(*good, dig=False) == _lib.CDC_E_INVALID
    with pytest.raises(_lib.CdcError) as e:
        check.object_digests_device(t, [[(SRC_LEN, 1)]])
    assert e.value.status == _lib.CDC_E_INVALID
    torch.cuda.synchronize()
    assert bool((sentinel == 0xA7).all())
    assert call(*good) == 0  # and the good lists do run
    assert sentinel.cpu().numpy()[0].tobytes() == _want(a, [(0, 100), (100, 50)])


# ---------------------------------------------------------------- the pipeline
def _write(d, files):
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i:02d}"
        p.write_bytes(b)
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """test_restore.py's corpus."""
    files = [b"", random_bytes(1, 1).tobytes(), random_bytes(1000, 2).tobytes(),
             random_bytes(65535, 3).tobytes(), random_bytes(65536, 4).tobytes(), random_bytes(70_000, 5).tobytes(),
             random_bytes(3 << 20, 6).tobytes(), low_entropy(6 << 20, 7).tobytes(), random_bytes(13 << 20, 8).tobytes()]
    files.append(files[6])        # a duplicate file
    files.append(b"")             # a second empty file
    files.append(files[8][:5 << 20] + random_bytes(1 << 20, 9).tobytes())  # shares a prefix
    return _write(tmp_path_factory.mktemp("check"), files), files


@pytest.fixture(scope="module")
def backups(corpus):
    """backup_files of the corpus per (key, compression), made once."""
    paths, _ = corpus
    made = {}

    def get(key, compression):
        if (key, compression) not in made:
            objs, packs, _ = snapshot.backup_files(paths, key=key, compression=compression, max_size=2 << 20,
                                                   batch_bytes=8 << 20, timestamp=11)
            made[(key, compression)] = (objs, packs)
        return made[(key, compression)]
    return get


def _plan(objects, budget):
    """restore_plan.h's batching rule restated: per batch (file bytes, the set
    of distinct (checksum, length), chunk occurrences), and the files that
    have chunks in more than one batch."""
    batches, out, seen, segs, spans = [], 0, set(), 0, set()
    for i, o in enumerate(objects):
        inb = set()
        for c in o.Chunks:
            if out and out + c.Length > budget:
                batches.append((out, seen, segs))
                out, seen, segs = 0, set(), 0
            seen.add((bytes(c.Checksum), c.Length))
            out += c.Length
            segs += 1
            inb.add(len(batches))
        if len(inb) > 1:
            spans.add(i)
    if out or segs or objects:
        batches.append((out, seen, segs))
    return batches, spans


def _sha(b):
    return hashlib.sha256(b).digest()


CODECS = [(KEY, "LZ4"), (None, None), (KEY, "GZIP")]


@pytest.mark.parametrize("key,compression", CODECS)
def test_intact_snapshot_checks_ok_on_every_split(corpus, backups, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    assert len(packs) > 1
    plan, spans = _plan(objs, 8 << 20)
    assert 8 in spans  # the 13-MiB file cannot fit a batch of 8 MiB
    runs = {}
    for hml in (0, 1, U64_MAX):
        res, st = snapshot.check_files(objs, packs, key=key, compression=compression, batch_bytes=8 << 20,
                                       host_min_len=hml)
        runs[hml] = (res, st)
        for i, (r, f, o) in enumerate(zip(res, files, objs)):
            assert r["status"] == 0 and r["bad_chunk"] == -1 and r["size"] == len(f), (hml, i, r)
            assert r["checksum"] == _sha(f) == bytes(o.Checksum), (hml, i)
            assert r["hashed"] == 2 if i in spans else r["hashed"] in (1, 2), (hml, i)
        assert st["batches"] == len(plan) >= 3 and st["distinct_blobs"] < st["segments"]
        assert st["segments"] == sum(len(o.Chunks) for o in objs) and st["bytes"] == sum(len(f) for f in files)
        assert st["distinct_blobs"] == len({bytes(c.Checksum) for o in objs for c in o.Chunks})
        assert st["decoded_blobs"] == sum(len(s) for _, s, _ in plan)  # once per batch it occurs in
        assert st["decoded_bytes"] == sum(n for _, s, _ in plan for _, n in s)
        assert st["files"] == len(files) and st["failed_files"] == 0
        assert st["pieces"] > len(files)
        assert st["device_bytes"] + st["host_bytes"] == st["bytes"]
        assert st["device_objects"] == sum(r["hashed"] == 1 for r in res)
        assert st["host_objects"] == sum(r["hashed"] == 2 for r in res)
        assert st["host_bytes"] == sum(r["size"] for r in res if r["hashed"] == 2)
    res, st = runs[1]    # everything on the host
    assert st["device_objects"] == 0 and st["seam_bytes"] == 0 and all(r["hashed"] == 2 for r in res)
    res, st = runs[U64_MAX]  # only the files that span batches on the host
    for i, (r, f) in enumerate(zip(res, files)):
        if f:
            assert r["hashed"] == (2 if i in spans else 1), i
    assert st["device_objects"] >= len([f for i, f in enumerate(files) if f and i not in spans])
    assert st["seam_bytes"] <= 64 * st["segments"]  # at most one block per chunk boundary


def _damage(packs, checksum):
    """The packfiles with one bit flipped in the middle of that chunk's blob."""
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


@pytest.mark.parametrize("key,compression,status", [(KEY, "LZ4", _lib.CDC_E_AUTH), (None, None, _lib.CDC_E_MISMATCH)])
def test_a_damaged_blob_fails_exactly_its_files(corpus, backups, key, compression, status):
    _, files = corpus
    objs, packs = backups(key, compression)
    in11 = {bytes(c.Checksum) for c in objs[11].Chunks}
    shared = [bytes(c.Checksum) for c in objs[8].Chunks if bytes(c.Checksum) in in11]
    victim = shared[len(shared) // 2]  # in the 5-MiB prefix that files 8 and 11 share
    users = [i for i, o in enumerate(objs) if any(bytes(c.Checksum) == victim for c in o.Chunks)]
    assert users == [8, 11]
    bad_packs = _damage(packs, victim)
    for hml in (0, 1):
        res, st = snapshot.check_files(objs, bad_packs, key=key, compression=compression, batch_bytes=8 << 20,
                                       host_min_len=hml)
        assert st["failed_files"] == 2
        for i, (r, f, o) in enumerate(zip(res, files, objs)):
            if i in users:
                idx = [bytes(c.Checksum) for c in o.Chunks].index(victim)
                assert (r["status"], r["bad_chunk"], r["hashed"], r["checksum"]) == (status, idx, 0, None), (i, r)
            else:
                assert r["status"] == 0 and r["bad_chunk"] == -1 and r["checksum"] == _sha(f), (i, r)


def _obj(chunks, checksum=bytes(32)):
    return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in chunks],
                                 Checksum=checksum)


def _bad_objects(objs):
    chunks6 = [(bytes(c.Checksum), c.Length) for c in objs[6].Chunks]
    missing = _obj(chunks6[:1] + [(_sha(b"in no packfile"), 1234)] + chunks6[1:])
    (c0, n0) = chunks6[0]
    return [missing, _obj([(c0, n0 + 1)] + chunks6[1:]), _obj([(c0, n0 - 1)] + chunks6[1:])]


@pytest.mark.parametrize("key,compression", [(KEY, "LZ4"), (None, None)])
def test_a_missing_chunk_and_a_wrong_length_fail_their_file_alone(corpus, backups, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    todo = list(objs) + _bad_objects(objs)
    res, st = snapshot.check_files(todo, packs, key=key, compression=compression, batch_bytes=8 << 20)
    n = len(files)
    for r, f in zip(res[:n], files):
        assert r["status"] == 0 and r["checksum"] == _sha(f)
    assert [(r["status"], r["bad_chunk"], r["hashed"]) for r in res[n:]] == [
        (_lib.CDC_E_NOTFOUND, 1, 0), (_lib.CDC_E_MISMATCH, 0, 0), (_lib.CDC_E_MISMATCH, 0, 0)]
    assert st["failed_files"] == 3 and st["files"] == n + 3


def test_a_permuted_chunk_list_is_a_wrong_object(corpus, backups):
    """All chunks intact, the list reordered, the record's checksum the real
    file's: only the object checksum can tell.  On the device path and on the
    host's."""
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    chunks = [(bytes(c.Checksum), c.Length) for c in objs[6].Chunks]
    assert len(chunks) >= 2
    ends = np.cumsum([n for _, n in chunks])
    parts = [files[6][e - n:e] for e, (_, n) in zip(ends, chunks)]
    assert b"".join(parts) == files[6]
    perm = _obj(chunks[::-1], bytes(objs[6].Checksum))
    want = _sha(b"".join(parts[::-1]))
    assert want != bytes(objs[6].Checksum)
    for hml, where in ((U64_MAX, 1), (1, 2)):
        res, st = snapshot.check_files([objs[6], perm], packs, key=KEY, host_min_len=hml)
        assert (res[0]["status"], res[0]["hashed"], res[0]["checksum"]) == (0, where, _sha(files[6]))
        assert res[1] == dict(status=_lib.CDC_E_MISMATCH, bad_chunk=-1, hashed=where, checksum=want, size=len(files[6]))
        assert st["failed_files"] == 1 and st["decoded_blobs"] == len(set(chunks))
        res, st = snapshot.check_files([perm], packs, key=KEY, host_min_len=hml, verify_checksum=False)
        assert res[0] == dict(status=0, bad_chunk=-1, hashed=where, checksum=want, size=len(files[6]))
        assert st["failed_files"] == 0


def test_deduplicated_files_are_hashed_where_their_one_blob_lies(tmp_path):
    zeros = bytes(3 * MIB)
    objs, packs, _ = snapshot.backup_files(_write(tmp_path, [zeros, zeros, zeros]), key=KEY, max_size=2 << 20)
    res, st = snapshot.check_files(objs, packs, key=KEY, host_min_len=U64_MAX)
    assert [(r["status"], r["hashed"], r["checksum"]) for r in res] == [(0, 1, _sha(zeros))] * 3
    assert st["device_bytes"] == 9 * MIB and st["device_objects"] == 3 and st["host_bytes"] == 0
    assert st["decoded_bytes"] * 3 <= st["device_bytes"]  # each distinct blob decoded once, read in many places
    assert st["seam_bytes"] <= 64 * st["segments"] and st["batches"] == 1


def test_fast_asks_the_locator_only(corpus, backups):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    victim = bytes(objs[6].Chunks[0].Checksum)
    todo = list(objs) + _bad_objects(objs)
    res, st = snapshot.check_files(todo, _damage(packs, victim), key=KEY, fast=True)
    n = len(files)
    assert [(r["status"], r["bad_chunk"]) for r in res] == [(0, -1)] * n + [(_lib.CDC_E_NOTFOUND, 1), (0, -1), (0, -1)]
    assert all(r["hashed"] == 0 and r["checksum"] is None for r in res)
    assert [r["size"] for r in res[:n]] == [len(f) for f in files]
    assert st["decoded_blobs"] == 0 and st["encoded_bytes"] == 0 and st["batches"] == 0
    assert st["files"] == n + 3 and st["failed_files"] == 1


def test_packfiles_by_path_and_from_memory_and_a_reused_session(corpus, backups, tmp_path):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    pack_paths = []
    for i, p in enumerate(packs):
        q = tmp_path / f"pack{i}"
        q.write_bytes(p)
        pack_paths.append(str(q))
    with check.CheckSession(key=KEY, batch_bytes=8 << 20, threads=3) as s:
        for q in pack_paths:
            s.add_packfile(q)
        by_path, stats_path = s.run(objs)
        again, stats_again = s.run(objs)  # the same session, a second run
    from_mem, stats_mem = snapshot.check_files(objs, packs, key=KEY, batch_bytes=8 << 20, threads=3)
    assert by_path == from_mem == again
    assert [r["checksum"] for r in by_path] == [_sha(f) for f in files]
    counters = [k for k in stats_mem if not k.endswith("_s")]
    assert "device_bytes" in counters and "seam_bytes" in counters
    for k in counters:
        assert stats_path[k] == stats_mem[k] == stats_again[k], k


@pytest.mark.parametrize("how", ["removed", "truncated"])
def test_an_unreadable_packfile_fails_exactly_its_files(corpus, backups, tmp_path, how):
    """Registered by path, then lost before the run: CDC_E_IO and the first
    lost chunk for the files with a blob there, every other file checked."""
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    paths = pack_loss.write_packs(tmp_path, packs)
    with check.CheckSession(key=KEY, batch_bytes=8 << 20, threads=3) as s:
        for q in paths:
            s.add_packfile(q)
        lost = pack_loss.lose(paths, packs, pack_loss.pick(objs, packs), how, objs)
        res, st = s.run(objs)
    want = [pack_loss.first_lost(o, lost) for o in objs]
    assert any(w is not None for w in want) and any(w is None and f for w, f in zip(want, files))
    for i, (r, f, w) in enumerate(zip(res, files, want)):
        if w is None:
            assert r["status"] == 0 and r["bad_chunk"] == -1 and r["checksum"] == _sha(f), (i, r)
        else:
            assert (r["status"], r["bad_chunk"], r["hashed"], r["checksum"]) == (_lib.CDC_E_IO, w, 0, None), (i, r)
    assert st["failed_files"] == sum(w is not None for w in want)
