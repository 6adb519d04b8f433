"""The restore path on the device: cdc_assemble_device against numpy, and
backup -> restore round trips through cdc_restore_files (snapshot.restore_files):
byte-identical files, each distinct blob decoded once per batch, per-file
failures (a damaged blob, a missing blob, a wrong Length, an unwritable
destination) that leave every other file intact."""
import hashlib
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from datagen import low_entropy, random_bytes  # noqa: E402
from plakar_amd import _lib, restore, snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32, 64))
MIB = 1 << 20
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, MIB + 3, 4 * MIB]


# ---------------------------------------------------------------- cdc_assemble_device
def _sentinel(n):
    return np.resize(((np.arange(256) * 7 + 3) & 0xFF).astype(np.uint8), n)


def _layout(rng, specs, src_size):
    """Segments for (length, source residue, destination residue) specs: sources
    anywhere in the source buffer (they repeat and overlap), destinations in
    order with small gaps, 64 bytes clear before the first."""
    segs, d = [], 64
    for n, sr, dr in specs:
        so = int(rng.integers(0, (src_size - n - 16) // 16)) * 16 + sr
        d += int(rng.integers(0, 3)) * 16
        d += (dr - d) % 16
        segs.append((so, n, d))
        d += n
    return segs, d + 64


def _run_assemble(src_np, segs, dst_size, dst_shift=0):
    """Run the kernel into a sentinel-filled destination (the tensor starts
    dst_shift bytes into its allocation) and compare the whole destination,
    gaps and margins included, with numpy's copy."""
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(src_np).to(dev)
    want = _sentinel(dst_size)
    whole = torch.from_numpy(np.concatenate([np.zeros(dst_shift, np.uint8), want])).to(dev)
    dst = whole[dst_shift:]
    for so, n, do in segs:
        want[do:do + n] = src_np[so:so + n]
    restore.assemble_device(src, segs, dst)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} (of {dst_size})")


@pytest.fixture(scope="module")
def src_np():
    return random_bytes(6 * MIB, 77)


def test_assemble_small_lengths_every_residue_pair(src_np):
    rng = np.random.default_rng(1)
    specs = [(n, sr, dr) for n in LENGTHS if n <= 65537 for sr in range(16) for dr in range(16)]
    order = rng.permutation(len(specs))
    segs, size = _layout(rng, [specs[i] for i in order], src_np.size)
    _run_assemble(src_np, segs, size)


@pytest.mark.parametrize("dst_shift", [0, 5])
def test_assemble_large_lengths_every_residue(src_np, dst_shift):
    rng = np.random.default_rng(2 + dst_shift)
    specs = [(n, r, (5 * r + 3 + k) % 16) for k, n in enumerate((MIB + 3, 4 * MIB)) for r in range(16)]
    specs += [(n, int(rng.integers(0, 16)), int(rng.integers(0, 16))) for n in LENGTHS]
    segs, size = _layout(rng, [specs[i] for i in rng.permutation(len(specs))], src_np.size)
    _run_assemble(src_np, segs, size, dst_shift)


def test_assemble_one_large_segment_beside_500_tiny_ones(src_np):
    rng = np.random.default_rng(3)
    specs = [(int(rng.integers(1, 200)), int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in range(500)]
    specs.insert(250, (4 * MIB, 7, 9))
    segs, size = _layout(rng, specs, src_np.size)
    _run_assemble(src_np, segs, size)


def test_assemble_one_source_to_many_places(src_np):
    """The deduplicated case: one 1-MiB source copied to 20 places, and
    sources that overlap each other by half."""
    segs, d = [], 64
    for i in range(20):
        segs.append((12345, MIB, d))
        d += MIB + (i % 3)
    for i in range(20):
        segs.append((100 + i * 32768, 65536, d))
        d += 65536 + 1
    _run_assemble(src_np, segs, d + 64)


def test_assemble_single_empty_segment_and_no_segments(src_np):
    _run_assemble(src_np, [(5, 0, 100)], 256)
    _run_assemble(src_np, [], 256)


@pytest.mark.parametrize("policy", [0, 1, 3])
def test_assemble_cache_policies_write_the_same_bytes(src_np, policy):
    rng = np.random.default_rng(4)
    specs = [(n, int(rng.integers(0, 16)), int(rng.integers(0, 16))) for n in LENGTHS if n <= MIB + 3] * 2
    segs, size = _layout(rng, specs, src_np.size)
    assert _lib.lib().cdc_debug_set_assemble_policy(policy) == 0
    try:
        _run_assemble(src_np, segs, size)
    finally:
        _lib.lib().cdc_debug_set_assemble_policy(2)


def test_assemble_rejects_on_the_host(src_np):
    dev = torch.device("cuda", 0)
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    dst = torch.zeros(4096, dtype=torch.uint8, device=dev)
    for segs in ([(0, 100, 50), (0, 100, 149)], [(0, 10, 500), (0, 10, 100)], [(0, 100, 4000)], [(4000, 100, 0)]):
        with pytest.raises(_lib.CdcError) as e:
            restore.assemble_device(src, segs, dst)
        assert e.value.status == _lib.CDC_E_INVALID
    with pytest.raises(_lib.CdcError):
        restore.assemble_device(src, [(0, 100, 0)], src)  # the two buffers alias
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0


# ---------------------------------------------------------------- round trips
def _write(d, files):
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i:02d}"
        p.write_bytes(b)
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    files = [b"", random_bytes(1, 1).tobytes(), random_bytes(1000, 2).tobytes(),
             random_bytes(65535, 3).tobytes(), random_bytes(65536, 4).tobytes(), random_bytes(70_000, 5).tobytes(),
             random_bytes(3 << 20, 6).tobytes(), low_entropy(6 << 20, 7).tobytes(), random_bytes(13 << 20, 8).tobytes()]
    files.append(files[6])        # a duplicate file
    files.append(b"")             # a second empty file
    files.append(files[8][:5 << 20] + random_bytes(1 << 20, 9).tobytes())  # shares a prefix
    return _write(tmp_path_factory.mktemp("restore"), files), files


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
    """restore_plan.h's batching rule restated: per batch, (output bytes, the
    set of distinct (checksum, length), chunk occurrences)."""
    batches, out, seen, segs = [], 0, set(), 0
    for o in objects:
        for c in o.Chunks:
            if out and out + c.Length > budget:
                batches.append((out, seen, segs))
                out, seen, segs = 0, set(), 0
            seen.add((bytes(c.Checksum), c.Length))
            out += c.Length
            segs += 1
    if out or segs or objects:
        batches.append((out, seen, segs))
    return batches


@pytest.mark.parametrize("key,compression", [(KEY, "LZ4"), (None, None), (None, "LZ4")])
def test_backup_then_restore_is_byte_identical(corpus, backups, tmp_path, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    assert len(packs) > 1
    contents, statuses, st = snapshot.restore_files(objs, packs, key=key, compression=compression,
                                                    batch_bytes=8 << 20)
    assert statuses == [0] * len(files)
    for i, (got, want) in enumerate(zip(contents, files)):
        assert got == want, f"file {i}"
    plan = _plan(objs, 8 << 20)
    assert st["batches"] == len(plan) >= 3 and st["distinct_blobs"] < st["segments"]
    assert st["segments"] == sum(len(o.Chunks) for o in objs) and st["bytes"] == sum(len(f) for f in files)
    assert st["distinct_blobs"] == len({bytes(c.Checksum) for o in objs for c in o.Chunks})
    assert st["decoded_blobs"] == sum(len(s) for _, s, _ in plan)  # once per batch it occurs in
    assert st["decoded_bytes"] == sum(n for _, s, _ in plan for _, n in s)
    assert st["files"] == len(files) and st["failed_files"] == 0
    assert st["pieces"] > len(files)  # the 13-MiB file went in pieces
    # and onto disk
    dests = [str(tmp_path / f"out{i:02d}") for i in range(len(files))]
    contents, statuses, st2 = snapshot.restore_files(objs, packs, dests, key=key, compression=compression,
                                                     batch_bytes=8 << 20)
    assert statuses == [0] * len(files) and contents == [None] * len(files)
    for d, want in zip(dests, files):
        assert os.path.getsize(d) == len(want)
        with open(d, "rb") as f:
            assert hashlib.sha256(f.read()).digest() == hashlib.sha256(want).digest()
    assert st2["batches"] == st["batches"]


def test_deduplicated_data_is_decoded_once_per_batch(tmp_path):
    zeros = bytes(24 * MIB)
    paths = _write(tmp_path, [zeros, zeros, zeros])
    objs, packs, _ = snapshot.backup_files(paths, key=KEY, batch_bytes=32 << 20)
    contents, statuses, st = snapshot.restore_files(objs, packs, key=KEY, batch_bytes=16 << 20)
    assert statuses == [0, 0, 0] and all(c == zeros for c in contents)
    plan = _plan(objs, 16 << 20)
    assert st["batches"] == len(plan) >= 2 and st["decoded_blobs"] == sum(len(s) for _, s, _ in plan)
    assert st["distinct_blobs"] <= st["decoded_blobs"] < st["segments"]
    assert st["decoded_bytes"] == sum(n for _, s, _ in plan for _, n in s) < st["bytes"] == 72 * MIB
    assert st["batches"] - st["batches_identity"] >= 1


def test_duplicate_free_files_in_one_batch_skip_the_assemble(tmp_path):
    files = [random_bytes(3 * MIB + 17, 21).tobytes(), random_bytes(100, 22).tobytes(),
             random_bytes(5 * MIB, 23).tobytes()]
    objs, packs, _ = snapshot.backup_files(_write(tmp_path, files), key=None, compression="LZ4")
    contents, statuses, st = snapshot.restore_files(objs, packs, key=None, compression="LZ4")
    assert statuses == [0, 0, 0] and contents == files
    assert st["batches"] == 1 and st["batches_identity"] == 1 and st["distinct_blobs"] == st["segments"]


def test_packfiles_by_path_and_from_memory_and_a_reused_session(corpus, backups, tmp_path):
    _, files = corpus
    objs, packs = backups(KEY, "LZ4")
    pack_paths = []
    for i, p in enumerate(packs):
        q = tmp_path / f"pack{i}"
        q.write_bytes(p)
        pack_paths.append(str(q))
    with restore.RestoreSession(key=KEY, batch_bytes=8 << 20, writers=3) as s:
        for q in pack_paths:
            s.add_packfile(q)
        by_path, st_path, stats_path = s.run(objs)
        again, st_again, stats_again = s.run(list(reversed(objs)))  # the same session, a second run
    from_mem, st_mem, stats_mem = snapshot.restore_files(objs, packs, key=KEY, batch_bytes=8 << 20)
    assert by_path == from_mem == files and st_path == st_mem == [0] * len(files)
    assert again == list(reversed(files)) and st_again == [0] * len(files)
    for k in ("bytes", "segments", "distinct_blobs", "decoded_blobs", "encoded_bytes", "decoded_bytes", "batches"):
        assert stats_path[k] == stats_mem[k], k
    assert stats_again["bytes"] == stats_path["bytes"]
    # a mix: half by path, half from memory
    half = len(packs) // 2
    mixed, st_mixed, _ = snapshot.restore_files(objs, pack_paths[:half] + packs[half:], key=KEY)
    assert mixed == files and st_mixed == [0] * len(files)


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
def test_a_damaged_blob_fails_exactly_its_files(corpus, backups, tmp_path, key, compression, status):
    _, files = corpus
    objs, packs = backups(key, compression)
    in11 = {bytes(c.Checksum) for c in objs[11].Chunks}
    shared = [bytes(c.Checksum) for c in objs[8].Chunks if bytes(c.Checksum) in in11]
    victim = shared[len(shared) // 2]  # in the 5-MiB prefix that files 8 and 11 share
    users =[i for i, o in enumerate(objs) if any(bytes(c.Checksum) == victim for c in o.Chunks)]
    assert users == [8, 11]
    bad_packs = _damage(packs, victim)
    dests = [str(tmp_path / f"out{i:02d}") for i in range(len(files))]
    _, statuses, st = snapshot.restore_files(objs, bad_packs, dests, key=key, compression=compression,
                                             batch_bytes=8 << 20)
    assert statuses == [status if i in users else 0 for i in range(len(files))]
    assert st["failed_files"] == 2
    for i, (d, want) in enumerate(zip(dests, files)):
        if i in users:
            assert not os.path.exists(d), f"failed file {i} was left on disk"
        else:
            with open(d, "rb") as f:
                assert f.read() == want, f"file {i}"
    contents, statuses, _ = snapshot.restore_files(objs, bad_packs, key=key, compression=compression,
                                                   batch_bytes=8 << 20)
    assert [c is None for c in contents] == [i in users for i in range(len(files))]
    assert all(c == files[i] for i, c in enumerate(contents) if c is not None)
    if key is None and compression is None:
        # without verify nothing notices: the flipped bit is restored.  That is what verify is for.
        contents, statuses, _ = snapshot.restore_files(objs, bad_packs, key=None, compression=None, verify=False,
                                                       batch_bytes=8 << 20)
        assert statuses == [0] * len(files)
        for i, (got, want) in enumerate(zip(contents, files)):
            if i in users:
                diff = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
                assert len(got) == len(want) and diff.size == 1 and (got[diff[0]] ^ want[diff[0]]) == 0x10
            else:
                assert got == want


def _obj(chunks):
    return types.SimpleNamespace(Chunks=[types.SimpleNamespace(Checksum=c, Length=n) for c, n in chunks])


@pytest.mark.parametrize("key,compression", [(KEY, "LZ4"), (None, None)])
def test_a_missing_blob_and_a_wrong_length_fail_their_file_alone(corpus, backups, tmp_path, key, compression):
    _, files = corpus
    objs, packs = backups(key, compression)
    chunks6 = [(bytes(c.Checksum), c.Length) for c in objs[6].Chunks]
    missing = _obj(chunks6[:1] + [(hashlib.sha256(b"in no packfile").digest(), 1234)])
    (c0, n0) = chunks6[0]
    longer, shorter = _obj([(c0, n0 + 1)] + chunks6[1:]), _obj([(c0, n0 - 1)] + chunks6[1:])
    todo = list(objs) + [missing, longer, shorter]
    dests = [str(tmp_path / f"out{i:02d}") for i in range(len(todo))]
    contents, statuses, st = snapshot.restore_files(todo, packs, key=key, compression=compression,
                                                    batch_bytes=8 << 20)
    n = len(files)
    assert statuses[:n] == [0] * n and contents[:n] == files
    assert statuses[n:] == [_lib.CDC_E_NOTFOUND, _lib.CDC_E_MISMATCH, _lib.CDC_E_MISMATCH]
    assert contents[n:] == [None, None, None] and st["failed_files"] == 3
    _, statuses, _ = snapshot.restore_files(todo, packs, dests, key=key, compression=compression,
                                            batch_bytes=8 << 20)
    assert statuses[n:] == [_lib.CDC_E_NOTFOUND, _lib.CDC_E_MISMATCH, _lib.CDC_E_MISMATCH]
    assert [os.path.exists(d) for d in dests] == [True] * n + [False] * 3


def test_an_unwritable_destination_fails_that_file_alone(corpus, backups, tmp_path):
    _, files = corpus
    objs, packs = backups(None, "LZ4")
    dests = [str(tmp_path / f"out{i:02d}") for i in range(len(files))]
    dests[5] = str(tmp_path / "no" / "such" / "dir" / "f")
    dests[8] = str(tmp_path / "nor" / "this")  # the file that goes in pieces
    _, statuses, st = snapshot.restore_files(objs, packs, dests, key=None, compression="LZ4", batch_bytes=8 << 20)
    assert statuses == [_lib.CDC_E_IO if i in (5, 8) else 0 for i in range(len(files))]
    assert st["failed_files"] == 2
    for i, (d, want) in enumerate(zip(dests, files)):
        if i not in (5, 8):
            with open(d, "rb") as f:
                assert f.read() == want


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restore_random_corpora(tmp_path, seed):
    rng = np.random.default_rng(np.random.PCG64(7700 + seed))
    files = []
    for i in range(int(rng.integers(10, 21))):
        r = rng.random()
        if files and r < 0.15:
            files.append(files[int(rng.integers(0, len(files)))])  # a planted duplicate
        elif files and r < 0.3:
            f = files[int(rng.integers(0, len(files)))]
            files.append(f[:len(f) // 2] + random_bytes(int(rng.integers(1, MIB)), 7800 + 64 * seed + i).tobytes())
        else:
            n = 0 if r < 0.4 else int(np.exp(rng.uniform(0, np.log(6 * MIB))))
            gen = random_bytes if rng.random() < 0.7 else (lambda k, s: low_entropy(k, s, 0.01))
            files.append(gen(n, 7900 + 64 * seed + i).tobytes())
    key, compression = [(KEY, "LZ4"), (None, None), (None, "LZ4")][seed % 3]
    (tmp_path / "in").mkdir()
    objs, packs, _ = snapshot.backup_files(_write(tmp_path / "in", files), key=key, compression=compression,
                                           max_size=int(rng.choice([1 << 20, 4 << 20])), batch_bytes=8 << 20)
    batch = int(rng.choice([2 << 20, 5 << 20, 64 << 20]))
    what = f"seed {seed}: batch {batch} sizes {[len(f) for f in files]}"
    contents, statuses, st = snapshot.restore_files(objs, packs, key=key, compression=compression,
                                                    batch_bytes=batch, writers=int(rng.integers(1, 9)))
    assert statuses == [0] * len(files), what
    for i, (got, want) in enumerate(zip(contents, files)):
        assert got == want, f"{what}: file {i}"
    plan = _plan(objs, batch)
    assert st["batches"] == len(plan) and st["decoded_blobs"] == sum(len(s) for _, s, _ in plan), what
    dests = [str(tmp_path / f"out{i:02d}") for i in range(len(files))]
    _, statuses, _ = snapshot.restore_files(objs, packs, dests, key=key, compression=compression, batch_bytes=batch)
    assert statuses == [0] * len(files), what
    for d, want in zip(dests, files):
        with open(d, "rb") as f:
            assert f.read() == want, what
