"""The native sync pipeline (cdc_sync_* behind sync.SyncPipeline) end to end:
packfiles of one repository in, packfiles of another out, compared with
sync.SyncSession's loop, read back with restore_files and with libcrypto."""
import collections
import ctypes
import hashlib

import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref as dr  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, decode, packer, restore, snapshot, sync  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402
from plakar_amd.sync import SyncPipeline, sync_packfiles  # noqa: E402 - the native pipeline under test

pytestmark = pytest.mark.gpu

KEY_A = bytes(range(32, 64))
KEY_B = bytes(range(200, 232))
A_LZ4 = dict(src_key=KEY_A, src_compression="LZ4")


def _small_chunks():
    # chunks of 4 to 64 KiB: about 2 MiB is over a hundred blobs, so a batch budget
    # of 256 KiB makes eight batches and more
    return Repository(Configuration("FASTCDC", 4096, 16384, 65536))


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    """Three files like tests/test_sync.py's (empty, about 100 KiB, about
    2.5 MiB with a repeated region: 2.4 MB of distinct bytes) backed up under
    key A / LZ4 in small chunks, into several packfiles."""
    d = tmp_path_factory.mktemp("syncpipe")
    region = random_bytes(300_000, 21).tobytes()
    files = [b"", random_bytes(100_003, 20).tobytes(),
             region + random_bytes(1_000_000, 22).tobytes() + region + random_bytes(1_000_001, 23).tobytes()]
    paths = []
    for i, b in enumerate(files):
        p = d / f"f{i}"
        p.write_bytes(b)
        paths.append(str(p))
    objs, packs, _ = snapshot.backup_files(paths, repo=_small_chunks(), key=KEY_A, compression="LZ4",
                                           max_size=512 << 10, batch_bytes=8 << 20, packers=1, timestamp=11)
    assert len(packs) >= 3 and sum(len(_index(p)) for p in packs) >= 64
    return files, objs, packs


def _index(p):
    return restore.packfile_index(p)[1]


def _rows(packs):
    out = []
    for p in packs:
        out += [(t, c, p[o:o + n]) for t, c, o, n in _index(p)]
    return out


def _keys(packs):
    return [(t, c) for t, c, _ in _rows(packs)]


def _native(packs, wanted=None, **kw):
    kw.setdefault("timestamp", 12)
    kw.setdefault("packers", 1)
    return sync_packfiles(packs, wanted=wanted, **kw)


def _session(packs, wanted=None, **kw):
    kw.setdefault("timestamp", 12)
    s = sync.SyncSession(**kw)
    for p in packs:
        s.add_packfile(p)
    return s.run(wanted)


@pytest.fixture(scope="module")
def plain_lz4(source):
    """The source opened: the same blobs in a repository without a key (the
    source of the copy and seal paths)."""
    _, _, packs = source
    out, failures, stats = _native(packs, **A_LZ4)
    assert failures == {} and stats["path"] == "open"
    return out


# ---- 1. the five paths --------------------------------------------------------------
@pytest.mark.parametrize("path,src,dst", [
    ("rekey", (KEY_A, "LZ4"), (KEY_B, "LZ4")),
    ("open", (KEY_A, "LZ4"), (None, "LZ4")),
    ("reencode", (KEY_A, "LZ4"), (KEY_B, "GZIP")),
    ("copy", (None, "LZ4"), (None, "LZ4")),
    ("seal", (None, "LZ4"), (KEY_B, "LZ4")),
])
def test_every_path_round_trips(source, plain_lz4, path, src, dst):
    files, objs, packs = source
    inp = packs if src[0] is not None else plain_lz4
    out, failures, stats = _native(inp, src_key=src[0], src_compression=src[1], dst_key=dst[0], dst_compression=dst[1])
    assert failures == {} and stats["path"] == path and stats["failed"] == 0 and stats["skipped"] == 0
    assert _keys(out) == _keys(inp) and stats["blobs"] == len(_keys(inp))
    assert stats["bytes_in"] == sum(len(b) for _, _, b in _rows(inp))
    assert stats["bytes_out"] == sum(len(b) for _, _, b in _rows(out))
    assert stats["packfiles"] == len(out) >= 1 and stats["packed_bytes"] == sum(len(p) for p in out)
    assert stats["batches"] == 1 and stats["wall_s"] > 0
    contents, statuses, _ = snapshot.restore_files(objs, out, key=dst[0], compression=dst[1], verify=True)
    assert statuses == [0] * len(files) and contents == files
    if path == "rekey":  # only the envelope changed: the frame under B is the frame under A
        assert stats["bytes_in"] == stats["bytes_out"]
        for (_, c, a), (_, _, b) in zip(_rows(inp), _rows(out)):
            frame = crypto_ref.decrypt_stream(KEY_A, a)[0]
            assert crypto_ref.decrypt_stream(KEY_B, b)[0] == frame and a != b
            assert hashlib.sha256(crypto_ref.decode(a, KEY_A, True)).digest() == c


# ---- 2. equality with SyncSession ---------------------------------------------------
SHAPES = {
    "flush_inside_a_batch": dict(max_size=256 << 10, batch_bytes=1 << 20),
    "packfile_spans_batches": dict(max_size=1 << 20, batch_bytes=256 << 10),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("path,dst", [("rekey", (KEY_B, "LZ4")), ("open", (None, "LZ4")), ("reencode", (None, "GZIP"))])
def test_packers_1_equals_the_python_loop(source, shape, path, dst):
    _, _, packs = source
    kw = dict(A_LZ4, dst_key=dst[0], dst_compression=dst[1], **SHAPES[shape])
    want, wf, ws = _session(packs, **kw)
    got, gf, gs = _native(packs, **kw)
    assert wf == gf == {} and gs["path"] == ws["path"] == path
    for name in ("blobs", "skipped", "failed", "bytes_in", "bytes_out", "batches", "packfiles"):
        assert gs[name] == ws[name], name
    assert len(got) == len(want) > 1
    assert [_index(p) for p in got] == [_index(p) for p in want]  # boundaries, and every row's type, checksum, offset, length
    assert [restore.packfile_index(p)[0]["timestamp"] for p in got] == [12] * len(got)
    if shape == "packfile_spans_batches":
        assert gs["batches"] >= 8 and gs["packfiles"] < gs["batches"]  # the slots rotate more than once
    else:
        assert gs["packfiles"] > gs["batches"] > 1
    if dst[0] is None:  # nothing random in the output: the same bytes
        assert got == want


# ---- 3. a small budget ----------------------------------------------------------------
def test_blobs_above_the_budget_go_alone(source):
    files, objs, packs = source
    big = dr.rnd(100_000, 77)  # one blob that is larger than the budget whatever the chunker cut
    pk = packer.Packer(timestamp=5)
    pk.AddBlob(1, hashlib.sha256(big).digest(), dr.seal_stream(KEY_A, dr.lz4f_compress(big), 78))
    extra = pk.Serialize()
    pk.close()
    inp = [packs[0], extra] + packs[1:]
    budget = 64 << 10
    lens = [len(b) for _, _, b in _rows(inp)]
    assert max(lens) > budget
    # the cut restated: a batch closes before the row that would take it past the budget
    batches, size = 0, 0
    for n in lens:
        if batches == 0 or size + n > budget:
            batches, size = batches + 1, 0
        size += n
    out, failures, stats = _native(inp, dst_key=KEY_B, batch_bytes=budget, **A_LZ4)
    assert failures == {} and stats["batches"] == batches and stats["blobs"] == len(lens)
    assert _keys(out) == _keys(inp)  # nothing lost, nothing twice, in order
    plains = decode.decode_blobs([b for _, _, b in _rows(out)], key=KEY_B, compressed="LZ4")
    assert [hashlib.sha256(p).digest() for p in plains] == [c for _, c in _keys(inp)]
    contents, statuses, _ = snapshot.restore_files(objs, out, key=KEY_B, compression="LZ4", verify=True)
    assert statuses == [0] * len(files) and contents == files


# ---- 4. several packers -----------------------------------------------------------------
def test_three_packers_keep_source_order_inside_each_packfile(source):
    _, _, packs = source
    kw = dict(A_LZ4, dst_key=None, dst_compression="LZ4", max_size=256 << 10, batch_bytes=512 << 10)
    one, _, s1 = _native(packs, packers=1, **kw)
    three, failures, s3 = _native(packs, packers=3, **kw)
    assert failures == {} and s3["blobs"] == s1["blobs"] and s3["bytes_out"] == s1["bytes_out"]
    multiset = lambda ps: collections.Counter((t, c, len(b)) for t, c, b in _rows(ps))  # noqa: E731
    assert multiset(three) == multiset(one)
    assert collections.Counter(_rows(three)) == collections.Counter(_rows(one))  # no key: the same blobs byte for byte
    order = {k: i for i, k in enumerate(_keys(packs))}
    for p in three:
        footer, rows = restore.packfile_index(p)
        assert footer["count"] == len(rows) >= 1
        at = [order[(t, c)] for t, c, _, _ in rows]
        assert at == sorted(at)
    assert s3["packfiles"] == len(three)


# ---- 5. every blob type, a duplicate registration, a damaged row ---------------------------
def _typed_packfile():
    """tests/test_sync.py's recipe: blobs of types 1 to 5 under key A / LZ4, one
    checksum under two types, and one row whose bytes are damaged."""
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


def test_every_blob_type_is_carried_and_a_failed_blob_is_reported_once():
    raw, rows = _typed_packfile()
    assert rows[0][1] == rows[5][1] and rows[0][0] != rows[5][0]
    out, failures, stats = _native([raw, raw], dst_key=KEY_B, dst_compression="GZIP", timestamp=6, **A_LZ4)
    assert failures == {(1, rows[6][1]): _lib.CDC_E_AUTH}
    assert stats["blobs"] == 7 and stats["failed"] == 1 and stats["skipped"] == 7  # the second registration
    got = _rows(out)
    assert [(t, c) for t, c, _ in got] == [(t, c) for t, c, _ in rows[:6]]  # in order, the duplicate checksum twice
    assert sorted({t for t, _, _ in got}) == [1, 2, 3, 4, 5]
    plains = decode.decode_blobs([b for _, _, b in got], key=KEY_B, compressed="GZIP")
    assert plains == [content for _, _, content in rows[:6]]
    # the failure is reported through on_fail exactly once
    calls = []
    with SyncPipeline(dst_key=KEY_B, dst_compression="GZIP", timestamp=6, packers=1, **A_LZ4) as s:
        s.add_packfile(raw)
        s.add_packfile(raw)
        fb = _lib.SYNC_BLOB_FN(lambda ctx, t, c, st: calls.append((t, ctypes.string_at(c, 32), st)))
        pb = _lib.BACKUP_PACK_FN(lambda ctx, data, n: 0)
        assert _lib.lib().cdc_sync_run(s._h, None, 0, pb, fb, None, None) == _lib.CDC_OK
    assert calls == [(1, rows[6][1], _lib.CDC_E_AUTH)]


# ---- 6. known and wanted -----------------------------------------------------------------------
def test_known_blobs_are_skipped_and_wanted_narrows(source):
    _, _, packs = source
    known = set(_keys(packs))
    out, failures, stats = _native(packs, dst_key=KEY_B, known=known, **A_LZ4)
    assert out == [] and failures == {}
    assert stats["blobs"] == 0 and stats["skipped"] == len(_keys(packs)) and stats["batches"] == 0
    assert stats["packfiles"] == 0
    some = sorted(known)[:2]
    out, failures, stats = _native(packs, wanted=some, dst_key=KEY_B, **A_LZ4)
    assert sorted(_keys(out)) == some and stats["blobs"] == 2 and stats["skipped"] == 0
    # a known subset: the others are carried, in order
    half = set(sorted(known)[::2])
    out, failures, stats = _native(packs, dst_key=KEY_B, known=half, **A_LZ4)
    assert _keys(out) == [k for k in _keys(packs) if k not in half] and stats["skipped"] == len(half)
    # wanted and known together; a wanted pair that no packfile holds changes nothing
    out, _, stats = _native(packs, wanted=some + [(9, bytes(32))], dst_key=KEY_B, known={some[0]}, **A_LZ4)
    assert _keys(out) == [some[1]] and stats["skipped"] == 1 and stats["blobs"] == 1


# ---- 7. packfiles by path ----------------------------------------------------------------------
def test_a_truncated_packfile_fails_its_blobs_alone(source, tmp_path):
    _, _, packs = source
    paths = []
    for i, p in enumerate(packs):
        f = tmp_path / f"pack{i}"
        f.write_bytes(p)
        paths.append(str(f))
    with SyncPipeline(dst_key=KEY_B, timestamp=12, packers=1, readers=3, **A_LZ4) as s:
        for f in paths:
            s.add_packfile(f)
        with open(paths[1], "r+b") as f:  # after registration: the index is known, the blobs are gone
            f.truncate(0)
        out, failures, stats = s.run()
    lost = _keys([packs[1]])
    assert failures == {k: _lib.CDC_E_IO for k in lost} and stats["failed"] == len(lost)
    assert _keys(out) == _keys([packs[0]] + packs[2:])
    want, _, _ = _native([packs[0]] + packs[2:], dst_key=None, **A_LZ4)
    got, _, _ = _native([paths[0]] + paths[2:], dst_key=None, **A_LZ4)
    assert got == want  # the path form reads the same bytes


# ---- 8. on_pack stops the run ------------------------------------------------------------------
def test_a_negative_on_pack_status_stops_the_run_and_the_context_runs_again(source):
    _, _, packs = source
    kw = dict(A_LZ4, dst_key=None, max_size=256 << 10, batch_bytes=256 << 10)
    want, _, _ = _native(packs, **kw)
    assert len(want) > 2
    with SyncPipeline(timestamp=12, packers=1, **kw) as s:
        for p in packs:
            s.add_packfile(p)
        calls = []

        def refuse(raw):
            calls.append(raw)
            return -5

        with pytest.raises(_lib.CdcError) as e:
            s.run(on_pack=refuse)
        assert e.value.status == -5 and calls == [want[0]]  # not called again
        got, failures, stats = s.run()
        assert got == want and failures == {} and stats["packfiles"] == len(want)


# ---- 9. a stored length of 0 -------------------------------------------------------------------
def test_a_zero_length_stored_blob_is_carried(tmp_path):
    files = [b"", random_bytes(70_001, 31).tobytes()]
    paths = []
    for i, b in enumerate(files):
        p = tmp_path / f"z{i}"
        p.write_bytes(b)
        paths.append(str(p))
    objs, packs, _ = snapshot.backup_files(paths, repo=_small_chunks(), key=None, compression=None, timestamp=11)
    empty = (1, hashlib.sha256(b"").digest())
    stored = lambda ps: [len(b) for t, c, b in _rows(ps) if (t, c) == empty]  # noqa: E731
    assert stored(packs) == [0]  # stored with no bytes at all
    for dst in ((None, None), (KEY_B, None)):
        kw = dict(src_key=None, src_compression=None, dst_key=dst[0], dst_compression=dst[1])
        out, failures, stats = _native(packs, **kw)
        want, _, ws = _session(packs, **kw)
        assert failures == {} and _keys(out) == _keys(packs) and empty in _keys(out)
        assert [_index(p) for p in out] == [_index(p) for p in want] and stats["blobs"] == ws["blobs"]
        contents, statuses, _ = snapshot.restore_files(objs, out, key=dst[0], compression=dst[1], verify=True)
        assert statuses == [0, 0] and contents == files
    out, _, _ = _native(packs, src_key=None, src_compression=None, dst_key=None, dst_compression=None)
    assert stored(out) == [0]


# ---- 10. a context run twice; what cdc_sync_run checks first -------------------------------------
def test_a_second_run_starts_with_an_empty_taken_set(source):
    _, _, packs = source
    with SyncPipeline(dst_key=None, timestamp=12, packers=1, batch_bytes=512 << 10, **A_LZ4) as s:
        for p in packs:
            s.add_packfile(p)
        first, f1, s1 = s.run()
        second, f2, s2 = s.run()
    assert first == second and f1 == f2 == {} and _keys(first) == _keys(packs)
    assert s1["blobs"] == s2["blobs"] == len(_keys(packs)) and s1["bytes_in"] == s2["bytes_in"]
    assert s1["skipped"] == s2["skipped"] == 0


def test_run_checks_wanted_and_an_empty_context_runs_to_nothing():
    L = _lib.lib()
    calls = []
    pb = _lib.BACKUP_PACK_FN(lambda ctx, data, n: calls.append(n) or 0)
    fb = _lib.SYNC_BLOB_FN(lambda ctx, t, c, st: calls.append(st))
    with SyncPipeline(dst_key=KEY_B, **A_LZ4) as s:
        st = _lib.cdc_sync_stats()
        st.struct_size = ctypes.sizeof(st)
        assert L.cdc_sync_run(s._h, None, 0, pb, fb, None, ctypes.byref(st)) == _lib.CDC_OK  # no packfile registered
        assert (st.packfiles, st.batches, st.blobs, st.path) == (0, 0, 0, sync.PATHS.index("rekey")) and calls == []
        bad = bytes([2]) + bytes(32) + bytes([1]) + bytes(32)  # descending
        assert L.cdc_sync_run(s._h, bad, 2, pb, fb, None, None) == _lib.CDC_E_INVALID
        assert L.cdc_sync_run(s._h, None, 0, _lib.BACKUP_PACK_FN(), fb, None, None) == _lib.CDC_E_INVALID
        st.struct_size = 4
        assert L.cdc_sync_run(s._h, None, 0, pb, fb, None, ctypes.byref(st)) == _lib.CDC_E_INVALID
        assert L.cdc_sync_add_packfile(s._h, b"x" * 60, 60) == _lib.CDC_E_CORRUPT
        assert L.cdc_sync_add_packfile_path(s._h, b"/nonexistent/packfile") == _lib.CDC_E_IO
    assert calls == []
