"""Maintenance on the device (cdc_state_mark, cdc_state_delete_snapshots,
cdc_state_sweep, plakar_amd/maintenance.py) against the rule over Python dicts
(tests/maintenance_ref.py).  States are given in the plain form, serialised
ascending, so a record's number is its place in maintenance_ref's list.  A
plan is compared whole: the packfile list and both row lists as sequences."""
import ctypes
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import maintenance_ref as mref  # noqa: E402
import state_ref as sref  # noqa: E402
import stored_ref as sr  # noqa: E402
import stream_busy as sb  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, maintenance, restore, snapshot, state  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK, OBJECT, SNAP = sref.TYPE_CHUNK, sref.TYPE_OBJECT, sref.TYPE_SNAPSHOT
PACK_FIELDS = ("extent", "live_bytes", "live_rows", "first_record", "row_first", "row_count", "verdict")


def csum(*parts):
    return hashlib.sha256(repr(parts).encode()).digest()


def _open():
    return state.State(key=None, compression=None)


def _merge(S, agg, states, tag="s"):
    """The same states into the library's aggregate and the reference's."""
    plains = [st if isinstance(st, bytes) else st.serialize("asc") for st in states]
    ids = [csum("state", tag, i) for i in range(len(plains))]
    assert S.merge(plains, ids=ids, form="plain") == [0] * len(plains)
    agg.merge(plains)


def _mark(S, agg, refs):
    found, missing = S.mark(refs)
    want_found, want_missing = agg.mark(refs)
    assert found.tolist() == want_found and missing == want_missing
    return found


def _same_plan(plan, want):
    got = [dict(packfile=p, **{f: int(row[f]) for f in PACK_FIELDS})
           for p, row in zip(state._column(plan.packs, "packfile"), plan.packs)]
    assert got == want.packs
    assert state.rows_as_tuples(plan.kept_rows) == want.kept_rows        # as sequences: record order
    assert state.rows_as_tuples(plan.repack_rows) == want.repack_rows
    assert (plan.kept_rows["found"] == 1).all() and (plan.repack_rows["found"] == 1).all()
    assert {k: plan.info[k] for k in want.stats} == want.stats
    # the slices tile the repack rows and ascend in offset
    at = 0
    for p in plan.packs:
        if p["verdict"] != _lib.SWEEP_REPACK:
            assert (p["row_first"], p["row_count"]) == (0, 0)
            continue
        assert p["row_first"] == at and p["row_count"] > 0
        part = plan.repack_rows[at:at + int(p["row_count"])]
        assert (np.diff(part["offset"].astype(np.int64)) >= 0).all()
        assert set(state._column(part, "packfile")) == {bytes(p["packfile"].tobytes())}
        at += int(p["row_count"])
    assert at == len(plan.repack_rows)


def _sweep_both(S, agg, keep_types=1, permille=500):
    plan = S.sweep(keep_types=keep_types, repack_permille=permille)
    _same_plan(plan, agg.sweep(keep_types=keep_types, permille=permille))
    return plan


def _chunks(n, tag, per_pack=5, length=lambda i: 10 + i):
    """n chunk rows, per_pack to a packfile, laid end to end in it."""
    rows, at = [], {}
    for i in range(n):
        pack = csum("pack", tag, i // per_pack)
        rows.append((CHUNK, csum("blob", tag, i), pack, at.get(pack, 0), length(i)))
        at[pack] = at.get(pack, 0) + length(i)
    return rows


# ---- 1. the mark bitmap's word edges ----------------------------------------------------

def test_bitmap_word_edges():
    with _open() as S:
        agg = mref.Aggregate()
        _merge(S, agg, [sref.from_rows(_chunks(70, "edges", per_pack=70))])
        assert len(agg.records) == 70
        edges = [0, 31, 32, 33, 63, 64, 69]
        assert _mark(S, agg, [(CHUNK, agg.records[r][1]) for r in edges]).all()
        plan = _sweep_both(S, agg, keep_types=0, permille=0)
        assert state.rows_as_tuples(plan.kept_rows) == [agg.records[r] for r in edges]
        # a whole wave on one word
        assert _mark(S, agg, [(CHUNK, agg.records[40][1])] * 64).tolist() == [True] * 64
        plan = _sweep_both(S, agg, keep_types=0, permille=0)
        assert state.rows_as_tuples(plan.kept_rows) == [agg.records[r] for r in sorted(edges + [40])]
        # the same checksum under another type marks nothing
        found, missing = S.mark([(OBJECT, agg.records[41][1])])
        assert (found.tolist(), missing) == ([False], 1)
        agg.mark([(OBJECT, agg.records[41][1])])
        assert _sweep_both(S, agg, keep_types=0, permille=0).info["live"] == 8
        # found and missing are exact and in the order of the references
        refs = [(CHUNK, agg.records[1][1]), (CHUNK, csum("absent", 1)), (OBJECT, agg.records[2][1]), (CHUNK, agg.records[69][1]),
                (CHUNK, csum("absent", 2)), (CHUNK, agg.records[1][1])]
        found, missing = S.mark(refs)
        assert (found.tolist(), missing) == ([True, False, False, True, False, True], 3)
        agg.mark(refs)
        assert _sweep_both(S, agg, keep_types=0, permille=0).info["live"] == 9
        # the 33-byte records as one bytes object are the same call
        raw = b"".join(bytes([t]) + c for t, c in refs)
        assert S.mark(raw)[0].tolist() == found.tolist()


# ---- 2. marks accumulate, clear, and survive a merge --------------------------------------

def test_marks_accumulate_clear_and_survive_merges():
    snap = (SNAP, csum("snap"), csum("pack", "snaps"), 0, 40)
    with _open() as S, _open() as T:
        capacity = S.info()["capacity"]
        limit = capacity // 2
        rows = _chunks(limit - 1, "acc") + [snap]
        first, second = mref.Aggregate(), mref.Aggregate()
        _merge(S, first, [sref.from_rows(rows)])
        _merge(T, second, [sref.from_rows(rows)])
        assert S.info()["records"] == limit and S.info()["capacity"] == capacity
        a = [(CHUNK, r[1]) for r in rows[0:200:3]]
        b = [(CHUNK, r[1]) for r in rows[100:400:2]]
        _mark(S, first, a)
        _mark(S, first, b)
        _mark(T, second, a + b)
        plan = _sweep_both(S, first)
        _sweep_both(T, second)
        assert plan.info["live"] == len(set(a + b)) + 1
        # one more record doubles the table; the marks set before still hold, and the newcomer has none
        more = sref.from_rows([(CHUNK, csum("blob", "acc", 3), csum("other pack"), 9, 9), (CHUNK, csum("new"), csum("other pack"), 18, 9)])
        _merge(S, first, [more], tag="more")
        assert S.info()["records"] == limit + 2 and S.info()["capacity"] == 2 * capacity
        again = _sweep_both(S, first)
        assert again.info["live"] == plan.info["live"] and again.info["losers"] == 1
        assert again.packs[-1]["verdict"] == _lib.SWEEP_DROP
        _mark(S, first, [(CHUNK, csum("new"))])
        assert _sweep_both(S, first).info["live"] == plan.info["live"] + 1
        # cleared, nothing is live but the snapshot nobody deleted
        S.clear_marks()
        first.clear_marks()
        cleared = _sweep_both(S, first)
        assert cleared.info["live"] == 1 and state.rows_as_tuples(cleared.kept_rows) == [snap]
        assert _sweep_both(S, first, keep_types=0).info["live"] == 0


# ---- 3. losers ------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [(0, 1, 2), (1, 0, 2)])
def test_losers_are_dead(order):
    P, Q, x = csum("P"), csum("Q"), csum("x")
    states = [sref.from_rows([(CHUNK, x, P, 0, 100), (CHUNK, csum("y"), P, 100, 100)]),
              sref.from_rows([(CHUNK, x, Q, 0, 100)]),
              sref.from_rows([(CHUNK, x, P, 0, 100)])]  # an aggregate state and the delta it extends name one place
    with _open() as S:
        agg = mref.Aggregate()
        _merge(S, agg, [states[i] for i in order])
        _mark(S, agg, [(CHUNK, x)])
        plan = _sweep_both(S, agg, permille=0)
        by = {bytes(p["packfile"].tobytes()): p for p in plan.packs}
        assert plan.info["live"] == 1 and plan.info["losers"] == 2 and plan.info["records"] == 4
        if order[0] == 0:
            assert by[Q]["verdict"] == _lib.SWEEP_DROP and (by[P]["live_rows"], by[P]["live_bytes"]) == (1, 100)
            assert state.rows_as_tuples(plan.kept_rows) == [(CHUNK, x, P, 0, 100)]
        else:
            assert by[P]["verdict"] == _lib.SWEEP_DROP and by[Q]["live_rows"] == 1
            assert state.rows_as_tuples(plan.kept_rows) == [(CHUNK, x, Q, 0, 100)]
        assert by[P]["extent"] == 200 and by[Q]["extent"] == 100


# ---- 4. deleted snapshots -------------------------------------------------------------------

def test_deleted_snapshots():
    a, b, pack = csum("snapshot A"), csum("snapshot B"), csum("pack")
    st = sref.from_rows([(SNAP, a, pack, 0, 10), (SNAP, b, pack, 10, 30), (CHUNK, a, pack, 40, 5),
                         (CHUNK, csum("a chunk only"), pack, 45, 5)])
    with _open() as S, _open() as fresh:
        agg = mref.Aggregate()
        _merge(S, agg, [st])
        assert sorted(S.list_snapshots()) == sorted([a, b])
        # a checksum that is only a chunk is no snapshot, nor is one the aggregate has never seen
        got = S.delete_snapshots([a, csum("a chunk only"), b"\0" * 32], when_ns=77)
        assert got == [0, _lib.CDC_E_NOTFOUND, _lib.CDC_E_NOTFOUND]
        assert agg.delete_snapshots([a, csum("a chunk only"), b"\0" * 32]) == [True, False, False]
        assert S.list_snapshots() == [b] and S.info()["deleted_snapshots"] == 1 and S.info()["records"] == 5
        assert S.blob_exists(SNAP, [a]).tolist() == [True]  # still found, as in the reference
        # deletion beats a mark; the other is live by keep_types
        _mark(S, agg, [(SNAP, a)])
        plan = _sweep_both(S, agg, permille=0)
        assert state.rows_as_tuples(plan.kept_rows) == [(SNAP, b, pack, 10, 30)]
        # with keep_types = 0 both need marks, and A's does not help it
        assert _sweep_both(S, agg, keep_types=0, permille=0).info["live"] == 0
        _mark(S, agg, [(SNAP, b), (CHUNK, a)])
        both = _sweep_both(S, agg, keep_types=0, permille=0)
        assert state.rows_as_tuples(both.kept_rows) == [(CHUNK, a, pack, 40, 5), (SNAP, b, pack, 10, 30)]
        # the delta rm stores, merged into a fresh aggregate, gives the same sweep
        delta = state.serialize_rows([], 5, deleted=[(a, 77)])
        other = mref.Aggregate()
        _merge(fresh, other, [st, delta])
        assert fresh.list_snapshots() == [b]
        _mark(fresh, other, [(SNAP, a), (SNAP, b), (CHUNK, a)])
        again = _sweep_both(fresh, other, keep_types=0, permille=0)
        assert again.packs.tobytes() == both.packs.tobytes() and again.kept_rows.tobytes() == both.kept_rows.tobytes()
        # deleted again: found again, and nothing changes
        assert S.delete_snapshots([a]) == [0] and S.info()["deleted_snapshots"] == 1
        agg.delete_snapshots([a])
        _sweep_both(S, agg, keep_types=0, permille=0)


# ---- 5. verdicts ----------------------------------------------------------------------------

def _verdict_state():
    rows, live = [], []

    def pack(name, parts):
        for k, (off, length, is_live) in enumerate(parts):
            rows.append((CHUNK, csum("blob", name, k), csum("pack", name), off, length))
            if is_live:
                live.append((CHUNK, csum("blob", name, k)))

    pack("at", [(0, 500, True), (500, 500, False)])
    pack("under", [(0, 499, True), (499, 501, False)])
    pack("over", [(0, 501, True), (501, 499, False)])
    pack("dead", [(0, 10, False), (10, 10, False)])
    pack("full", [(0, 300, True), (300, 700, True)])
    # 0xFFFFFFF0 + 0x20 is past 2^32: the extent is a u64 sum
    pack("far dead", [(0, 16, True), (0xFFFFFFF0, 0x20, False)])
    pack("far live", [(0, 16, False), (0xFFFFFFF0, 0x20, True)])
    pack("far half", [(0, 0x80000008, True), (0xFFFFFFF0, 0x20, False)])
    pack("far under", [(0, 0x80000007, True), (0xFFFFFFF0, 0x20, False)])
    return rows, live


@pytest.mark.parametrize("permille", [500, 0, 1000, 1, 999])
def test_verdicts(permille):
    rows, live = _verdict_state()
    K, D, R = _lib.SWEEP_KEEP, _lib.SWEEP_DROP, _lib.SWEEP_REPACK
    with _open() as S:
        agg = mref.Aggregate()
        _merge(S, agg, [sref.from_rows(rows)])
        _mark(S, agg, live)
        plan = _sweep_both(S, agg, permille=permille)
        by = {c: p for c, p in zip(state._column(plan.packs, "packfile"), plan.packs)}
        got = {name: int(by[csum("pack", name)]["verdict"]) for name in
               ("at", "under", "over", "dead", "full", "far dead", "far live", "far half", "far under")}
        for name in ("far dead", "far live", "far half", "far under"):
            assert int(by[csum("pack", name)]["extent"]) == 0x100000010
        assert got["dead"] == D
        if permille == 500:
            assert got == {"at": K, "under": R, "over": K, "dead": D, "full": K, "far dead": R, "far live": R,
                           "far half": K, "far under": R}
            assert plan.info["reclaimable_bytes"] == 501 + 20 + 3 * 0x100000010 - 16 - 0x20 - 0x80000007
        elif permille == 0:
            assert set(got.values()) == {K, D} and len(plan.repack_rows) == 0
        elif permille == 1000:
            assert {n for n, v in got.items() if v == K} == {"full"}
        elif permille == 1:
            assert got["far dead"] == R and got["far live"] == R and got["under"] == K  # 16 and 32 of 4 GiB
        else:
            assert got["full"] == K and got["far half"] == R


# ---- 6. the stable compaction -----------------------------------------------------------------

def test_stable_compaction():
    n = 3000
    # in every other packfile the rows that will be live are the large ones: about 2/3 live there, 1/3 elsewhere
    rows = _chunks(n, "compact", per_pack=100, length=lambda i: 50 if i % 3 == 0 and (i // 100) % 2 else 10 + i % 7)
    with _open() as S:
        agg = mref.Aggregate()
        _merge(S, agg, [sref.from_rows(rows)])
        recs = agg.records
        assert len(recs) == n
        _mark(S, agg, [(CHUNK, recs[i][1]) for i in range(0, n, 3)])
        plan = _sweep_both(S, agg, permille=500)
        assert len(plan.kept_rows) > 100 and len(plan.repack_rows) > 100 and plan.info["live"] == 1000
        # kept rows are in record order across many tiles, not merely the right set
        numbers = {rec[1]: r for r, rec in enumerate(recs)}
        order = [numbers[c] for c in state._column(plan.kept_rows, "checksum")]
        assert order == sorted(order) and order[-1] - order[0] > 4 * 256
        for permille in (0, 1000):
            _sweep_both(S, agg, permille=permille)
        _mark(S, agg, [(CHUNK, rec[1]) for rec in recs])
        full = _sweep_both(S, agg, permille=1000)
        assert state.rows_as_tuples(full.kept_rows) == recs and len(full.repack_rows) == 0
        S.clear_marks()
        agg.clear_marks()
        none = _sweep_both(S, agg)
        assert len(none.kept_rows) == 0 and len(none.repack_rows) == 0 and none.info["drop"] == 30
    with _open() as S:
        empty = _sweep_both(S, mref.Aggregate())
        assert len(empty.packs) == 0 and empty.info["records"] == 0


def _scattered(n):
    """n chunk rows, 1,000 to a packfile; the rows to mark: two thirds of an
    odd packfile's, a fifth of an even one's, so that both row lists run
    through the whole store."""
    rows = _chunks(n, "many tiles", per_pack=1000, length=lambda i: 10 + i % 13)
    live = [i for i in range(n) if ((i % 3 != 0) if (i // 1000) % 2 else (i * 7) % 5 == 0)]
    return rows, live


@pytest.mark.parametrize("blocks", [0, 2], ids=["whole grid", "two blocks"])
def test_compaction_over_many_tiles(blocks):
    """140,000 records are 547 tiles of 256: k_sweep_scan's loop, which takes
    256 tile counts at a time and carries their sum, goes round three times
    (256, 256 and 35 counts), and every row past record 65,536 is placed
    through a carry that is not zero.  Both lists are compared as sequences."""
    n = 140_000
    rows, live = _scattered(n)
    L = _lib.lib()
    assert L.cdc_debug_set_state_blocks(blocks) == 0
    try:
        with _open() as S:
            agg = mref.Aggregate()
            _merge(S, agg, [sref.from_rows(rows)])
            recs = agg.records
            assert len(recs) == n > 2 * 256 * 256 and [r[1] for r in recs[:3]] == [r[1] for r in rows[:3]]
            _mark(S, agg, [(CHUNK, recs[i][1]) for i in live])
            plan = _sweep_both(S, agg, permille=500)
            assert plan.info["keep"] == 70 and plan.info["repack"] == 70
            # rows of both lists lie in each of the scan's three trips
            numbers = {rec[1]: r for r, rec in enumerate(recs)}
            for part in (plan.kept_rows, plan.repack_rows):
                trips = {numbers[c] // (256 * 256) for c in state._column(part, "checksum")}
                assert trips == {0, 1, 2}
    finally:
        assert L.cdc_debug_set_state_blocks(0) == 0


# ---- 7. the grid-stride loops past their first trip -------------------------------------------

BLOCKS, THREADS = 2, 256                      # cdc_debug_set_state_blocks(2); cst::kThreads
ITEMS = 2 * BLOCKS * THREADS + 70             # 1,094


def test_capped_grid():
    """With the grid capped at 2 blocks of 256 lanes the grid-stride loops go
    round at least three times: 3,300 references, 3,400 records (14 tiles of
    the compaction, seven per block), and 1,100 packfiles in a table of 8,192
    slots.  k_sweep_scan's own loop, over 256 tile counts at a time, takes one
    trip here; test_compaction_over_many_tiles sends it round three times."""
    packs, per = 1100, 3
    rows = _chunks(packs * per, "capped", per_pack=per, length=lambda i: 5 + i % 11)
    L = _lib.lib()
    assert L.cdc_debug_set_state_blocks(BLOCKS) == 0
    try:
        with _open() as S:
            agg = mref.Aggregate()
            _merge(S, agg, [sref.from_rows(rows[:1500]), sref.from_rows(rows[1400:])])
            recs = agg.records
            refs = []
            for i, rec in enumerate(recs[:3300]):
                if i % 3 != 2:
                    refs.append((CHUNK, rec[1]))
                if i % 3 == 0:
                    refs.append((CHUNK, rec[1]))
            assert len(refs) == 3300 >= ITEMS and len(recs) == 3400 and packs >= ITEMS
            _mark(S, agg, refs)
            plan = _sweep_both(S, agg, permille=700)
            assert plan.info["packs"] == packs and plan.info["losers"] == 100
            assert plan.info["repack"] > 100 and plan.info["keep"] > 100
            snaps = [csum("snap", i) for i in range(ITEMS)]
            _merge(S, agg, [sref.from_rows([(SNAP, c, csum("snap pack"), 8 * i, 8) for i, c in enumerate(snaps)])], tag="snaps")
            assert S.delete_snapshots(snaps[::2]) == [0] * len(snaps[::2])
            agg.delete_snapshots(snaps[::2])
            assert _sweep_both(S, agg, permille=700).info["live"] == plan.info["live"] + ITEMS // 2
    finally:
        assert L.cdc_debug_set_state_blocks(0) == 0


# ---- 8. mark_device on a busy stream ----------------------------------------------------------

def test_mark_device_on_a_busy_stream():
    rows = _chunks(600, "busy", per_pack=20)
    st = sref.from_rows(rows)
    sums = [r[1] for r in rows[::2]] + [csum("absent", i) for i in range(50)] + [rows[0][1]] * 70
    with _open() as A, _open() as B:
        agg = mref.Aggregate()
        _merge(A, agg, [st])
        assert B.merge([st.serialize("asc")], ids=[csum("b")], form="plain") == [0]
        want_found = _mark(A, agg, [(CHUNK, c) for c in sums])
        want = _sweep_both(A, agg, keep_types=0)
        B.mark([(CHUNK, csum("absent"))])  # the bitmap's allocation is behind B
        sb.calibrate()
        s = torch.cuda.Stream()
        staged = [torch.from_numpy(np.frombuffer(b"".join(sums), dtype=np.uint8).reshape(-1, 32).copy()).cuda()]
        inp = [torch.zeros_like(staged[0])]
        found = torch.full((len(sums),), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def call(stream):
            _lib.check(_lib.lib().cdc_state_mark_device(B._h, CHUNK, ctypes.c_void_p(inp[0].data_ptr()), len(sums),
                                                        ctypes.c_void_p(found.data_ptr()),
                                                        ctypes.c_void_p(stream.cuda_stream)), "cdc_state_mark_device")

        try:
            _, gate = sb.run_busy(call, s, staged, inp)
            still = gate.pending()
            s.synchronize()
            assert still, f"the call did not return while its stream was busy: it is not asynchronous ({sb.calibration()})"
            assert found.cpu().numpy().astype(bool).tolist() == want_found.tolist()
            got = B.sweep(keep_types=0)
            assert got.packs.tobytes() == want.packs.tobytes() and got.kept_rows.tobytes() == want.kept_rows.tobytes()
            assert got.repack_rows.tobytes() == want.repack_rows.tobytes()
            # the wrapper, on the current stream: the other half of the rows, with and without found
            rest = torch.from_numpy(np.frombuffer(b"".join(r[1] for r in rows[1::2]), dtype=np.uint8).reshape(-1, 32).copy()).cuda()
            assert B.mark_device(CHUNK, rest) is None
            f = B.mark_device(CHUNK, rest[:10], found=True)
            torch.cuda.synchronize()
            assert f.cpu().tolist() == [1] * 10 and B.sweep(keep_types=0).info["live"] == 600
        finally:
            torch.cuda.synchronize()


# ---- 9. end to end ----------------------------------------------------------------------------

CONFIGS = [("LZ4", True, "plain"), ("GZIP", False, "plain"), ("LZ4", True, "stored")]


def _repository(tmp_path, comp, key, form):
    """Two backups that share half their files, their states merged, snapshot A deleted."""
    files = [random_bytes(24 << 10, 900 + i).tobytes() + bytes(8 << 10) for i in range(9)]
    paths = []
    for i, b in enumerate(files):
        (tmp_path / f"f{i}").write_bytes(b)
        paths.append(str(tmp_path / f"f{i}"))
    set_a, set_b = [0, 3, 1, 4, 2, 5], [3, 6, 4, 7, 5, 8]
    args = dict(repo=Repository(Configuration("FASTCDC", 2048, 8192, 32768)), key=key, compression=comp, max_size=48 << 10,
                packers=1, packfile_form=form)
    objs_a, packs_a, _ = snapshot.backup_files([paths[i] for i in set_a], timestamp=1, **args)
    delta_a = state.delta_from_packfiles(packs_a, form=form, key=key, compression=comp, timestamp_ns=1)
    repo = Repository()
    assert repo.RebuildState([delta_a], ids=[csum("delta a")], key=key, compression=comp, form="plain") == [0]
    known = set(repo.State().list_blobs(CHUNK))
    objs_b, packs_b, st_b = snapshot.backup_files([paths[i] for i in set_b], known=known, timestamp=2, **args)
    assert st_b["new_blobs"] > 0 and len(packs_a) >= 3 and len(packs_b) >= 2
    delta_b = state.delta_from_packfiles(packs_b, form=form, key=key, compression=comp, timestamp_ns=2)
    snap_a, snap_b, snap_pack = csum("snapshot A"), csum("snapshot B"), csum("the snapshots' packfile")
    snaps = state.serialize_rows([(SNAP, snap_a, snap_pack, 0, 10), (SNAP, snap_b, snap_pack, 10, 90)], 3)
    assert repo.RebuildState([delta_b, snaps], ids=[csum("delta b"), csum("snaps")], form="plain") == [0, 0]
    repo.DeleteSnapshot(snap_a)
    with pytest.raises(KeyError):
        repo.DeleteSnapshot(csum("no such snapshot"))
    by_sum = {hashlib.sha256(p).digest(): p for p in packs_a + packs_b}
    chunks_a = {bytes(c.Checksum) for o in objs_a for c in o.Chunks}
    refs_b = [(CHUNK, bytes(c.Checksum)) for o in objs_b for c in o.Chunks]
    return repo, by_sum, chunks_a, refs_b, objs_b, [files[i] for i in set_b], (snap_a, snap_b, snap_pack)


@pytest.mark.parametrize("comp,keyed,form", CONFIGS, ids=["lz4-key", "gzip", "lz4-key-stored"])
def test_cleanup_end_to_end(tmp_path, comp, keyed, form):
    key = sr.KEY if keyed else None
    repo, by_sum, chunks_a, refs_b, objs_b, files_b, (snap_a, snap_b, snap_pack) = _repository(tmp_path, comp, key, form)
    asked = []

    def packfile_of(c):
        asked.append(c)
        return by_sum[c]

    opts = dict(key=key, compression=comp, packfile_form=form, repack_permille=900, max_size=48 << 10, timestamp=9)
    res = repo.Cleanup(refs_b, packfile_of, **opts)
    assert res.ok and not res.failures and res.new_state is not None
    plan = res.plan
    assert sorted(asked) == sorted(plan.packfiles("repack")) and len(asked) >= 1 and len(res.new_packfiles) >= 1
    assert res.delete_packfiles == plan.packfiles("drop") + plan.packfiles("repack") and plan.info["keep"] >= 2
    assert res.delete_states == [csum("delta a"), csum("delta b"), csum("snaps")]
    # both codecs are the repository's: no blob is decompressed (with a key each is resealed, cdc_sync's "rekey")
    assert res.stats["sync"]["path"] == ("rekey" if keyed else "copy") and res.stats["sync"]["failed"] == 0
    # a fresh aggregate from the new state alone
    only_b = {c for _, c in refs_b}
    with state.State(key=key, compression=comp) as fresh:
        assert fresh.merge([res.new_state], ids=[csum("new")], form="plain") == [0]
        assert sref.deserialize(res.new_state).aggregate and not sref.deserialize(res.new_state).extends
        assert fresh.list_snapshots() == [snap_b] and not fresh.blob_exists(SNAP, [snap_a])[0]
        assert set(fresh.list_blobs(CHUNK)) == only_b
        gone = sorted(chunks_a - only_b)
        assert gone and not fresh.blob_exists(CHUNK, gone).any()
        # restore B from the kept and the new packfiles only
        have = {c: by_sum[c] for c in plan.packfiles("keep") if c != snap_pack}
        have.update(dict(res.new_packfiles))
        needed = fresh.packfile_rows(CHUNK)
        assert set(needed) == set(have)
        order = sorted(needed)
        with restore.RestoreSession(key=key, compression=comp) as rs:
            assert rs.add_packfiles([have[p] for p in order], rows=[needed[p] for p in order]) == [0] * len(order)
            contents, statuses, _ = rs.run(objs_b)
            assert statuses == [0] * len(objs_b) and contents == files_b
        # smaller than before
        kept_extents = sum(int(p["extent"]) for p in plan.packs if p["verdict"] == _lib.SWEEP_KEEP)
        assert kept_extents + sum(len(p) for _, p in res.new_packfiles) < sum(len(p) for p in by_sum.values())
        # a second cleanup on the result, same marks, finds nothing to drop or repack
        fresh.mark(refs_b)
        second = maintenance.cleanup(fresh, packfile_of, **opts)
        assert second.ok and second.delete_packfiles == [] and second.new_packfiles == []
        assert second.plan.info["keep"] == second.plan.info["packs"] == len(have) + 1
        one, two = sref.deserialize(res.new_state), sref.deserialize(second.new_state)
        assert all(one.rows(t) == two.rows(t) for t in sref.TYPES)


# ---- 10. a failed blob ------------------------------------------------------------------------

def test_cleanup_with_a_failed_blob(tmp_path):
    key = sr.KEY
    repo, by_sum, _, refs_b, _, _, _ = _repository(tmp_path, "LZ4", key, "plain")
    S = repo.State()
    S.clear_marks()
    S.mark(refs_b)
    plan = S.sweep(repack_permille=900)
    pack, rows = plan.repack_slices()[0]
    typ, blob, off, length = rows[len(rows) // 2]
    bad = bytearray(by_sum[pack])
    bad[off + length // 2] ^= 0x10  # inside a live blob
    broken = dict(by_sum)
    broken[pack] = bytes(bad)
    res = maintenance.cleanup(S, broken.__getitem__, key=key, compression="LZ4", repack_permille=900, verify=True,
                              max_size=48 << 10, timestamp=9)
    assert not res.ok and res.new_state is None and res.delete_packfiles == [] and res.delete_states == []
    assert list(res.failures) == [(typ, blob)] and res.failures[(typ, blob)] < 0
    # intact, the same plan goes through
    assert maintenance.cleanup(S, by_sum.__getitem__, key=key, compression="LZ4", repack_permille=900, max_size=48 << 10,
                               timestamp=9).ok
