"""Maintenance's checks that need no GPU: the host-only pieces (the verdict
arithmetic and the grouping sort of plakar_amd/csrc/sweep_plan.h, the
DeletedSnapshots writer of state_plan.h) under the sanitizers
(tests/c/sweep_plan_check.cpp), the reference of tests/maintenance_ref.py
against hand-worked cases, the ctypes table and the struct layouts, the
argument checks the entry points make before they touch a device, and the
compiler's resource report of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import maintenance_ref as mref
import state_ref as sref
from plakar_amd import _lib, build, maintenance, repository, snapshot, state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cdc_state_delete_snapshots", "cdc_state_serialize_deleted", "cdc_state_mark", "cdc_state_mark_device",
               "cdc_state_clear_marks", "cdc_sweep_default_opts", "cdc_state_sweep", "cdc_sweep_packs",
               "cdc_sweep_kept_rows", "cdc_sweep_repack_rows", "cdc_sweep_info", "cdc_sweep_free"]
KERNELS = ["k_state_mark", "k_state_missing", "k_state_packs", "k_state_sweep", "k_state_verdict", "k_sweep_classes",
           "k_sweep_scan", "k_sweep_compact"]


def csum(*parts):
    import hashlib
    return hashlib.sha256(repr(parts).encode()).digest()


@pytest.fixture(scope="module")
def sweep_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("swplan") / "sweep_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "plakar_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "c", "sweep_plan_check.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_host_pieces_under_sanitizers(sweep_check_exe):
    """The thresholds at live * 1000 == extent * permille and one byte either
    side, permille 0 and 1000, an extent of 0xFFFFFFF0 + 0x20, 20,000 random
    cases against 128-bit arithmetic; 200 random groupings against a brute
    force; a state with deletions written and read back with splan::read."""
    r = subprocess.run([sweep_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) verdicts, (\d+) groupings, (\d+) writer checks, ok", r.stdout)
    assert m, r.stdout
    verdicts, groupings, writer = (int(g) for g in m.groups())
    assert verdicts >= 20000 + 24 and groupings == 201 and writer == 4
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_reference_on_hand_worked_cases():
    P, Q, R = csum("P"), csum("Q"), csum("R")
    a, b, c, snap = csum("a"), csum("b"), csum("c"), csum("snap")
    s1 = sref.from_rows([(1, a, P, 0, 100), (1, b, P, 100, 300), (0, snap, R, 0, 50)])
    s2 = sref.from_rows([(1, a, Q, 0, 100)])
    s3 = sref.from_rows([(1, a, P, 0, 100), (1, c, P, 400, 600)])
    agg = mref.Aggregate().merge([s1, s2, s3])
    # record numbers: s1 chunks a, b (ids ascending: P 0, a 1, b 2, R 3, snap 4), s1 snapshot, s2 a, s3 a, c
    assert [r[:2] for r in agg.records] == [(1, a), (1, b), (0, snap), (1, a), (1, a), (1, c)]
    assert agg.mark([(1, a), (1, a), (2, a), (1, csum("absent"))]) == ([True, True, False, False], 2)
    plan = agg.sweep(keep_types=1, permille=500)
    assert [p["packfile"] for p in plan.packs] == [P, R, Q] and [p["first_record"] for p in plan.packs] == [0, 2, 3]
    assert (plan.pack(P)["extent"], plan.pack(P)["live_rows"], plan.pack(P)["live_bytes"]) == (1000, 1, 100)
    assert [p["verdict"] for p in plan.packs] == [mref.REPACK, mref.KEEP, mref.DROP]
    assert plan.kept_rows == [(0, snap, R, 0, 50)] and plan.repack_rows == [(1, a, P, 0, 100)]
    assert (plan.pack(P)["row_first"], plan.pack(P)["row_count"]) == (0, 1)
    assert plan.stats == dict(records=6, live=2, dead=4, losers=2, packs=3, keep=1, drop=1, repack=1, kept_rows=1,
                              repack_rows=1, live_bytes=150, reclaimable_bytes=900 + 100)
    # exactly at the threshold is KEEP; deletion beats keep_types and a mark
    agg.mark([(1, b), (1, c)])  # 100 + 300 + 600 of 1000
    assert agg.sweep(permille=1000).pack(P)["verdict"] == mref.KEEP
    agg.clear_marks()
    agg.mark([(1, b), (1, a)])  # 400 of 1000
    assert agg.sweep(permille=400).pack(P)["verdict"] == mref.KEEP
    assert agg.sweep(permille=401).pack(P)["verdict"] == mref.REPACK
    assert agg.delete_snapshots([snap, a]) == [True, False]
    agg.mark([(0, snap)])
    plan = agg.sweep()
    assert plan.pack(R)["verdict"] == mref.DROP and plan.stats["records"] == 6
    # given in the other order, the winner changes with it
    other = mref.Aggregate().merge([s2, s1, s3])
    other.mark([(1, a)])
    plan = other.sweep(keep_types=0)
    assert plan.pack(Q)["live_rows"] == 1 and plan.pack(P)["verdict"] == mref.DROP and plan.pack(R)["verdict"] == mref.DROP


def test_serialize_rows_with_deleted_snapshots():
    """serialize_rows(deleted=...) deserialised by state_ref: the deleted ids
    come after the rows' ids, a checksum a row names keeps its id, and
    without deletions the bytes are the ones cdc_state_serialize writes."""
    rows = [(0, csum("snap", i), csum("pack"), 10 * i, 5) for i in range(3)] + [(1, csum("chunk"), csum("pack"), 99, 1)]
    gone = [(csum("snap", 1), 777), (csum("elsewhere"), -5)]
    data = state.serialize_rows(rows, 123, aggregate=False, extends=[csum("e")], deleted=gone)
    got = sref.deserialize(data)
    want = sref.from_rows(rows, timestamp=123, extends=[csum("e")])
    for c, when in gone:
        want.delete_snapshot(c, when)
    assert got.maps == want.maps and got.id_to_checksum == want.id_to_checksum and got.deleted == want.deleted
    assert got.deleted == {2: 777, 5: -5} and got.id_to_checksum[5] == csum("elsewhere")
    assert data == want.serialize("asc") and len(data) == want.size()
    assert sorted(got.list_snapshots()) == sorted([csum("snap", 0), csum("snap", 2)])
    # no deletion: cdc_state_serialize's bytes
    n = ctypes.c_uint64()
    arr = np.zeros(len(rows), dtype=state.ROW_DTYPE)
    for k, (typ, c, p, off, ln) in enumerate(rows):
        arr[k] = (c, p, off, ln, typ, 0, b"")
    L = _lib.lib()
    assert L.cdc_state_serialize(arr.ctypes.data, len(rows), 123, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_NOSPACE
    out = ctypes.create_string_buffer(n.value)
    assert L.cdc_state_serialize(arr.ctypes.data, len(rows), 123, 0, None, 0, out, n.value, ctypes.byref(n)) == _lib.CDC_OK
    assert out.raw[:n.value] == state.serialize_rows(rows, 123)
    # the delta `rm` stores: deletions alone
    only = sref.deserialize(state.serialize_rows([], 9, deleted=[(csum("snap", 1), 4)]))
    assert only.deleted == {0: 4} and only.id_to_checksum == {0: csum("snap", 1)} and not any(only.maps.values())
    with pytest.raises(ValueError):
        state.serialize_rows([], 0, deleted=[(b"short", 1)])


def test_lib_exports_the_new_symbols():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "plakar_cdc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1], name
        assert re.search(r"\b%s\(" % name, header), name
    assert (_lib.SWEEP_KEEP, _lib.SWEEP_DROP, _lib.SWEEP_REPACK) == (0, 1, 2)
    for name, value in (("KEEP", 0), ("DROP", 1), ("REPACK", 2)):
        assert re.search(r"#define CDC_SWEEP_%s\s+%d\b" % (name, value), header)
    assert "cleanup.go:35-45" in header and "state.go:628-647" in header
    pack = _lib.cdc_sweep_pack
    assert ctypes.sizeof(pack) == 88 == state.PACK_DTYPE.itemsize
    assert [(n, getattr(pack, n).offset) for n, _ in pack._fields_] == \
        [("packfile", 0), ("extent", 32), ("live_bytes", 40), ("live_rows", 48), ("first_record", 56), ("row_first", 64),
         ("row_count", 72), ("verdict", 80), ("reserved", 84)]
    assert [state.PACK_DTYPE.fields[n][1] for n, _ in pack._fields_] == [0, 32, 40, 48, 56, 64, 72, 80, 84]
    assert ctypes.sizeof(_lib.cdc_sweep_opts) == 16 and ctypes.sizeof(_lib.cdc_sweep_stats) == 8 + 12 * 8 + 5 * 8
    o = _lib.cdc_sweep_opts()
    L.cdc_sweep_default_opts(ctypes.byref(o))
    assert (o.struct_size, o.keep_types, o.repack_permille, o.reserved) == (16, 1, 500, 0)
    L.cdc_sweep_default_opts(None)
    # the Python names
    for name in ("cleanup", "CleanupResult", "SweepPlan"):
        assert hasattr(maintenance, name) and name in snapshot.__all__ and hasattr(snapshot, name)
    for name in ("mark", "mark_device", "clear_marks", "sweep", "delete_snapshots"):
        assert callable(getattr(state.State, name))
    assert callable(repository.Repository.DeleteSnapshot) and callable(repository.Repository.Cleanup)
    import plakar_amd
    assert {"state", "maintenance"} <= set(plakar_amd.__all__)


def test_invalid_arguments_return_before_a_device_is_touched():
    """Run without a GPU, a call that reached for a device would be
    CDC_E_DEVICE, not CDC_E_INVALID; and an aggregate nothing was merged into
    answers a sweep, a deletion and clear_marks without one."""
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cdc_state_new(0, 1, None, ctypes.byref(h)) == _lib.CDC_OK and h
    try:
        ref = bytes([1]) + csum("a")
        two = ref + bytes([8]) + csum("b")
        found = (ctypes.c_uint8 * 2)(7, 7)
        miss = ctypes.c_uint64(5)
        assert L.cdc_state_mark(None, two, 2, found, ctypes.byref(miss)) == _lib.CDC_E_INVALID
        assert L.cdc_state_mark(h, None, 2, found, ctypes.byref(miss)) == _lib.CDC_E_INVALID
        for bad in (9, 10, 255):  # the type byte of any record: the whole call
            assert L.cdc_state_mark(h, ref + bytes([bad]) + csum("b"), 2, found, ctypes.byref(miss)) == _lib.CDC_E_INVALID
            assert L.cdc_state_mark(h, bytes([bad]) + csum("b") + ref, 2, found, ctypes.byref(miss)) == _lib.CDC_E_INVALID
        assert (miss.value, list(found)) == (5, [7, 7])
        assert L.cdc_state_mark(h, None, 0, None, ctypes.byref(miss)) == _lib.CDC_OK and miss.value == 0
        assert L.cdc_state_mark(h, None, 0, None, None) == _lib.CDC_OK
        q = ctypes.create_string_buffer(64)
        assert L.cdc_state_mark_device(None, 1, q, 2, None, None) == _lib.CDC_E_INVALID
        assert L.cdc_state_mark_device(h, 9, q, 2, None, None) == _lib.CDC_E_INVALID
        assert L.cdc_state_mark_device(h, 255, q, 2, None, None) == _lib.CDC_E_INVALID
        assert L.cdc_state_mark_device(h, 1, None, 2, None, None) == _lib.CDC_E_INVALID
        assert L.cdc_state_mark_device(h, 1, None, 0, None, None) == _lib.CDC_OK
        assert L.cdc_state_clear_marks(None) == _lib.CDC_E_INVALID
        assert L.cdc_state_clear_marks(h) == _lib.CDC_OK  # nothing was marked: no device needed
        status = (ctypes.c_int32 * 2)(7, 7)
        assert L.cdc_state_delete_snapshots(None, q, 2, 0, status) == _lib.CDC_E_INVALID
        assert L.cdc_state_delete_snapshots(h, None, 2, 0, status) == _lib.CDC_E_INVALID
        assert L.cdc_state_delete_snapshots(h, q, 2, 0, None) == _lib.CDC_E_INVALID
        assert list(status) == [7, 7]
        assert L.cdc_state_delete_snapshots(h, None, 0, 0, None) == _lib.CDC_OK
        # an aggregate without a snapshot row answers without a device
        assert L.cdc_state_delete_snapshots(h, q, 2, 0, status) == _lib.CDC_OK
        assert list(status) == [_lib.CDC_E_NOTFOUND] * 2
        # sweep
        o = _lib.cdc_sweep_opts()
        L.cdc_sweep_default_opts(ctypes.byref(o))
        p = ctypes.c_void_p()
        assert L.cdc_state_sweep(None, ctypes.byref(o), ctypes.byref(p)) == _lib.CDC_E_INVALID
        assert L.cdc_state_sweep(h, ctypes.byref(o), None) == _lib.CDC_E_INVALID
        o.repack_permille = 1001
        assert L.cdc_state_sweep(h, ctypes.byref(o), ctypes.byref(p)) == _lib.CDC_E_INVALID and not p
        o.repack_permille, o.struct_size = 1000, 12
        assert L.cdc_state_sweep(h, ctypes.byref(o), ctypes.byref(p)) == _lib.CDC_E_INVALID and not p
        o.struct_size, o.keep_types = 16, 1 << 9
        assert L.cdc_state_sweep(h, ctypes.byref(o), ctypes.byref(p)) == _lib.CDC_E_INVALID and not p
        o.keep_types = 0x1FF
        for opts in (ctypes.byref(o), None):  # an empty aggregate: an empty plan, and no device
            assert L.cdc_state_sweep(h, opts, ctypes.byref(p)) == _lib.CDC_OK and p
            need = ctypes.c_uint64(5)
            packs = (_lib.cdc_sweep_pack * 1)()
            rows = (_lib.cdc_state_row * 1)()
            assert L.cdc_sweep_packs(p, packs, 1, ctypes.byref(need)) == _lib.CDC_OK and need.value == 0
            assert L.cdc_sweep_kept_rows(p, rows, 1, ctypes.byref(need)) == _lib.CDC_OK and need.value == 0
            assert L.cdc_sweep_repack_rows(p, rows, 1, None) == _lib.CDC_OK
            assert L.cdc_sweep_packs(None, packs, 1, ctypes.byref(need)) == _lib.CDC_E_INVALID
            assert L.cdc_sweep_packs(p, None, 1, ctypes.byref(need)) == _lib.CDC_E_INVALID
            assert L.cdc_sweep_kept_rows(p, None, 1, ctypes.byref(need)) == _lib.CDC_E_INVALID
            assert L.cdc_sweep_repack_rows(None, rows, 1, ctypes.byref(need)) == _lib.CDC_E_INVALID
            st = _lib.cdc_sweep_stats()
            assert L.cdc_sweep_info(p, ctypes.byref(st)) == _lib.CDC_E_INVALID  # struct_size not set
            assert L.cdc_sweep_info(p, None) == _lib.CDC_E_INVALID
            st.struct_size = ctypes.sizeof(st)
            assert L.cdc_sweep_info(None, ctypes.byref(st)) == _lib.CDC_E_INVALID
            assert L.cdc_sweep_info(p, ctypes.byref(st)) == _lib.CDC_OK
            assert (st.records, st.live, st.dead, st.packs, st.reclaimable_bytes) == (0, 0, 0, 0, 0)
            L.cdc_sweep_free(p)
            p = ctypes.c_void_p()
    finally:
        L.cdc_state_free(h)
    L.cdc_sweep_free(None)
    n = ctypes.c_uint64()
    rows = (_lib.cdc_state_row * 1)()
    gone, when = ctypes.create_string_buffer(32), (ctypes.c_int64 * 1)(1)
    ser = L.cdc_state_serialize_deleted
    assert ser(None, 1, None, None, 0, 0, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert ser(rows, 1, None, when, 1, 0, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert ser(rows, 1, gone, None, 1, 0, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert ser(rows, 1, gone, when, 1, 0, 0, None, 1, None, 0, ctypes.byref(n)) == _lib.CDC_E_INVALID
    assert ser(rows, 1, gone, when, 1, 0, 0, None, 0, None, 0, None) == _lib.CDC_E_INVALID
    assert ser(rows, 1, gone, when, 1, 0, 0, None, 0, None, 0, ctypes.byref(n)) == _lib.CDC_E_NOSPACE
    assert n.value == 109 + 16 + 40 + 24  # one id: the zero checksum is the row's blob, its packfile and the snapshot


def test_python_layer_checks_its_arguments():
    with state.State(key=None, compression=None) as s:
        with pytest.raises(ValueError):
            s.mark([(9, csum("a"))])
        with pytest.raises(ValueError):
            s.mark([(1, b"short")])
        with pytest.raises(ValueError):
            s.mark(b"x" * 34)
        with pytest.raises(ValueError):
            s.sweep(repack_permille=1001)
        with pytest.raises(ValueError):
            s.sweep(keep_types=(9,))
        with pytest.raises(ValueError):
            s.delete_snapshots([b"short"])
        found, missing = s.mark([])
        assert found.tolist() == [] and missing == 0
        plan = s.sweep()
        assert len(plan.packs) == len(plan.kept_rows) == len(plan.repack_rows) == 0 and plan.info["records"] == 0
        assert plan.repack_slices() == [] and plan.packfiles("drop") == []
        assert s.delete_snapshots([csum("a")]) == [_lib.CDC_E_NOTFOUND]
        s.clear_marks()
        with pytest.raises(ValueError):
            maintenance.cleanup(s, lambda c: b"", packfile_form="rows")
        # nothing to do: an empty aggregate state, nothing to delete, packfile_of never asked
        res = maintenance.cleanup(s, None, timestamp=5)
        assert res.ok and res.new_packfiles == [] and res.delete_packfiles == [] and res.delete_states == [] and not res.failures
        got = sref.deserialize(res.new_state)
        assert got.aggregate and got.timestamp == 5 and not any(got.maps.values()) and not got.extends
    with pytest.raises(ValueError):
        repository.Repository().DeleteSnapshot(csum("a"))  # RebuildState has not run


def test_new_kernels_use_no_private_segment():
    path = build.resources_path()
    assert os.path.exists(path), f"{path}: the library is built by plakar_amd.build, which keeps the compiler's report"
    text = open(path).read()
    for k in KERNELS:
        m = re.search(r"Function Name: \S*%s\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)" % k, text, re.S)
        assert m, k
        assert (int(m.group(1)), int(m.group(2))) == (0, 0), (k, m.groups())
