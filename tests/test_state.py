"""The repository state on the device (cdc_state_*, plakar_amd/state.py)
against the reference over Python dicts (tests/state_ref.py, written from
repository/state/state.go).  Stored states are made with tests/stored_ref.py's
encoder (system libraries only).  Every comparison is of sets of rows or of
dicts: the order of a listing is nobody's promise."""
import ctypes
import hashlib
import random
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import state_ref as sref  # noqa: E402
import stored_ref as sr  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, chunkers, device, encode, hashing, restore, snapshot, state  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = pytest.mark.parametrize("cfg", sr.CONFIGS, ids=sr.config_id)
LZ4_KEY = ("LZ4", True)


def csum(*parts):
    return hashlib.sha256(repr(parts).encode()).digest()


def _codec(cfg):
    return cfg[0], (sr.KEY if cfg[1] else None)


def _given(st, cfg, form, seed=1, order="asc"):
    """The state's bytes as merge() takes them in this form."""
    plain = st.serialize(order, seed)
    if form == "plain":
        return plain
    comp, key = _codec(cfg)
    return sr.encoder(comp, key, seed)(plain)


def _open(cfg):
    comp, key = _codec(cfg)
    return state.State(key=key, compression=comp)


def _rows(S, typ):
    r = S.rows(typ)
    assert (r["found"] == 1).all() and (r["type"] == typ).all()
    return set(zip(r["type"].tolist(), state._column(r, "checksum"), state._column(r, "packfile"), r["offset"].tolist(),
                   r["length"].tolist()))


def _same_as_reference(S, agg, absent=()):
    """Listings, lookups of every present key and of `absent`, and the counts."""
    info = S.info()
    for typ in sref.TYPES:
        want = agg.rows(typ)
        if typ != sref.TYPE_SNAPSHOT:
            assert _rows(S, typ) == want, typ
            assert sorted(S.list_blobs(typ)) == sorted(agg.list_blobs(typ))
        assert info["rows"][typ] == len(want)
        keys = [r[1] for r in want] + list(absent)
        if not keys:
            continue
        found, packs, offs, lens = S.get_subpart_for_blob(typ, keys)
        for k, f, p, o, n in zip(keys, found, packs, offs, lens):
            assert (p, int(o), int(n), bool(f)) == agg.get_subpart_for_blob(typ, k), (typ, k.hex())
        assert S.blob_exists(typ, keys).tolist() == [agg.blob_exists(typ, k) for k in keys]
    assert sorted(S.list_snapshots()) == sorted(agg.list_snapshots())
    assert info["deleted_snapshots"] == len(agg.deleted)


def _state_with(per_type, tag, packs=2):
    """per_type rows in every one of the 9 types; keys and locations depend on tag."""
    rows = []
    for typ in sref.TYPES:
        for i in range(per_type):
            rows.append((typ, csum("blob", tag, typ, i), csum("pack", tag, i % packs), 1000 * typ + i, 10 + i))
    return sref.from_rows(rows, timestamp=tag)


# ---- 1. one state -----------------------------------------------------------------------

@CONFIGS
@pytest.mark.parametrize("form", ["stored", "plain"])
@pytest.mark.parametrize("per_type", [0, 1, 3])
def test_one_state(cfg, form, per_type):
    st = _state_with(per_type, tag=per_type)
    sid = csum("state", per_type)
    agg = sref.aggregate_of([(sid, st)])
    absent = [csum("absent", i) for i in range(50)]
    with _open(cfg) as S:
        assert S.merge([_given(st, cfg, form)], ids=[sid], form=form) == [0]
        _same_as_reference(S, agg, absent)
        # a present checksum under each wrong type
        for typ in sref.TYPES:
            for r in agg.rows(typ):
                for other in sref.TYPES:
                    if other != typ:
                        assert not S.blob_exists(other, [r[1]])[0], (typ, other)
        assert S.extends() == [sid]
        info = S.info()
        assert (info["states"], info["rejected"], info["records"]) == (1, 0, 9 * per_type)
        assert info["capacity"] >= 2 * info["records"] and info["device_bytes"] > 0
        # CDC_E_NOSPACE as cdc_packfile_index has it
        if per_type == 3:
            two = np.zeros(2, dtype=state.ROW_DTYPE)
            need = ctypes.c_uint64()
            assert _lib.lib().cdc_state_rows(S._h, 1, two.ctypes.data, 2, ctypes.byref(need)) == _lib.CDC_E_NOSPACE
            assert need.value == 3 and (two["found"] == 1).all() and len(set(state._column(two, "checksum"))) == 2


# ---- 2. precedence ----------------------------------------------------------------------

def _three_overlapping():
    shared = [(1 + i % 3, csum("shared", i)) for i in range(10)]
    states = []
    for s in range(3):
        rows = [(typ, blob, csum("pack", s if i < 5 else "common"), 100 * s + i, 7 + s) for i, (typ, blob) in enumerate(shared)]
        rows += [(1, csum("own", s, i), csum("pack", s), 5000 + i, i) for i in range(20)]
        # the same checksum under two types: two entries
        rows += [(sref.TYPE_CHUNK, csum("twice"), csum("pack", s), 1 + s, 2), (sref.TYPE_OBJECT, csum("twice"), csum("pack", s), 3 + s, 4)]
        states.append((csum("state", s), sref.from_rows(rows, timestamp=s)))
    return states


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
@pytest.mark.parametrize("calls", ["one", "three"])
def test_first_given_state_wins(order, calls):
    states = _three_overlapping()
    given = [states[i] for i in order]
    agg = sref.aggregate_of(given)
    with _open(LZ4_KEY) as S:
        blobs = [_given(st, LZ4_KEY, "stored", seed=5 + k) for k, (_, st) in enumerate(given)]
        ids = [sid for sid, _ in given]
        if calls == "one":
            assert S.merge(blobs, ids=ids) == [0, 0, 0]
        else:
            for b, i in zip(blobs, ids):
                assert S.merge([b], ids=[i]) == [0]
        _same_as_reference(S, agg)
        assert S.extends() == ids
        first = order[0]
        found, packs, offs, lens = S.get_subpart_for_blob(1, [csum("shared", 0), csum("twice")])
        assert found.all() and packs[0] == csum("pack", first) and int(offs[0]) == 100 * first and int(offs[1]) == 1 + first
        found, _, offs, _ = S.get_subpart_for_blob(sref.TYPE_OBJECT, [csum("twice")])
        assert found[0] and int(offs[0]) == 3 + first
        assert S.info()["records"] == 3 * 32  # every record is kept; the table holds the winners


# ---- 3. a state's ids are its own -------------------------------------------------------

def test_each_state_resolves_its_own_ids():
    a = sref.from_rows([(1, csum("a", i), csum("pack A"), i, 1) for i in range(5)])
    b = sref.from_rows([(1, csum("b", i), csum("pack B"), i, 2) for i in range(5)])
    assert a.id_to_checksum[0] == csum("pack A") and b.id_to_checksum[0] == csum("pack B")
    given = [(csum("sa"), a), (csum("sb"), b)]
    with _open(LZ4_KEY) as S:
        assert S.merge([_given(st, LZ4_KEY, "stored") for _, st in given], ids=[i for i, _ in given]) == [0, 0]
        _same_as_reference(S, sref.aggregate_of(given))
        _, packs, _, _ = S.get_subpart_for_blob(1, [csum("a", 3), csum("b", 3)])
        assert packs == [csum("pack A"), csum("pack B")]


# ---- 4. record order --------------------------------------------------------------------

@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_record_order_does_not_matter(order):
    rng = random.Random(4)
    rows = [(rng.randrange(9), csum("blob", i), csum("pack", rng.randrange(7)), rng.randrange(1 << 32), rng.randrange(1 << 32))
            for i in range(300)]
    st = sref.from_rows(rows)
    st.delete_snapshot(csum("an old snapshot"))
    assert sum(len(m) for m in st.maps.values()) == 300
    agg = sref.aggregate_of([(csum("s"), st)])
    with _open(LZ4_KEY) as S:
        assert S.merge([_given(st, LZ4_KEY, "stored", order=order)], ids=[csum("s")]) == [0]
        _same_as_reference(S, agg, [csum("absent", i) for i in range(10)])


# ---- 5. probe chains --------------------------------------------------------------------

def test_colliding_and_extreme_checksums():
    base = csum("base")
    tails = [base[:31] + bytes([v]) for v in range(64)]    # differ in byte 31 only
    heads = [bytes([v]) + base[1:] for v in range(64, 128)]  # differ in byte 0 only
    keys = tails + heads + [bytes(32), b"\xff" * 32]
    rows = [(1, k, csum("pack", i % 3), i, 1 + i) for i, k in enumerate(keys)]
    st = sref.from_rows(rows)
    agg = sref.aggregate_of([(csum("s"), st)])
    absent = [base[:31] + bytes([200]), bytes([200]) + base[1:], bytes(31) + b"\1", b"\xff" * 31 + b"\xfe"]
    with _open(LZ4_KEY) as S:
        assert S.merge([_given(st, LZ4_KEY, "stored")], ids=[csum("s")]) == [0]
        _same_as_reference(S, agg, absent)


def test_table_at_its_load_limit_and_one_more():
    with _open((None, False)) as S:
        capacity = S.info()["capacity"]
        limit = capacity // 2  # cdc_state_stats.capacity: the table holds at most capacity / 2 records
        full = sref.from_rows([(1, csum("blob", i), csum("pack", i % 5), i, i) for i in range(limit)])
        more = sref.from_rows([(1, csum("blob", 3), csum("other pack"), 9, 9), ])
        one = sref.from_rows([(1, csum("one more"), csum("pack", 0), 1, 1)])
        assert S.merge([full.serialize()], ids=[csum("full")], form="plain") == [0]
        info = S.info()
        assert info["records"] == limit and info["capacity"] == capacity
        _same_as_reference(S, sref.aggregate_of([(csum("full"), full)]), [csum("absent")])
        # one more record: the table is rebuilt larger, and the earlier state keeps its locations
        assert S.merge([more.serialize()], ids=[csum("more")], form="plain") == [0]
        info = S.info()
        assert info["records"] == limit + 1 and info["capacity"] == 2 * capacity
        given = [(csum("full"), full), (csum("more"), more)]
        _same_as_reference(S, sref.aggregate_of(given), [csum("absent")])
        assert S.merge([one.serialize()], ids=[csum("one")], form="plain") == [0]
        _same_as_reference(S, sref.aggregate_of(given + [(csum("one"), one)]), [csum("absent")])


# ---- 6. the grid-stride loops past their first trip -------------------------------------

BLOCKS, THREADS = 2, 256                      # cdc_debug_set_state_blocks(2); cst::kThreads
ITEMS = 2 * BLOCKS * THREADS + 70             # 1,094: a third trip for some lanes, and a ragged end


@pytest.mark.parametrize("shape", ["one state of 3000", "40 states of 75", "1100 states of 1"])
def test_capped_grid(shape):
    """With the grid capped at 2 blocks of 256 lanes every stage's loop goes
    round at least three times when it has 1,094 items or more: the id
    records, the location records, the inserts, the queries and the table's
    slots in all three shapes (3,000 rows, over 3,000 ids, 8,192 slots), the
    states themselves (k_state_plan) in the last (1,100 states)."""
    nstates, per = {"one state of 3000": (1, 3000), "40 states of 75": (40, 75), "1100 states of 1": (1100, 1)}[shape]
    given = []
    for s in range(nstates):
        rows = [(1 + (i % 2), csum("blob", s, i), csum("pack", s, i % 4), i, s) for i in range(per)]
        if s % 7 == 0:
            rows.append((sref.TYPE_SNAPSHOT, csum("snap", s), csum("pack", s, 0), 1, 1))
        given.append((csum("state", s), sref.from_rows(rows, timestamp=s)))
    agg = sref.aggregate_of(given)
    assert nstates * per >= ITEMS and len(agg.id_to_checksum) >= ITEMS
    form = "plain" if nstates > 100 else "stored"
    L = _lib.lib()
    assert L.cdc_debug_set_state_blocks(BLOCKS) == 0
    try:
        with _open(LZ4_KEY) as S:
            blobs = [_given(st, LZ4_KEY, form, seed=s) for s, (_, st) in enumerate(given)]
            assert S.merge(blobs, ids=[i for i, _ in given], form=form) == [0] * nstates
            assert S.info()["capacity"] >= ITEMS
            _same_as_reference(S, agg, [csum("absent", i) for i in range(20)])
    finally:
        assert L.cdc_debug_set_state_blocks(0) == 0


# ---- 7. rejected states -----------------------------------------------------------------

def _ids_offset(st):
    return 13 + 8 + 32 * len(st.extends) + 8 + 16 * len(st.deleted) + 8


@pytest.mark.parametrize("fault", ["location id past the count", "packfile id past the count", "an id given twice",
                                   "a deleted snapshot's id past the count"])
def test_rejected_states_are_statuses(fault):
    comp, key = _codec(LZ4_KEY)
    states = [_state_with(2, tag=100 + s) for s in range(5)]
    ids = [csum("state", s) for s in range(5)]
    plains = [st.serialize("shuffle", seed=s) for s, st in enumerate(states)]
    bad = states[3]
    n = len(bad.id_to_checksum)
    if fault == "location id past the count":
        bad.maps[1][n + 5] = (0, 1, 2)
    elif fault == "packfile id past the count":
        bad.maps[1][0] = (n, 1, 2)
    elif fault == "a deleted snapshot's id past the count":
        bad.deleted[n] = 5
    plains[3] = bad.serialize("asc")
    if fault == "an id given twice":  # the second IdToChecksum record names id 0 again
        at = _ids_offset(bad) + 40
        assert struct.unpack_from("<Q", plains[3], at)[0] == 1
        plains[3] = plains[3][:at] + struct.pack("<Q", 0) + plains[3][at + 8:]
    plains[2] = plains[2][:-1]  # a state that ends inside its last section
    blobs = [sr.encoder(comp, key, seed=20 + s)(p) for s, p in enumerate(plains)]
    blobs[1] = blobs[1][:-1] + bytes([blobs[1][-1] ^ 1])  # a GCM tag byte
    with _open(LZ4_KEY) as S:
        assert S.merge(blobs, ids=ids) == [0, _lib.CDC_E_AUTH, _lib.CDC_E_CORRUPT, _lib.CDC_E_CORRUPT, 0]
        agg = sref.aggregate_of([(ids[0], states[0]), (ids[4], states[4])])
        lost = [r[1] for s in (1, 2, 3) for r in _state_with(2, tag=100 + s).rows(1)]
        _same_as_reference(S, agg, lost)
        assert S.extends() == [ids[0], ids[4]]
        info = S.info()
        assert (info["states"], info["rejected"]) == (2, 3)
        # merged again on their own, the good ones change nothing and the bad ones stay out
        assert S.merge([blobs[3]], ids=[ids[3]]) == [_lib.CDC_E_CORRUPT]
        _same_as_reference(S, agg, lost)


# ---- 8. snapshots -----------------------------------------------------------------------

def test_deleted_snapshots_are_listed_out():
    a, b = csum("snapshot A"), csum("snapshot B")
    first = sref.from_rows([(sref.TYPE_SNAPSHOT, a, csum("pack"), 0, 10), (sref.TYPE_SNAPSHOT, b, csum("pack"), 10, 10)])
    later = sref.State()
    later.delete_snapshot(a, when=77)
    given = [(csum("first"), first), (csum("later"), later)]
    agg = sref.aggregate_of(given)
    assert agg.list_snapshots() == [b] and agg.blob_exists(sref.TYPE_SNAPSHOT, a)
    with _open(LZ4_KEY) as S:
        assert S.merge([_given(st, LZ4_KEY, "stored") for _, st in given], ids=[i for i, _ in given]) == [0, 0]
        assert S.list_snapshots() == [b]
        assert S.blob_exists(state.TYPE_SNAPSHOT, [a, b]).tolist() == [True, True]
        _same_as_reference(S, agg)
        assert S.info()["deleted_snapshots"] == 1


# ---- 9. queries that are already on the device ------------------------------------------

def test_lookup_of_device_digests():
    _lib.ensure_init()
    data = random_bytes(1 << 20, 77)
    t = torch.from_numpy(data).cuda()
    cuts = device.chunk_device([t], chunkers.ChunkerOpts(4096, 16384, 65536))[0]
    digests, _ = hashing.chunk_digests(t, cuts, hist=False)
    torch.cuda.synchronize()
    sums = [bytes(d) for d in digests.cpu().numpy()]
    host = data.tobytes()
    assert len(sums) > 30 and sums[0] == hashlib.sha256(host[:int(cuts[0][1])]).digest()
    st = sref.from_rows([(1, c, csum("pack", i % 3), 100 * i, int(cuts[i][1])) for i, c in enumerate(sums) if i % 2 == 0])
    with _open(LZ4_KEY) as S:
        assert S.merge([_given(st, LZ4_KEY, "stored")], ids=[csum("s")]) == [0]
        out = S.lookup_device(1, digests)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(-1).view(state.ROW_DTYPE)
        want = S.lookup(1, sums)
        assert got.tobytes() == want.tobytes()
        assert len(set(sums)) == len(sums)  # random bytes: no chunk twice
        assert got["found"].tolist() == [1 - i % 2 for i in range(len(sums))]
        for i in range(0, len(sums), 2):
            assert (bytes(got["packfile"][i].tobytes()), int(got["offset"][i])) == \
                st.get_subpart_for_blob(1, sums[i])[:2]


# ---- 10. round trip ---------------------------------------------------------------------

def test_backup_state_restore_round_trip(tmp_path):
    comp, key = _codec(LZ4_KEY)
    sizes = [0, 1, 5 << 10, 70 << 10, 150 << 10, 300 << 10, 450 << 10, 600 << 10]
    files = [random_bytes(n, 300 + i).tobytes() for i, n in enumerate(sizes)]
    paths = []
    for i, b in enumerate(files):
        (tmp_path / f"f{i}").write_bytes(b)
        paths.append(str(tmp_path / f"f{i}"))
    args = dict(repo=Repository(Configuration("FASTCDC", 4096, 16384, 65536)), key=key, compression=comp,
                max_size=256 << 10, packers=1, timestamp=31)
    objs, packs, st = snapshot.backup_files(paths, packfile_form="stored", **args)
    assert len(packs) >= 6
    # the delta Commit would store, through Encode, into a repository's aggregate
    delta = state.delta_from_packfiles(packs, form="stored", key=key, compression=comp, timestamp_ns=31)
    want = sref.State()
    for p in packs:
        for typ, c, o, n in sr.read(p, comp, key)[0].index:
            want.set_packfile_for_blob(typ, hashlib.sha256(p).digest(), c, o, n)
    got = sref.deserialize(delta)
    assert got.maps == want.maps and got.id_to_checksum == want.id_to_checksum and got.timestamp == 31
    stored_state = encode.DeviceEncoder(key=key, compression=comp)(delta)
    assert sr.decode(stored_state, comp, key) == delta
    repo = Repository()
    sid = hashlib.sha256(stored_state).digest()
    assert repo.RebuildState([stored_state], ids=[sid], key=key, compression=comp) == [0]
    S = repo.State()
    _same_as_reference(S, sref.aggregate_of([(sid, want)]))
    every = [bytes(c.Checksum) for o in objs for c in o.Chunks]
    assert repo.BlobExists(state.TYPE_CHUNK, every).all() and repo.ListSnapshots() == []
    assert repo.GetSubpartForBlob(state.TYPE_CHUNK, every[:1])[0][0]
    # three of the files from the packfiles the state names, and no others
    pick = [1, 3, 5]
    needed = S.packfile_rows(state.TYPE_CHUNK, [bytes(c.Checksum) for i in pick for c in objs[i].Chunks])
    by_sum = {hashlib.sha256(p).digest(): p for p in packs}
    assert set(needed) <= set(by_sum) and 0 < len(needed) < len(packs)
    for rows in needed.values():
        assert [r[2] for r in rows] == sorted(r[2] for r in rows)
    order = sorted(needed)
    with restore.RestoreSession(key=key, compression=comp) as rs:
        assert rs.add_packfiles([by_sum[p] for p in order], rows=[needed[p] for p in order]) == [0] * len(order)
        contents, statuses, _ = rs.run([objs[i] for i in pick])
        assert statuses == [0, 0, 0] and contents == [files[i] for i in pick]
        # a file whose packfiles were not all registered is not restorable from these
        assert rs.run([objs[7]])[1] == [_lib.CDC_E_NOTFOUND]
    # everything the state lists is known: a second backup stores no chunk
    _, _, st2 = snapshot.backup_files(paths, known=set(S.list_blobs(state.TYPE_CHUNK)), packfile_form="stored", **args)
    assert st2["new_blobs"] == 0 and st["new_blobs"] > 0
    S.close()
