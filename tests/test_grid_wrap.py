"""Every kernel loop that runs under a capped grid, taken past its first trip.

A grid capped by the CU count (or by a constant) sends a wave or a workgroup
round its loop again once there are more work items than the cap, with the
registers and the LDS of the item before.  Each case here has about
2 * cap + 70 items, so the first trip, the second and a partial third all
run, and is held to the plain reference its kernel's own test module uses:
exact equality everywhere.  The caps are mirrored below from
plakar_amd/csrc; tests/test_grid_caps_cpu.py compares them with the sources,
so that a changed cap fails there instead of leaving these cases short of the
wrap."""
import functools
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import diff_ref  # noqa: E402
import test_diff  # noqa: E402
import test_diff_emit  # noqa: E402
import test_digest  # noqa: E402
import test_entropy  # noqa: E402
import test_line_table  # noqa: E402
import test_restore  # noqa: E402
from datagen import random_bytes  # noqa: E402
from plakar_amd import hashing, snapshot  # noqa: E402
from plakar_amd.chunking import Configuration  # noqa: E402
from plakar_amd.repository import Repository  # noqa: E402
from test_diff_emit import sources  # noqa: E402,F401 - the module's fixture
from test_restore import src_np  # noqa: E402,F401 - the module's fixture

pytestmark = pytest.mark.gpu

# ---- the caps of plakar_amd/csrc, mirrored --------------------------------------------
kThreads = 256           # cdc_diff.hip: four waves per workgroup
kBlocksPerCU = 8         # cdc_diff.hip (grid_for) and cdc_restore.hip (k_assemble)
kEmitBlocksPerCU = 32    # cdc_diff.hip: k_diff_emit, one wave per workgroup
kHistBlocksPerCU = 8     # cdc_digest.hip: k_chunk_hist
kHistWaves = 4
kEntMaxBlocks = 2048     # cdc_digest.hip: k_chunk_entropy
kEntWaves = 4
LINE_TILE = 16384        # cdc_diff.hip kTile
ASSEMBLE_TILE = 64 << 10  # cdc_restore.hip kTile

# file -> constant -> (the value mirrored here, the cases to resize when it changes)
MIRRORED = {
    "cdc_diff.hip": {
        "kThreads": (kThreads, "test_line_table_past_w_tiles, test_long_line_hash_and_verify_past_w, "
                               "test_one_diff_batch_past_w_tiles"),
        "kBlocksPerCU": (kBlocksPerCU, "test_line_table_past_w_tiles, test_long_line_hash_and_verify_past_w, "
                                       "test_one_diff_batch_past_w_tiles"),
        "kEmitBlocksPerCU": (kEmitBlocksPerCU, "test_emit_past_w_units"),
        "kTile": (LINE_TILE, "test_line_table_past_w_tiles"),
    },
    "cdc_restore.hip": {
        "kBlocksPerCU": (kBlocksPerCU, "test_assemble_past_the_grid"),
        "kTile": (ASSEMBLE_TILE, "test_assemble_past_the_grid"),
    },
    "cdc_digest.hip": {
        "kHistBlocksPerCU": (kHistBlocksPerCU, "test_histograms_and_digests_past_w_chunks, "
                                               "test_one_backup_batch_past_w_cut_slots"),
        "kHistWaves": (kHistWaves, "test_histograms_and_digests_past_w_chunks, test_one_backup_batch_past_w_cut_slots"),
        "kEntMaxBlocks": (kEntMaxBlocks, "test_entropy_past_8192_rows"),
        "kEntWaves": (kEntWaves, "test_entropy_past_8192_rows"),
    },
}
assert kBlocksPerCU * (kThreads // 64) == kEmitBlocksPerCU == kHistBlocksPerCU * kHistWaves == 32  # W below is all three
ENT_ROWS = kEntMaxBlocks * kEntWaves  # 8,192 rows in flight, whatever the device

KEY = bytes(range(96, 128))
P, L, N = diff_ref.PREFIX, diff_ref.LITERAL, diff_ref.NEWLINE


@functools.lru_cache(maxsize=None)
def _cus():
    """The CU count cdc::device_cus reads."""
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _w():
    """Waves (k_line_*, k_chunk_hist) or workgroups (k_diff_emit) in flight: 32 per CU."""
    return 32 * _cus()


# ---- a. the line table past W tiles ---------------------------------------------------
def test_line_table_past_w_tiles():
    """2 W + 70 texts of 0-40 bytes, one tile each (every seventh is empty: one
    empty tile), and three texts of several tiles whose tiles lie across tile
    W - 1 | W and 2 W - 1 | 2 W, so a text's tiles are counted and marked in
    different trips of different waves (k_line_count, k_line_mark)."""
    W = _w()
    TILE = LINE_TILE
    rng = np.random.default_rng(101)
    alphabet = np.frombuffer(b"ab\n", dtype=np.uint8)
    big = {W - 1: TILE + 1, W + 1: 2 * TILE, 2 * W - 2: 2 * TILE + 5}  # first tile -> bytes
    bodies, first_tile, tile, small = [], [], 0, 0
    while small < 2 * W + 70 or tile <= max(big):
        if tile in big:
            n = big[tile]
        else:
            n = 0 if small % 7 == 0 else int(rng.integers(1, 41))
            small += 1
        bodies.append(bytes(rng.choice(alphabet, n)))
        first_tile.append(tile)
        tile += max(1, -(-n // TILE))
    assert small == 2 * W + 70 and tile == 2 * W + 70 + 7
    where = {len(b): first_tile[i] for i, b in enumerate(bodies) if len(b) > TILE}
    assert where == {TILE + 1: W - 1, 2 * TILE: W + 1, 2 * TILE + 5: 2 * W - 2}
    # TILE + 1: tiles W - 1 | W; 2 TILE + 5: tiles 2 W - 2, 2 W - 1 | 2 W; 2 TILE: tiles W + 1, W + 2, right behind
    # the first, so tiles W - 1 .. W + 2 are all full tiles of two texts across the first wrap
    texts, off = [], 0
    for b in bodies:
        texts.append((off, len(b)))
        off += len(b) + 1  # a newline between the texts: it belongs to neither
    buf = b"\n".join(bodies)
    counts = [b.count(b"\n") + 1 for b in bodies]
    groups = [0]
    for i in range(0, len(bodies), 2):  # pairs of texts
        groups.append(groups[-1] + sum(counts[i:i + 2]))
    test_line_table._run(buf, texts, groups=groups, bits=(0, 4))


# ---- b. long lines past W -------------------------------------------------------------
def test_long_line_hash_and_verify_past_w():
    """2 W + 70 non-empty lines of 1-600 bytes drawn with repeats from a pool,
    every one hashed by a wave (threshold 1) and, for the repeats, compared by
    a wave: more than W entries in both long lists (k_line_hash_long,
    k_line_verify_long).  Four lines past 16 KiB among the last W take the
    hash's inner loop round again on a later trip."""
    W = _w()
    rng = np.random.default_rng(102)
    n = 2 * W + 70
    pool, seen = [], set()
    while len(pool) < min(2000, W // 2):
        ln = bytes(rng.integers(11, 256, int(rng.integers(1, 601)), dtype=np.uint8))
        if ln not in seen:
            seen.add(ln)
            pool.append(ln)
    lines = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    x = bytes(rng.integers(11, 256, 16385, dtype=np.uint8))
    y = bytes(rng.integers(11, 256, 40000, dtype=np.uint8))
    for at, ln in ((n - W + 3, x), (n - W // 2, x[:-1] + b"\x0b"), (n - 71, y), (n - 2, x)):
        lines[at] = ln
    ids = diff_ref.first_ids(lines)
    assert sum(1 for i, k in enumerate(ids) if k != i) > W  # one comparison launch with more than W long items
    buf = b"\n".join(lines)
    r = test_line_table._run(buf, [(0, len(buf))], thresholds=(test_line_table.LANE, test_line_table.WAVE), bits=(0, 4))
    assert r["len"].tolist() == [len(ln) for ln in lines]


# ---- c. emit past W units -------------------------------------------------------------
def _emit_units(recs):
    """The records of each unit as cdc_diff_emit_device forms them (0: a piece
    of a long record), to assert what the case is built for."""
    units, cur, cur_bytes, nxt = [], 0, 0, -1
    for i, r in enumerate(recs):
        ln, f = int(r["len"]), int(r["flags"])
        out = ln + bool(f & P) + bool(f & N)
        if not out:
            continue
        if ln >= 2048:
            if cur:
                units.append(cur)
            cur = cur_bytes = 0
            units.extend([0] * -(-ln // 16384))
            continue
        if cur and (cur == 64 or cur_bytes + out > 8192 or nxt != i):
            units.append(cur)
            cur = cur_bytes = 0
        cur += 1
        cur_bytes += out
        nxt = i + 1
    if cur:
        units.append(cur)
    return units


def test_emit_past_w_units(sources):  # noqa: F811
    """W + 40 records of 2,048-2,100 bytes (a piece unit each), a run of k
    records of 0-100 bytes before each (a unit of k records), k cycling through
    1..64 with a period that moves units u and u + W apart, so a workgroup's
    next unit has more records than the LDS tables hold from the one before, or
    fewer; four records of three pieces each at the end."""
    W = _w()
    rng = np.random.default_rng(103)
    half = W // 2  # a workgroup's units u and u + W are runs j and j + W / 2
    period = next(p for p in range(64, 200) if p / 4 <= half % p <= 3 * p / 4)
    short_flags = [P | N | ord("+"), P | N | ord("-"), P | N | ord(" "), N, P | ord("-"), L | P | N | ord(" "), L | N, N]
    specs = []
    for j in range(W + 40):
        k = 1 + (j % period) % 64
        lens = rng.integers(1, 101, k)
        lens[rng.random(k) < 0.06] = 0  # records of no bytes: a prefix and/or a newline alone
        which = rng.integers(0, len(short_flags), k)
        specs += [(int(n), short_flags[int(w)]) for n, w in zip(lens, which)]
        specs.append((int(rng.integers(2048, 2101)), [P | N | ord("+"), N, 0, P | ord("-")][j % 4]))
        if j % 97 == 50:
            specs.append((0, L if j % 2 else 0))  # nothing to write at all: no unit holds it
    specs += [(40000, P | N | ord("-")), (39990, 0), (40001, N), (40007, P | N | ord(" "))]
    recs, end = test_diff_emit._records(specs, start=5)
    units = _emit_units(recs)
    assert len(units) >= 2 * W + 70 and units[-12:] == [0] * 12
    pairs = list(zip(units, units[W:]))
    gains = sum(1 for a, b in pairs if 0 < a < b)
    loses = sum(1 for a, b in pairs if 0 < b < a)
    assert gains >= W // 8 and loses >= W // 8, (period, gains, loses)
    test_diff_emit._check(sources, recs, end)


# ---- d. assemble past 8 CUS tiles -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _assemble_layout(src_size):
    cap = kBlocksPerCU * _cus()
    target = (2 * cap + 3) * ASSEMBLE_TILE
    rng = np.random.default_rng(104)
    specs, total = [], 0
    while total < target:
        mix = [4 << 20, (1 << 20) + 3, 65537] + [int(n) for n in rng.integers(1, 201, 200)]
        specs += [(n, int(rng.integers(0, 16)), int(rng.integers(0, 16))) for n in mix]
        total += sum(mix)
    segs, _ = test_restore._layout(rng, specs, src_size)
    segs = [s for s in segs if s[2] + s[1] <= target - 300]
    segs.append((12345, 100, target - 200))  # the last tile holds a segment
    return segs, target, cap


@pytest.mark.parametrize("dst_shift", [0, 5])
def test_assemble_past_the_grid(src_np, dst_shift):  # noqa: F811
    """A destination of 2 * 8 CUS + 3 tiles of 64 KiB: every workgroup of
    k_assemble searches the table again from a new tile, twice, and three take
    a fourth tile; 4-MiB, 1-MiB and 64-KiB segments between runs of 200 tiny
    ones, so the search lands inside long segments and among short ones."""
    segs, size, cap = _assemble_layout(src_np.size)
    first, last = segs[0][2], segs[-1][2] + segs[-1][1]
    assert first < 128 and len(segs) > 200
    assert (last + dst_shift - 1) // ASSEMBLE_TILE - (first + dst_shift) // ASSEMBLE_TILE + 1 == 2 * cap + 3
    test_restore._run_assemble(src_np, segs, size, dst_shift)


# ---- e. histograms and digests past W chunks ------------------------------------------
def test_histograms_and_digests_past_w_chunks():
    """2 W + 70 chunks of one buffer, at every alignment: 0-300 bytes, every
    64th 5,000 (the 1-KiB step of k_chunk_hist goes round), a quarter empty,
    placed so that chunk c is empty where c + W is not and the reverse: counts
    left in the LDS copies by the chunk before would show in either."""
    W = _w()
    rng = np.random.default_rng(105)
    n = 2 * W + 70
    lens = rng.integers(1, 301, n)
    c = np.arange(n)
    lens[(c + c // W) % 4 == 0] = 0  # W is a multiple of 4: c empty -> c + W not; c % 4 == 3 in its trip -> c + W empty
    lens[c % 64 == 63] = 5000
    a, b = lens[:-W], lens[W:]
    assert int(((a > 0) & (b == 0)).sum()) >= W // 8 and int(((a == 0) & (b > 0)).sum()) >= W // 8
    cuts, off = [], 0
    for k, m in enumerate(lens):
        off += k % 7
        cuts.append((off, int(m)))
        off += int(m)
    assert {o % 16 for o, m in cuts if m} == set(range(16))
    buf = random_bytes(off + 64, 1050)
    d, h = test_digest._run(buf, cuts)
    test_digest._check(buf, cuts, d, h)


# ---- f. entropy past 8,192 rows -------------------------------------------------------
def test_entropy_past_8192_rows():
    """3 * 8,192 + 5 rows: test_entropy's rows, then seeded sparse and dense
    ones; an all-zero row where the same wave's next row is dense, and the
    reverse, in both wraps."""
    rng = np.random.default_rng(106)
    base = test_entropy._rows()
    n = 3 * ENT_ROWS + 5
    more = n - base.shape[0]
    bits = rng.integers(1, 20, (more, 1))
    vals = (rng.integers(0, 1 << 30, (more, 256)) >> (30 - bits)) + 1
    keep = rng.random((more, 256)) < rng.random((more, 1))
    keep[np.arange(more), rng.integers(0, 256, more)] = True
    rows = np.concatenate([base, vals * keep])
    dense = rng.integers(1, 1 << 12, (8, 256))
    for k, r in enumerate((400, 1001, 4097, 8191)):
        order = (0, 1, 0) if k % 2 else (1, 0, 1)  # dense, empty, dense / empty, dense, empty
        for trip, full in enumerate(order):
            if r + trip * ENT_ROWS < n:
                rows[r + trip * ENT_ROWS] = dense[2 * k + trip % 2] if full else 0
    assert rows.shape == (n, 256) and int(rows.max()) < 1 << 26
    lens = rows.sum(1)
    want = hashing.entropy_rows(rows, lens)
    got = hashing.chunk_entropy_device(torch.from_numpy(rows.astype(np.int32)).cuda()).cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"
    for i in (0, 400, 400 + ENT_ROWS, 1001 + ENT_ROWS, n - 1):  # the scalar form too
        assert got[i] == hashing.entropy_from_freq(rows[i].tolist(), int(lens[i]))


# ---- g. one backup batch past W cut slots ---------------------------------------------
BATCH_FILES = 4000  # a batch of the backup pipeline holds at most 4,096 files


def test_one_backup_batch_past_w_cut_slots(tmp_path):
    """One batch of the backup pipeline with 2 W + 70 cut slots in its one
    digest buffer, so k_chunk_hist and k_chunk_entropy go round inside the
    pipeline.  A file takes len / MinSize + 2 slots and a batch at most 4,096
    files, so files of 1-300 bytes alone stop at 8,192 slots (W on 256 CUs):
    half the files here are such (two slots, the second empty), the others a
    few MinSize (4 KiB in this repository) long, with the slots they need to
    reach the total.  Every object and every chunk against hashlib and the
    host entropy; the pipeline sorts a batch's files by size, largest first."""
    W = _w()
    rng = np.random.default_rng(107)
    cfg = Configuration("FASTCDC", 4096, 16384, 65536)
    nfiles = min(BATCH_FILES, (2 * W + 70) // 4)  # four slots a file on average, or more
    nsmall = nfiles // 2
    nbig = nfiles - nsmall
    slots = 2 * W + 70 - 2 * nsmall  # of the files past MinSize: three or more each
    lens = [int(n) for n in rng.integers(1, 301, nsmall)]
    for i in range(nbig):
        k = slots // nbig + (i < slots % nbig)  # this file's slots
        lens.append((k - 2) * cfg.MinSize + int(rng.integers(0, cfg.MinSize)))
    lens = [lens[int(i)] for i in rng.permutation(nfiles)]
    files = [random_bytes(n, 7000 + i).tobytes() for i, n in enumerate(lens)]
    order = sorted(range(nfiles), key=lambda i: -lens[i])  # stable, as the pipeline's
    slot0 = np.cumsum([0] + [lens[i] // cfg.MinSize + 2 for i in order])
    assert slot0[-1] == 2 * W + 70  # past 2 * 8,192 rows of k_chunk_entropy too from 256 CUs on
    paths = test_diff._write(tmp_path, files)
    objs, _, st = snapshot.backup_files(paths, repo=Repository(cfg), key=KEY, compression="LZ4")
    assert st["batches"] == 1 and st["files"] == nfiles and st["failed_files"] == 0
    sample = {order[0], order[-1]}
    for slot in (W, 2 * W):
        j = int(np.searchsorted(slot0, slot, side="right")) - 1  # the file that holds the slot
        sample.update(order[k] for k in (j - 1, j, j + 1) if 0 <= k < nfiles)
    sample.update(range(0, nfiles, 89))
    for i, (f, o) in enumerate(zip(files, objs)):
        assert o.Checksum == hashlib.sha256(f).digest(), f"file {i}"
        assert sum(c.Length for c in o.Chunks) == len(f) and 1 <= len(o.Chunks) <= len(f) // cfg.MinSize + 1, f"file {i}"
        off = 0
        for k, c in enumerate(o.Chunks):
            part = f[off:off + c.Length]
            off += c.Length
            freq = np.bincount(np.frombuffer(part, np.uint8), minlength=256)
            assert c.Checksum == hashlib.sha256(part).digest() and c.Length == len(part) > 0, f"file {i} chunk {k}"
            assert c.Entropy == hashing.entropy_from_freq(freq.tolist(), len(part)), f"file {i} chunk {k}"
            if i in sample:
                assert list(c.Distribution) == [x / len(part) for x in freq.tolist()], f"file {i} chunk {k}"


# ---- h. one diff batch past W tiles ---------------------------------------------------
def test_one_diff_batch_past_w_tiles(tmp_path):
    """16 CUS + 40 pairs of texts of 3-12 lines, every pair different, some
    texts without a final newline: 32 CUS + 80 texts, a tile each, in one
    batch of cdc_diff_files; every text is difflib's."""
    npairs = 16 * _cus() + 40
    blobs, want = [], []
    for i in range(npairs):
        a = test_diff._text(3 + i % 10, 3000 + i)
        la = a.split(b"\n")
        lb = list(la)
        lb[i % (len(la) - 1)] = b"pair %d" % i
        if i % 4 == 0:
            del lb[1:2]
        b = b"\n".join(lb)
        if i % 5 == 1:
            a = a[:-1]
        if i % 5 == 3:
            b = b[:-1]
        assert a != b and 3 <= a.count(b"\n") + (not a.endswith(b"\n")) <= 12
        blobs += [a, b]
        want.append(diff_ref.expected_diff(a, b, b"a/%d" % i, b"b/%d" % i))
    assert 2 * npairs > _w()  # a tile per text
    paths = test_diff._write(tmp_path, blobs)
    objs, packs, _ = snapshot.backup_files(paths, key=KEY, compression="LZ4", timestamp=7)
    jobs = [(objs[2 * i], objs[2 * i + 1], "a/%d" % i, "b/%d" % i) for i in range(npairs)]
    res, st = snapshot.diff_files(jobs, packs, key=KEY, compression="LZ4")
    assert st["batches"] == 1 and st["failed_pairs"] == 0 and st["skipped_pairs"] == 0
    for i, (r, w) in enumerate(zip(res, want)):
        assert r["status"] == 0 and r["text"] == w, f"pair {i}"
    assert st["verify_rounds"] == 1
