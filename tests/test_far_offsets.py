"""Every device entry point below cdc_chunk at byte offsets that do not fit in
32 bits.

The ABI takes a device base pointer and 64-bit offsets everywhere, and most
entry points return 64-bit output offsets that a kernel computes with a prefix
sum.  An offset held in 32 bits for one step, a `16 * i` done in 32 bits, a
narrowed 64-bit shuffle or a truncated base address is invisible below 4 GiB.
Part A hands every entry point sources (and, where it takes one, a
destination) that start just below, just above and well above 2^31 and 2^32,
next to a control item at 1 MiB in the same batch, in shuffled order (two
batches: the items across the boundaries and the items just past them overlap,
see BATCHES).  Part B lets the running output offset of Encode, Decode, prefix
Decode and Transcode pass 2^32 inside one call.

The arena is 2^32 + 64 MiB of torch.empty and is never filled as a whole.
Whatever is placed at or across 2^32 gets a decoy first: other bytes of the same
length at its address modulo 2^32, so that a truncated address reads (or
leaves) something definite inside the arena and the case fails by comparison.
Everything is exact, against hashlib, numpy, zlib, liblz4, libcrypto and
difflib (crypto_ref, decode_ref, diff_ref)."""
import ctypes
import functools
import hashlib
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import crypto_ref  # noqa: E402
import decode_ref  # noqa: E402
import diff_ref  # noqa: E402
from datagen import random_bytes, text_like  # noqa: E402
from plakar_amd import _lib, archive, check, decode, diff, encode, hashing, restore, sync  # noqa: E402
from test_archive_zip import _crc_mul, _crc_shift  # noqa: E402

pytestmark = pytest.mark.gpu

MIB = 1 << 20
B31, B32 = 1 << 31, 1 << 32
ARENA = B32 + 64 * MIB
N = 200_003  # four 64-KiB GCM pieces, twenty-five 8-KiB segments, seven 32-KiB spans
KEY = bytes(range(7, 39))
KEY_B = bytes(range(100, 132))
SENTINEL = 0xA5
GUARD = 64

# name -> (where it starts, its content kind)
PLACES = {
    "near": (1 * MIB, "random"),             # the control
    "across-2^31": (B31 - 100_001, "random"),
    "past-2^31": (B31 + 4_099, "text"),
    "across-2^32": (B32 - 100_001, "text"),
    "past-2^32": (B32 + 4_099, "random"),
    "far": (B32 + 32 * MIB + 1, "text"),
}
NAMES = list(PLACES)
POS = {k: v[0] for k, v in PLACES.items()}
# An item of N bytes that starts at B - 100,001 ends past B + 4,099, so the items across a boundary and the
# ones just past it cannot lie in the arena together: two batches, each with the control and the far item,
# in a shuffled order, so that far and near items meet in the same workgroups and waves.
BATCHES = {"across": ["across-2^32", "near", "far", "across-2^31"], "past": ["far", "past-2^31", "near", "past-2^32"]}
BIG_AT, BIG_LEN = B32 + 40 * MIB + 3, MIB + 3  # the digests' large chunk

_peak = [0]


def _used():
    free, total = torch.cuda.mem_get_info()
    return total - free


def _need(nbytes, what):
    """Skip with the reason when the device has less free memory than the case needs."""
    free, _ = torch.cuda.mem_get_info()
    free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()  # torch's own cached blocks are reusable
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")


@pytest.fixture(autouse=True)
def _watch_memory():
    yield
    _peak[0] = max(_peak[0], _used())
    torch.cuda.empty_cache()  # the library allocates beside torch: give back what a case held


@pytest.fixture(scope="module")
def arena():
    _lib.ensure_init()
    _need(ARENA + 256 * MIB, "the arena")
    t = torch.empty(ARENA, dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()
    print(f"\ntest_far_offsets: peak device memory in use {_peak[0] / 2 ** 30:.1f} GiB")


@pytest.fixture(scope="module")
def arena2():
    """A second arena, for the calls that write at far offsets: source and destination must not alias."""
    _need(ARENA + 256 * MIB, "the second arena")
    t = torch.empty(ARENA, dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.fixture(params=list(BATCHES))
def order(request):
    """The names of one batch's items, in batch order."""
    return BATCHES[request.param]


def _role(order):
    """(near, the item at 2^31, the item at 2^32, far) of a batch."""
    return "near", next(k for k in order if "2^31" in k), next(k for k in order if "2^32" in k), "far"


@functools.lru_cache(maxsize=None)
def _items():
    out = {}
    for i, (name, (_, kind)) in enumerate(PLACES.items()):
        out[name] = bytes(text_like(N, 300 + i)) if kind == "text" else random_bytes(N, 300 + i).tobytes()
        assert len(out[name]) == N
    return out


def _dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _place(t, at, data):
    """data at t[at:], after a decoy at the same address modulo 2^32 for the part that lies past 2^32."""
    n = len(data)
    assert at + n + 4096 <= t.numel()
    lo = max(at, B32)
    if lo < at + n:
        decoy = random_bytes(at + n - lo, at % 9973 + 1)
        t[lo - B32:at + n - B32].copy_(torch.from_numpy(decoy))
        assert decoy.tobytes() != bytes(data[lo - at:])
    if n:
        t[at:at + n].copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))


def _place_all(t, blobs):
    """{name: bytes} at their places; no item overlaps another or a decoy."""
    spans = sorted((POS[k], POS[k] + len(b)) for k, b in blobs.items())
    assert all(e <= s for (_, e), (s, _) in zip(spans, spans[1:])), "items overlap"
    for a, b in spans:
        if b > B32:
            assert all(e <= max(a, B32) - B32 or b - B32 <= s for s, e in spans), "a decoy lands on an item"
    for name, b in blobs.items():
        _place(t, POS[name], b)


def _get(t, at, n):
    return t[at:at + n].cpu().numpy().tobytes()


def _items_in(arena, order):
    items = {k: _items()[k] for k in order}
    _place_all(arena, items)
    return items


def _rows(n, seed):
    return random_bytes(56 * n, seed).tobytes()


def _gzip(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def _stored(plain, compression, key, seed):
    """A blob as a repository with this codec stores it, written by liblz4 / zlib / libcrypto."""
    body = plain if not compression else _gzip(plain) if compression == "GZIP" else decode_ref.lz4f_compress(plain)
    return decode_ref.seal_stream(key, body, seed) if key is not None else body


def _read_back(blob, compression, key):
    body = crypto_ref.decrypt_stream(key, blob)[0] if key is not None else blob
    if not compression:
        return body
    return zlib.decompress(body, 31) if compression == "GZIP" else crypto_ref.lz4f_decompress(body)


def _sel(compression):
    return "GZIP" if compression == "GZIP" else bool(compression)


# ======================================================================================
# A. far sources, small outputs
# ======================================================================================
ENCODE_SETTINGS = [(None, None, 0), (KEY, None, 0)] + [(k, c, lv) for c in ("LZ4", "GZIP") for k in (None, KEY)
                                                       for lv in (0, 1, 9)]


def _sid(s):
    key, comp, level = s
    return f"{'key' if key else 'plain'}-{comp or 'none'}-{level}"


@pytest.mark.parametrize("setting", ENCODE_SETTINGS, ids=_sid)
def test_encode_from_far_sources(arena, order, setting):
    """encode_device with base = the arena: every blob read back by libcrypto
    and liblz4 / zlib, and the whole output equal to the same items encoded
    from a compact tensor with the same random bytes."""
    key, comp, level = setting
    items = _items_in(arena, order)
    offs = [POS[k] for k in order]
    lens = [N] * len(order)
    cap = sum(encode.encode_bound(N, _sel(comp), key is not None) for _ in order)
    rnd = _rows(len(order), 41) if key else None
    out = torch.full((cap + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(arena, offs, lens, out, key=key, compress=_sel(comp), random=rnd, level=level)
    assert oo[0] == 0 and (np.diff(oo) > 0).all() and oo[-1] <= cap
    host = out.cpu().numpy()
    assert (host[int(oo[-1]):] == SENTINEL).all()
    for i, name in enumerate(order):
        blob = host[oo[i]:oo[i + 1]].tobytes()
        assert _read_back(blob, comp, key) == items[name], f"blob {i} ({name} at {POS[name]:#x})"
    compact = _dev(b"".join(items[k] for k in order))
    out2 = torch.full((cap + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo2 = encode.encode_device(compact, [N * i for i in range(len(order))], lens, out2, key=key, compress=_sel(comp),
                               random=rnd, level=level)
    assert oo2.tolist() == oo.tolist()
    assert torch.equal(out, out2), "the output depends on where the source lies"


DECODE_SETTINGS = [(None, None), (KEY, None), (None, "LZ4"), (KEY, "LZ4"), (None, "GZIP"), (KEY, "GZIP")]


@functools.lru_cache(maxsize=None)
def _stored_item(name, comp, key):
    return _stored(_items()[name], comp, key, 500 + NAMES.index(name))


def _blobs_in(arena, order, comp, key):
    items = {k: _items()[k] for k in order}
    blobs = {k: _stored_item(k, comp, key) for k in order}
    _place_all(arena, blobs)
    return items, blobs


@pytest.mark.parametrize("setting", DECODE_SETTINGS, ids=lambda s: _sid(s + (0,))[:-2])
def test_decode_prefix_and_check_from_far_sources(arena, order, setting):
    """Blobs written by liblz4, zlib and libcrypto at the far places: exact
    plaintext, status 0 and exact out_offsets from decode_device and from
    decode_prefix_device; cdc_check_device finds the one wrong checksum."""
    key, comp = setting
    items, blobs = _blobs_in(arena, order, comp, key)
    n = len(order)
    offs = [POS[k] for k in order]
    lens = [len(blobs[k]) for k in order]
    out = torch.full((n * N + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo, st = decode.decode_device(arena, offs, lens, out[:n * N], key=key, compressed=_sel(comp))
    assert st.tolist() == [0] * n
    assert oo.tolist() == [N * i for i in range(n + 1)]
    host = out.cpu().numpy()
    assert host[:n * N].tobytes() == b"".join(items[k] for k in order)
    assert (host[n * N:] == SENTINEL).all()
    for upto in (1, 70_000, N):
        out.fill_(SENTINEL)
        oo, st = decode.decode_prefix_device(arena, offs, lens, [upto] * n, out[:n * upto], key=key, compressed=_sel(comp))
        assert st.tolist() == [0] * n, upto
        assert oo.tolist() == [upto * i for i in range(n + 1)]
        host = out.cpu().numpy()
        assert host[:n * upto].tobytes() == b"".join(items[k][:upto] for k in order), upto
        assert (host[n * upto:] == SENTINEL).all()
    mixed = [70_000, 0, N, 65_536]  # and a different prefix of each blob in one call
    oo, st = decode.decode_prefix_device(arena, offs, lens, mixed, out, key=key, compressed=_sel(comp))
    assert st.tolist() == [0] * n and oo.tolist() == np.concatenate([[0], np.cumsum(mixed)]).tolist()
    assert out[:int(oo[-1])].cpu().numpy().tobytes() == b"".join(items[k][:u] for k, u in zip(order, mixed))
    # Check: every checksum right but one
    wrong = order.index(_role(order)[2])  # the one at 2^32
    sums = [hashlib.sha256(items[k]).digest() for k in order]
    sums[wrong] = hashlib.sha256(b"something else").digest()
    offs_a, lens_a = np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64)
    st_a = np.zeros(n, dtype=np.int32)
    needed = ctypes.c_uint64()
    p64 = ctypes.POINTER(ctypes.c_uint64)
    scratch = torch.empty(n * N + 4096, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().cdc_check_device(0, ctypes.c_void_p(arena.data_ptr()), offs_a.ctypes.data_as(p64), lens_a.ctypes.data_as(p64),
                                     n, _lib.compress_code(comp), key, b"".join(sums), ctypes.c_void_p(scratch.data_ptr()),
                                     scratch.numel(), ctypes.byref(needed), st_a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert st_a.tolist() == [_lib.CDC_E_MISMATCH if i == wrong else 0 for i in range(n)]


TRANSCODE_PATHS = {"rekey": ((KEY, "LZ4"), (KEY_B, "LZ4")), "open": ((KEY, "LZ4"), (None, "LZ4")),
                   "seal": ((None, "LZ4"), (KEY_B, "LZ4")), "reencode": ((KEY, "LZ4"), (KEY_B, "GZIP"))}


@pytest.mark.parametrize("path", list(TRANSCODE_PATHS))
def test_transcode_from_far_sources(arena, order, path):
    """transcode_device with checksums on: every output blob opened and
    inflated by the references; the sizes of the paths that keep the
    compression are cdc_transcode_size's."""
    src, dst = TRANSCODE_PATHS[path]
    assert sync.path_of(src, dst) == path
    items, blobs = _blobs_in(arena, order, src[1], src[0])
    n = len(order)
    offs = [POS[k] for k in order]
    lens = [len(blobs[k]) for k in order]
    sums = [hashlib.sha256(items[k]).digest() for k in order]
    cap = sum(encode.encode_bound(N, _sel(dst[1]), dst[0] is not None) for _ in order)
    out = torch.full((cap + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    oo, st = sync.transcode_device(arena, offs, lens, out[:cap], src=src, dst=dst, checksums=sums,
                                   random=_rows(n, 42) if dst[0] else None)
    assert st.tolist() == [0] * n
    if path != "reencode":
        sizes = [sync.transcode_size(m, src[0] is not None, dst[0] is not None) for m in lens]
        assert oo.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    host = out.cpu().numpy()
    assert (host[int(oo[-1]):] == SENTINEL).all()
    for i, name in enumerate(order):
        assert _read_back(host[oo[i]:oo[i + 1]].tobytes(), dst[1], dst[0]) == items[name], f"blob {i} ({name})"
    sums[2] = hashlib.sha256(b"something else").digest()  # and the checksums are looked at
    oo, st = sync.transcode_device(arena, offs, lens, out[:cap], src=src, dst=dst, checksums=sums,
                                   random=_rows(n, 42) if dst[0] else None)
    assert st.tolist() == [_lib.CDC_E_MISMATCH if i == 2 else 0 for i in range(n)] and oo[2] == oo[3]


# two segments per item: the second starts 16-byte aligned in none of them, the first in one
CUT = 70_001


def test_assemble_from_far_sources(arena, order):
    """Far src_off into a compact destination: each item in two segments, 64
    sentinel bytes around every segment, the whole destination compared."""
    items = _items_in(arena, order)
    segs, want, d = [], bytearray(), 0
    for name in order:
        for a, b in ((0, CUT), (CUT, N)):
            want += bytes([SENTINEL]) * GUARD
            d += GUARD
            segs.append((POS[name] + a, b - a, d))
            want += items[name][a:b]
            d += b - a
    want += bytes([SENTINEL]) * GUARD
    for shift in (0, 5):  # the destination 16-byte aligned, and not
        dst = torch.full((shift + len(want),), SENTINEL, dtype=torch.uint8, device="cuda")
        restore.assemble_device(arena, segs, dst[shift:])
        torch.cuda.synchronize()
        assert dst[shift:].cpu().numpy().tobytes() == bytes(want), f"shift {shift}"
        assert (dst[:shift] == SENTINEL).all()


def test_assemble_to_far_destinations(arena2, order):
    """A compact source into far dst_off of the second arena: the destination
    bytes equal the source, the 64 bytes on each side of every segment stay."""
    items = _items()
    src = _dev(b"".join(items[k] for k in order))
    at = {k: N * i for i, k in enumerate(order)}
    segs = []
    for name in sorted(order, key=lambda k: POS[k]):  # destinations ascend
        # decoys where a truncated destination would land, then the guards and a fill the copy must replace
        _place(arena2, POS[name] - GUARD, bytes([SENTINEL]) * (N + 3 * GUARD))
        arena2[POS[name]:POS[name] + CUT].fill_(0x11)
        arena2[POS[name] + CUT + GUARD:POS[name] + N + GUARD].fill_(0x11)
        segs.append((at[name], CUT, POS[name]))
        segs.append((at[name] + CUT, N - CUT, POS[name] + CUT + GUARD))  # a guard between the two halves too
    restore.assemble_device(src, segs, arena2)
    torch.cuda.synchronize()
    g = bytes([SENTINEL]) * GUARD
    for name in order:
        got = _get(arena2, POS[name] - GUARD, N + 3 * GUARD)
        assert got == g + items[name][:CUT] + g + items[name][CUT:] + g, name


def _far_cuts(order):
    """(offset, length) chunks at the batch's places: the items, the SHA-256
    padding edges across, up to and just past both boundaries (those that lie
    inside an item of the batch), and one chunk past 1 MiB."""
    cuts = [(POS[k], N) for k in order]
    for b in (B31, B32):
        for n in (0, 1, 55, 56, 64):
            edge = [(b - n // 2, n), (b - n, n), (b, n), (b + 4_099 + n, n)]  # across, ending at, starting at, past
            cuts += [(o, m) for o, m in edge if any(POS[k] <= o and o + m <= POS[k] + N for k in order)]
    assert len(cuts) >= len(order) + 10
    cuts += [(POS["far"] + 7, 64), (POS["far"] + 9, 55), (POS["near"] + 3, 56), (BIG_AT, BIG_LEN), (POS["far"], 0)]
    return cuts


def _digest_arena(arena, order):
    items = _items_in(arena, order)
    big = random_bytes(BIG_LEN, 77).tobytes()
    _place(arena, BIG_AT, big)

    def data(o, n):
        if o == BIG_AT:
            return big[:n]
        for k, b in items.items():
            if POS[k] <= o and o + n <= POS[k] + N:
                return b[o - POS[k]:o - POS[k] + n]
        raise AssertionError((o, n))
    return data


def _check_digests(data, cuts, d, h):
    d, h = d.cpu().numpy(), h.cpu().numpy()
    for i, (o, n) in enumerate(cuts):
        part = data(o, n)
        assert bytes(d[i]) == hashlib.sha256(part).digest(), f"chunk {i} ({o:#x}, {n})"
        assert (h[i] == np.bincount(np.frombuffer(part, np.uint8), minlength=256)).all(), f"histogram {i} ({o:#x}, {n})"


def test_chunk_digests_at_far_cuts(arena, order):
    """chunk_digests, chunk_digests_batch and chunk_digests_hybrid with data =
    the arena against hashlib.sha256 and numpy.bincount."""
    data = _digest_arena(arena, order)
    cuts = _far_cuts(order)
    ct = torch.tensor(np.asarray(cuts, dtype=np.int64), device="cuda")
    d, h = hashing.chunk_digests(arena, ct)
    torch.cuda.synchronize()
    _check_digests(data, cuts, d, h)
    small = random_bytes(300_000, 78)
    scuts = [(5, 100_000), (100_007, 0), (150_000, 150_000)]
    bufs = [_dev(small), arena]
    lists = [torch.tensor(np.asarray(scuts, dtype=np.int64), device="cuda"), ct]
    sdata = lambda o, n: small[o:o + n].tobytes()  # noqa: E731
    outs = hashing.chunk_digests_batch(bufs, lists)
    torch.cuda.synchronize()
    _check_digests(sdata, scuts, *outs[0])
    _check_digests(data, cuts, *outs[1])
    nonempty = sum(1 for _, n in cuts + scuts if n)
    for host_min_len in (0, 1, 1 << 40):  # the library's balance, every chunk's SHA-256 on the host, none
        outs, hc, hb = hashing.chunk_digests_hybrid(bufs, lists, host_threads=8, host_min_len=host_min_len)
        torch.cuda.synchronize()
        _check_digests(sdata, scuts, *outs[0])
        _check_digests(data, cuts, *outs[1])
        assert (hc, hb) == {1: (nonempty, sum(n for _, n in cuts + scuts)), 1 << 40: (0, 0)}.get(host_min_len, (hc, hb))


def test_object_digests_of_far_segments(arena, order):
    """Objects whose segment lists mix the near, the boundary and the far
    items, against hashlib over the concatenation.  In the batch whose items lie
    across the boundaries, byte 100,001 of an item is the boundary's: the
    30-byte and 64-byte segments around it lie across 2^31 and 2^32."""
    data = _digest_arena(arena, order)
    near, m31, m32, far = (POS[k] for k in _role(order))
    objects = [
        [(near, N), (m32, N), (far, N)],
        [(m31 + 99_990, 30), (near + 1, 1), (m32 + 99_990, 30), (m32, 55)],
        [(m32 + 99_937, 64), (m32 + 100_001, 64), (near, 0), (m31 + 100_000, 2), (BIG_AT, BIG_LEN), (m31 + 7, 65_537)],
        [(far + 100_000, 100_003)],
        [],
        [(m32 + k * 1000, 999 + k) for k in range(100)] + [(near + k * 64, 63) for k in range(100)],
        [(POS[k], N) for k in sorted(order, key=lambda k: -POS[k])],
    ]
    got = check.object_digests_device(arena, objects).cpu().numpy()
    for i, segs in enumerate(objects):
        assert bytes(got[i]) == hashlib.sha256(b"".join(data(o, n) for o, n in segs)).digest(), f"object {i}"


# ---- the line table, the ids and the emit plan ---------------------------------------
@functools.lru_cache(maxsize=None)
def _line_text(seed, n=N):
    """n bytes of lines: pool lines that repeat, numbered lines that do not,
    empty ones; a line of 20,000 bytes (more than a tile) across byte 100,001,
    where a text placed at B - 100,001 meets the boundary, and two equal lines
    of 5,000 bytes (a wave hashes and compares them)."""
    rng = np.random.default_rng(seed)
    pool = [b"pool line %d " % k * (1 + k % 3) for k in range(40)]
    long5 = bytes(rng.integers(11, 256, 5_000, dtype=np.uint8))
    lines, total, big = [], 0, False
    while total < n:
        r = int(rng.integers(0, 10))
        if not big and total > 92_000:
            big = True
            new = [bytes(rng.integers(11, 256, 20_000, dtype=np.uint8)), b"after the long line", long5, b"between", long5]
        elif r < 3:
            new = [pool[int(rng.integers(0, len(pool)))]]
        elif r == 3:
            new = [b""]
        else:
            new = [b"%d: " % len(lines) + bytes(text_like(int(rng.integers(1, 120)), seed + len(lines)))]
        lines += new
        total += sum(len(x) + 1 for x in new)
    return b"\n".join(lines)[:n]


def _changed(text, seed):
    """The text with a line in a hundred replaced, a few removed and a few added."""
    rng = np.random.default_rng(seed)
    lines = text.split(b"\n")
    out = []
    for i, ln in enumerate(lines):
        r = int(rng.integers(0, 300))
        if ln == b"after the long line":
            out.append(b"after the long line, changed")  # the 20,000-byte line is context: copied from the plaintext
        elif r < 3 and len(ln) < 200:
            out.append(b"changed %d" % i)
        elif r == 3 and len(ln) < 200:
            continue
        elif r == 4:
            out += [ln, b"added %d" % i]
        else:
            out.append(ln)
    return b"\n".join(out)


def test_line_table_ids_and_emit_at_far_texts(arena, arena2, order):
    """Texts at the far places: the records (off at or above 2^32 among them)
    against diff_ref.line_records, the ids against diff_ref.first_ids with all
    hash bits and with 4 (nearly every line is compared byte for byte); then
    the two pairs' emit plans with dst_base across and past 2^32 and plain =
    the arena, executed into the second arena, against difflib."""
    near, m31, m32, far = _role(order)
    pairs = [(near, m32), (m31, far)]
    texts = {}
    for i, (a, b) in enumerate(pairs):
        texts[a] = _line_text(900 + i)
        texts[b] = _changed(texts[a], 910 + i)
        assert abs(len(texts[b]) - N) < 4000
    _place_all(arena, texts)
    names = [k for pair in pairs for k in pair]  # a pair's texts are neighbours in the table: one group
    table = [(POS[k], len(texts[k])) for k in names]
    recs, counts = diff.line_table_device(arena, table)
    r = recs.cpu().numpy().reshape(-1).view(diff.LINE_DTYPE).reshape(-1)
    want = [diff_ref.line_records(texts[k], POS[k]) for k in names]
    assert counts.tolist() == [len(w) for w in want]
    flat = [x for w in want for x in w]
    assert r["off"].tolist() == [o for o, _ in flat] and r["len"].tolist() == [n for _, n in flat]
    assert max(o for o, _ in flat) >= B32 and not r["reserved"].any()
    lines = [ln for k in names for ln in texts[k].split(b"\n")]
    by_line = {}
    for ln, h in zip(lines, r["hash"].tolist()):
        assert by_line.setdefault(ln, tuple(h)) == tuple(h), "equal lines with different hashes"
    groups = [0]
    for a, b in pairs:
        groups.append(groups[-1] + texts[a].count(b"\n") + 1 + texts[b].count(b"\n") + 1)
    want_ids = []
    for g0, g1 in zip(groups, groups[1:]):
        want_ids += diff_ref.first_ids(lines[g0:g1])
    for bits in (0, 4):
        ids, rounds = diff.line_ids_device(arena, r, groups, hash_bits=bits)
        assert ids.tolist() == want_ids, bits
        assert rounds >= 1
    # the emit plans, one per pair, executed in one call
    bases = [B32 - 3_000, B32 + 12_345 + MIB]  # across 2^32 (more than asked for), and past it
    all_recs, lit, expect = [], b"", []
    for (a, b), (g0, g1), base in zip(pairs, zip(groups, groups[1:]), bases):
        na = texts[a].count(b"\n") + 1
        ops = diff.diff_ops(want_ids[g0:g0 + na], want_ids[g0 + na:g1])
        er, el, size = diff.diff_emit_plan(ops, r[g0:g0 + na], r[g0 + na:g1], "a/" + a, "b/" + b, dst_base=base, lit_base=len(lit))
        w = diff_ref.expected_diff(texts[a], texts[b], b"a/" + a.encode(), b"b/" + b.encode())
        assert size == len(w) > 20_000 and int(er["dst_off"].min()) == base
        assert any(int(x["len"]) >= 20_000 and not int(x["flags"]) & diff_ref.LITERAL for x in er), "the long line from the plaintext"
        all_recs.append(er)
        lit += el
        expect.append((base, w))
        _place(arena2, base - GUARD, bytes([SENTINEL]) * (size + 2 * GUARD))
    er = np.concatenate(all_recs)
    assert int(er["src_off"][(er["flags"] & diff_ref.LITERAL) == 0].max()) >= B32
    diff.diff_emit_device(arena, _dev(lit), er, arena2)
    torch.cuda.synchronize()
    g = bytes([SENTINEL]) * GUARD
    for base, w in expect:
        got = _get(arena2, base - GUARD, len(w) + 2 * GUARD)
        assert got == g + w + g, f"the diff at {base:#x}"


@pytest.mark.parametrize("level", [0, 1])
def test_zip_pieces_from_far_sources(arena, order, level):
    """Every item an entry of two pieces at a far `off`: each entry's deflate
    bytes raw-inflated by zlib, the CRC registers combined to zlib.crc32, the
    descriptor's sizes."""
    items = _items_in(arena, order)
    pieces, headers = [], b""
    for e, name in enumerate(order):
        h = bytes((11 * e + i) & 255 for i in range(30 + e))
        pieces.append(dict(off=POS[name], len=CUT, first=True, last=False, hdr_off=len(headers), hdr_len=len(h), hdr=h, name=name,
                           body=items[name][:CUT]))
        pieces.append(dict(off=POS[name] + CUT, len=N - CUT, first=False, last=True, crc_reg=zlib.crc32(items[name][:CUT]) ^ 0xFFFFFFFF,
                           csize_before=0, usize_before=CUT, name=name, body=items[name][CUT:]))
        headers += h
    cap = sum(archive.zip_piece_bound(p["len"], p.get("hdr_len", 0)) for p in pieces)
    out = torch.full((cap + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    total, outs = archive.zip_pieces_device(arena, pieces, headers, out, out_cap=cap, level=level)
    host = out.cpu().numpy()
    assert total <= cap and (host[total:] == SENTINEL).all()
    data = host[:total].tobytes()
    at, raw, reg = 0, b"", None
    for p, o in zip(pieces, outs):
        assert o["out_off"] == at
        at += o["out_len"]
        q = o["out_off"]
        if p["first"]:
            assert data[q:q + p["hdr_len"]] == p["hdr"]
            q += p["hdr_len"]
            raw, reg = b"", 0xFFFFFFFF
        raw += data[q:q + o["deflate_len"]]
        assert o["crc_reg"] == zlib.crc32(p["body"]) ^ zlib.crc32(bytes(p["len"])), p["name"]
        reg = _crc_mul(reg, _crc_shift(p["len"])) ^ o["crc_reg"]
        if not p["last"]:
            csize = o["deflate_len"]
            continue
        body = items[p["name"]]
        assert reg ^ 0xFFFFFFFF == zlib.crc32(body), p["name"]
        z = zlib.decompressobj(-15)
        assert z.decompress(raw) == body and z.eof and z.unused_data == b"", p["name"]
        assert len(raw) == csize + o["deflate_len"]
        desc = data[q + o["deflate_len"]:q + o["deflate_len"] + 16]
        assert desc == struct.pack("<IIII", 0x08074B50, zlib.crc32(body), o["deflate_len"], N)  # csize_before was 0
    assert at == total


# ======================================================================================
# B. outputs whose running offset passes 2^32
# ======================================================================================
F = 64 * MIB   # one source region ...
NB = 68        # ... named by 68 blobs: 4.25 GiB of output
SEALED = 12 + 48 + F + 28 * (F // 65536)  # a sealed blob of F stored bytes
LZ4_STORED = 7 + (F // (4 * MIB)) * 4 + F + 4 + 4  # an LZ4 frame of stored 4-MiB blocks


def _opened(n_bytes):
    """The blobs to open by reference: the first, the one across 2^32, the one after it and the last."""
    s = B32 // n_bytes
    assert 0 < s < NB - 2 and s * n_bytes < B32 < (s + 1) * n_bytes
    return [0, s, s + 1, NB - 1]


@pytest.fixture(scope="module")
def source():
    host = random_bytes(F, 64)
    return host, torch.from_numpy(host).cuda()


def _equal_each(out, oo, want, what):
    for i in range(len(oo) - 1):
        assert torch.equal(out[int(oo[i]):int(oo[i + 1])], want), f"{what}: blob {i} at {int(oo[i]):#x}"


def _decode_all(out, oo, src_dev, key, compressed):
    """decode_device of the NB blobs of `out`: sources past 2^32 and an output that passes it again."""
    dec = torch.empty(NB * F + 4096, dtype=torch.uint8, device="cuda")
    dec[NB * F:].fill_(SENTINEL)
    o2, st = decode.decode_device(out, oo[:-1], np.diff(oo), dec[:NB * F], key=key, compressed=compressed)
    assert st.tolist() == [0] * NB
    assert o2.tolist() == [F * i for i in range(NB + 1)]
    _equal_each(dec, o2, src_dev, "decode")
    assert bool((dec[NB * F:] == SENTINEL).all())


def test_copy_past_4gib_of_output(source):
    """Encode without key or compression (k_copy)."""
    _need(6 << 30, "68 copies of 64 MiB")
    _, src = source
    out = torch.empty(NB * F, dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(src, [0] * NB, [F] * NB, out, key=None, compress=False)
    assert oo.tolist() == [F * i for i in range(NB + 1)]
    _equal_each(out, oo, src, "copy")


@pytest.fixture(scope="module")
def sealed68(source):
    """The 68 blobs sealed by encode_device: (output tensor, offsets)."""
    _need(11 << 30, "68 sealed blobs of 64 MiB (the output and Encode's frame slots)")
    _, src = source
    out = torch.empty(NB * SEALED + 4096, dtype=torch.uint8, device="cuda")
    out[NB * SEALED:].fill_(SENTINEL)
    oo = encode.encode_device(src, [0] * NB, [F] * NB, out[:NB * SEALED], key=KEY, compress=False, random=_rows(NB, 43))
    return out, oo


def _open_four(out, oo, key, host):
    want = host.tobytes()
    for i in _opened(SEALED):
        blob = out[int(oo[i]):int(oo[i + 1])].cpu().numpy().tobytes()
        assert crypto_ref.decrypt_stream(key, blob)[0] == want, f"blob {i} at {int(oo[i]):#x}"


def test_seal_past_4gib_of_output_and_decode_it(source, sealed68):
    """Encode, key only: the sizes are the arithmetic, four blobs open under
    libcrypto, and decode_device opens all 68 from where they lie."""
    _need(6 << 30, "the plaintext of 68 blobs")
    host, src = source
    out, oo = sealed68
    assert oo.tolist() == [SEALED * i for i in range(NB + 1)]
    assert SEALED == sync.transcode_size(F, False, True)
    assert bool((out[NB * SEALED:] == SENTINEL).all())
    _open_four(out, oo, KEY, host)
    _decode_all(out, oo, src, KEY, False)


@pytest.mark.parametrize("comp", ["LZ4", "GZIP"])
def test_compress_random_bytes_past_4gib_of_output(source, comp):
    """Encode of random bytes: stored blocks, so the output stays above 2^32.
    All 68 frames equal frame 0, which liblz4 / zlib reads; Decode reads all 68."""
    _need(20 << 30, "68 frames of 64 MiB, their plaintext and Encode's workspace")
    host, src = source
    bound = encode.encode_bound(F, _sel(comp), False)
    out = torch.empty(NB * bound, dtype=torch.uint8, device="cuda")
    oo = encode.encode_device(src, [0] * NB, [F] * NB, out, key=None, compress=_sel(comp))
    size = int(oo[1])
    assert F < size <= bound and oo.tolist() == [size * i for i in range(NB + 1)] and int(oo[-1]) > B32
    if comp == "LZ4":
        assert size == LZ4_STORED
    _opened(size)
    frame0 = out[:size]
    _equal_each(out, oo, frame0, comp)
    f0 = frame0.cpu().numpy().tobytes()
    assert (crypto_ref.lz4f_decompress(f0) if comp == "LZ4" else zlib.decompress(f0, 31)) == host.tobytes()
    _decode_all(out, oo, src, None, _sel(comp))


def test_rekey_past_4gib_of_output(source, sealed68):
    """transcode_device, rekey, of the 68 sealed blobs."""
    _need(5 << 30, "68 re-keyed blobs")
    host, _ = source
    out, oo = sealed68
    new = torch.empty(NB * SEALED + 4096, dtype=torch.uint8, device="cuda")
    new[NB * SEALED:].fill_(SENTINEL)
    o2, st = sync.transcode_device(out, oo[:-1], np.diff(oo), new[:NB * SEALED], src=(KEY, None), dst=(KEY_B, None),
                                   random=_rows(NB, 44))
    assert st.tolist() == [0] * NB
    assert o2.tolist() == [sync.transcode_size(SEALED, True, True) * i for i in range(NB + 1)] == oo.tolist()
    assert bool((new[NB * SEALED:] == SENTINEL).all())
    _open_four(new, o2, KEY_B, host)


def test_prefix_decode_past_4gib_of_output(source, sealed68):
    """decode_prefix_device with upto = 64 MiB for every blob: out_offsets is the exclusive sum of upto."""
    _need(5 << 30, "the plaintext of 68 blobs")
    _, src = source
    out, oo = sealed68
    dec = torch.empty(NB * F + 4096, dtype=torch.uint8, device="cuda")
    dec[NB * F:].fill_(SENTINEL)
    o2, st = decode.decode_prefix_device(out, oo[:-1], np.diff(oo), [F] * NB, dec[:NB * F], key=KEY, compressed=False)
    assert st.tolist() == [0] * NB
    assert o2.tolist() == [F * i for i in range(NB + 1)]
    _equal_each(dec, o2, src, "prefix decode")
    assert bool((dec[NB * F:] == SENTINEL).all())
