"""Contents with planted repeats, for the match searches' tests: plain Python
and numpy, no device.  A content is written front to back as runs, each
either fresh random literals or a copy (position, length, distance) of bytes
already written; the copies are returned beside the content, so a test knows
where a repeat begins, how long it is and how far back its twin lies."""
import numpy as np

EDGES = (1, 2, 3, 63, 64, 65, 8191, 8192, 8193, 32767, 32768, 32769)
RUN_MAX = 12_000        # the longest literal run and the longest copy
DIST_MAX = 40_000       # past the 32,768 any reader allows: such a copy cannot be taken whole
FAR = 8192              # "far": every distance above this (the level-0 window)
AGAIN = 0.4             # a copy follows a copy directly: about one run in four is such a copy


def _log_uniform(rng, lo, hi):
    """An integer of [lo, hi], its logarithm uniform (lo may be 0)."""
    v = int(np.exp(rng.uniform(np.log(lo + 1.0), np.log(hi + 2.0)))) - 1
    return min(max(v, lo), hi)


def planted(n, seed, distances="free"):
    """(content, plants): n bytes and the copies in them, [(pos, length,
    distance)] in ascending pos; deterministic in seed.  Literal runs are
    0..12,000 bytes, copies 4..12,000 (cut at n), both log-uniform, and a
    copy may overlap itself (distance < length).  distances: "free"
    (log-uniform from 1 to 40,000), "edges" (one of EDGES) or "far"
    (log-uniform from 8,193 to 40,000; the first literal run reaches 8,193);
    each clipped to pos."""
    if distances not in ("free", "edges", "far"):
        raise ValueError("distances: free, edges or far")
    rng = np.random.Generator(np.random.PCG64(seed))
    out, plants = bytearray(), []
    after_copy = False
    while len(out) < n:
        pos = len(out)
        copy = pos > 0 and after_copy and rng.random() < AGAIN
        if not copy:
            k = _log_uniform(rng, 0, RUN_MAX)
            if distances == "far":
                k = max(k, FAR + 1 - pos)       # the first copy stands at 8,193 or later
            k = min(k, n - pos)
            out += rng.integers(0, 256, size=k, dtype=np.uint8).tobytes()
            pos = len(out)
            copy = 0 < pos < n
        if distances == "far" and pos <= FAR:
            copy = False
        after_copy = copy
        if not copy:
            continue
        length = min(_log_uniform(rng, 4, RUN_MAX), n - pos)
        if distances == "edges":
            d = int(EDGES[int(rng.integers(0, len(EDGES)))])
        else:
            d = _log_uniform(rng, FAR + 1 if distances == "far" else 1, DIST_MAX)
        d = min(d, pos)
        seg = bytes(out[pos - d:pos - d + length]) if d >= length else (bytes(out[pos - d:]) * (length // d + 1))[:length]
        out += seg
        plants.append((pos, length, d))
    return bytes(out), plants


def replay(content, plants):
    """The content rebuilt from its literals (the bytes outside every plant)
    and the plants, byte by byte as a decoder copies."""
    out, at = bytearray(), 0
    for pos, length, d in plants:
        assert at <= pos and 1 <= d <= pos, (pos, length, d)
        out += content[at:pos]
        for _ in range(length):
            out.append(out[-d])
        at = pos + length
    return bytes(out + content[at:])


def far_share(plants, n):
    """The share of n bytes that lie in copies with a distance above 8,192."""
    return sum(ln for _, ln, d in plants if d > FAR) / max(n, 1)


# ---- the batches of tests/test_encode_wide_planted.py (built here so that the CPU tests see them too) ----
SEG = 8192
BLOCK = 4 << 20
WINDOW_TAILS = (1, 15, 16, 17, 4095, 8191)
WINDOW_LAST = 600
SIZE_CASES = (("far", 1 << 20, 800, "far"), ("free", 1 << 20, 803, "free"))   # name, bytes, seed, distances
BATCH_SEEDS = tuple(range(8))
TILE_BLOBS = 1500


def window_blobs():
    """Sixteen (content, plants), distances far: k * 8192 + r bytes for k in
    1..5 and r of WINDOW_TAILS, every k with three tails or more and every
    tail with two k or more.  The last WINDOW_LAST bytes of each are one more
    copy, from 8,200 + 16 i back (from the first byte where the blob is
    shorter), so that a match runs into the blob's last bytes."""
    out = []
    for i in range(16):
        n = (1 + i % 5) * SEG + WINDOW_TAILS[i % 6]
        content, plants = planted(n - WINDOW_LAST, 600 + i, "far")
        d = min(FAR + 8 + 16 * i, len(content))
        out.append((content + content[-d:][:WINDOW_LAST], plants + [(len(content), WINDOW_LAST, d)]))
    return out


def period(n, rng):
    p = rng.integers(0, 256, size=int(rng.integers(1, 300)), dtype=np.uint8).tobytes()
    return (p * (n // len(p) + 1))[:n]


def _kind(kind, n, seed, rng):
    import inflate_ref as ir
    if kind == 0:
        return planted(n, seed, ("free", "edges", "far")[seed % 3])
    return (period(n, rng) if kind == 1 else ir.text(n, seed) if kind == 2 else ir.rnd(n, seed)), []


def seeded_batch(seed):
    """[(content, plants)] of one seed: 1-120 blobs of 0-300,000 bytes
    (log-uniform; one in five at 8,192, 32,768 or 65,536 +- 2), planted, text,
    a short random period repeated or random, and one blob of 4 MiB +
    U(0, 40,000) at a random place (its kind: seed % 4, in that order)."""
    rng = np.random.Generator(np.random.PCG64(7320 + seed))
    count = int(rng.integers(1, 121))
    big_at = int(rng.integers(0, count))
    out = []
    for i in range(count):
        if i == big_at:
            out.append(_kind(seed % 4, BLOCK + int(rng.integers(0, 40001)), 7400 + 128 * seed + i, rng))
            continue
        n = int(rng.choice([SEG, 32768, 65536])) + int(rng.integers(-2, 3)) if rng.random() < 0.2 \
            else _log_uniform(rng, 0, 300_000)
        out.append(_kind(int(rng.integers(0, 4)), n, 7400 + 128 * seed + i, rng))
    return out


def tile_blobs():
    """1,500 (content, plants) of 9,000-20,000 planted bytes: more blobs than
    one call's first tile of 1,024, every one with a second or third segment."""
    rng = np.random.Generator(np.random.PCG64(7700))
    return [planted(int(rng.integers(9000, 20001)), 7800 + i, ("free", "edges", "far")[i % 3]) for i in range(TILE_BLOBS)]
