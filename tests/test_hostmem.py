"""The grow-only device/pinned buffers behind every stage (plakar_amd/csrc/
cdc_hostmem.h) at the smallest sizes that force a second allocation: a small
call, one that makes the per-device cache grow, the small one again -- for
Encode, Decode and the check (device workspace and pinned staging), the
assemble ring (four slots, 1,024-row floor) and the hybrid digests' scratch --
and a process that used all five caches and then exits cleanly."""
import hashlib
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from datagen import random_bytes  # noqa: E402
from plakar_amd import _lib, decode, encode, hashing, restore  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(64, 96))


@pytest.fixture(scope="module", autouse=True)
def _init():
    _lib.ensure_init()


@pytest.fixture(scope="module")
def batches():
    """A (blobs of 0, 100 and 1,000 bytes) and B (40 blobs of 65,537 bytes: one
    byte past the 64-KiB GCM piece), with the random bytes each call gets."""
    big = random_bytes(40 * 65537, 4242)
    a = [b"", random_bytes(100, 1).tobytes(), random_bytes(1000, 2).tobytes()]
    b = [big[i * 65537:(i + 1) * 65537].tobytes() for i in range(40)]
    rnd = {n: random_bytes(encode.RANDOM_BYTES * n, 900 + n).tobytes() for n in (len(a), len(b))}
    return a, b, rnd


@pytest.mark.parametrize("with_key", [False, True])
@pytest.mark.parametrize("compress", [False, "LZ4", "GZIP"])
def test_encode_decode_check_regrow_then_reuse(batches, compress, with_key):
    a, b, rnd = batches
    key = KEY if with_key else None
    encoded = []
    for blobs in (a, b, a):
        enc = encode.encode_blobs(blobs, key=key, compress=compress, random=rnd[len(blobs)] if with_key else None)
        got = decode.decode_blobs(enc, key=key, compressed=compress)
        assert got == blobs
        sums = [hashlib.sha256(x).digest() for x in blobs]
        st = decode.check_blobs(enc, sums, key=key, compressed=compress)
        assert st.tolist() == [0] * len(blobs)
        encoded.append(enc)
    assert encoded[2] == encoded[0]


def test_assemble_ring_wraps_and_regrows():
    """Six calls in a row over the four-slot ring: two slots grow past the
    1,024-row floor, and the fifth and sixth calls take slots again that the
    first two still use."""
    rng = np.random.default_rng(7)
    dev = torch.device("cuda", 0)
    src_np = random_bytes(1 << 16, 78)
    src = torch.from_numpy(src_np).to(dev)
    runs = []
    for nseg in (10, 3000, 10, 3000, 10, 10):
        lens = rng.integers(1, 65, nseg)
        so = rng.integers(0, src_np.size - 64, nseg)
        do = np.cumsum(lens + rng.integers(0, 3, nseg)) - lens  # ascending, small gaps
        size = int(do[-1] + lens[-1]) + 16
        segs = [(int(s), int(n), int(d)) for s, n, d in zip(so, lens, do)]
        want = np.full(size, 0xA5, np.uint8)
        for s, n, d in segs:
            want[d:d + n] = src_np[s:s + n]
        dst = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
        restore.assemble_device(src, segs, dst)  # asynchronous: the calls queue up on the ring
        runs.append((dst, want))
    torch.cuda.synchronize()
    for i, (dst, want) in enumerate(runs):
        assert np.array_equal(dst.cpu().numpy(), want), f"call {i}"


def test_hybrid_digest_scratch_regrows():
    """Cut lists of 8, 4,000 and 8 chunks, every non-empty chunk on the host
    (host_min_len = 1), so each scratch buffer grows with the chunk count."""
    rng = np.random.default_rng(8)
    data = random_bytes(4000 * 4096, 79)
    t = torch.from_numpy(data).cuda()
    for n in (8, 4000, 8):
        lens = rng.integers(0, 4097, n)
        offs = np.arange(n) * 4096 + rng.integers(0, 4096 - lens + 1)
        cuts = torch.tensor(np.stack([offs, lens], 1).astype(np.int64), device="cuda")
        ((d, h),), hc, _ = hashing.chunk_digests_hybrid([t], [cuts], host_threads=4, host_min_len=1)
        torch.cuda.synchronize()
        assert hc == int((lens > 0).sum())
        d, h = d.cpu().numpy(), h.cpu().numpy()
        for i in range(n):
            piece = data[offs[i]:offs[i] + lens[i]]
            assert d[i].tobytes() == hashlib.sha256(piece.tobytes()).digest(), (n, i)
            assert np.array_equal(h[i], np.bincount(piece, minlength=256)), (n, i)


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
# Opening the device is the system's work, not the library's: what the driver
# stack prints while it does (libdrm, about its table of card names) stays out
# of the stderr under test, which is live from the library's initialisation to
# the end of the process.
keep, null = os.dup(2), os.open(os.devnull, os.O_WRONLY)
os.dup2(null, 2)
torch.zeros(1, device="cuda")
torch.cuda.synchronize()
os.dup2(keep, 2)
from plakar_amd import _lib, decode, encode, hashing, restore
def main():
    _lib.ensure_init(gear=_lib.default_gear())  # the table given: no placeholder warning
    key = bytes(range(32))
    blobs = [b"", bytes(range(200)) * 5]
    enc = encode.encode_blobs(blobs, key=key, compress="LZ4")
    assert decode.decode_blobs(enc, key=key, compressed="LZ4") == blobs
    assert decode.check_blobs(enc, [hashlib.sha256(b).digest() for b in blobs], key=key, compressed="LZ4").tolist() == [0, 0]
    src = torch.arange(256, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    restore.assemble_device(src, [(3, 20, 16)], dst)
    cuts = torch.tensor([[0, 100], [100, 156]], dtype=torch.int64, device="cuda")
    ((d, _),), hc, _ = hashing.chunk_digests_hybrid([src], [cuts], host_threads=2, host_min_len=1)
    torch.cuda.synchronize()
    assert hc == 2 and d[0].cpu().numpy().tobytes() == hashlib.sha256(bytes(range(100))).digest()
    assert dst[16:36].cpu().numpy().tolist() == list(range(3, 23))
main()
"""


def test_process_that_used_every_cache_exits_cleanly():
    """The per-device caches hold device memory until the process ends; none of
    it is released from a static destructor (after the runtime may be gone)."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=root)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""
