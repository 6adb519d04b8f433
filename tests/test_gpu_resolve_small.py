"""k_resolve at its structural edges, bit-exact against the CPU oracle.

The sweep's smallest parameters (min 64 / normal 256 / max 1024) make a
resolution segment 1,024 bytes, so buffers of a few hundred KiB reach every
edge of the resolver: the four-wave workgroup that shares one launch
(1 - 5 segments), the 64-segment look-back window (63 - 65), the eight
windows one look-back round trip reads (511 - 513, 577) and a second round
trip (1025); launch groups whose workgroups straddle buffers; and the ticket
and status words reused by launch after launch on two streams.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from datagen import gear_table, low_entropy, random_bytes  # noqa: E402
from plakar_amd import _lib, device  # noqa: E402
from test_gpu_parity import _opts, assert_same, gpu_chunk  # noqa: E402

pytestmark = pytest.mark.gpu

P = dict(min_size=64, normal_size=256, max_size=1024)
SEG = 1024  # 16 * min_size (make_plan)
NSEGS = [1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 577, 1025]
KINDS = ["random", "low_entropy", "zeros"]
GEAR = gear_table(31)


@pytest.fixture(autouse=True)
def _restore_library_state():
    device.set_debug_mode(0)
    yield
    device.set_debug_mode(0)
    _lib.ensure_init(gear=_lib.default_gear())


@functools.lru_cache(maxsize=None)
def _pool(kind):
    """One read-only array per kind; every buffer of the tests is a slice of it."""
    n = (max(NSEGS) + 70) * SEG
    a = random_bytes(n, 301) if kind == "random" else low_entropy(n, 302, 0.01) if kind == "low_entropy" \
        else np.zeros(n, np.uint8)
    a.setflags(write=False)
    return a


def _buf(kind, nbytes, start=0):
    return _pool(kind)[start:start + nbytes]


@functools.lru_cache(maxsize=None)
def _ref_cached(kind, nbytes, start, cut_adj):
    from oracle_ref import Oracle
    r = Oracle().chunk(_buf(kind, nbytes, start), GEAR, cut_adj=cut_adj, **P)
    r.setflags(write=False)
    return r


def _ref(kind, nbytes, start=0, cut_adj=0):
    return _ref_cached(kind, nbytes, start, cut_adj)


@pytest.mark.parametrize("cut_adj", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nseg", NSEGS)
def test_single_buffer_of_n_segments(nseg, kind, cut_adj):
    for nbytes in (nseg * SEG, nseg * SEG - 7):
        (got,), _ = gpu_chunk([_buf(kind, nbytes)], P, gear=GEAR, cut_adj=cut_adj)
        assert_same(got, _ref(kind, nbytes, 0, cut_adj), f"{kind} {nbytes} B ({nseg} segments) cut_adj {cut_adj}")


def _group_case(segs):
    """Buffers of the given segment counts: kinds rotate, every other non-empty one is 7 bytes short."""
    out = []
    for i, s in enumerate(segs):
        nbytes = s * SEG - (7 if s and i % 2 else 0)
        out.append((KINDS[i % 3], nbytes, (i % 5) * SEG))
    return out


GROUPS = {
    "five_1_0_3_6_65": [1, 0, 3, 6, 65],       # 75 segments: the last workgroup holds three
    "32_of_1_to_3": ([1, 2, 3] * 11)[:32],     # kMaxBufsPerLaunch buffers, 63 segments
}


@pytest.mark.parametrize("cut_adj", [0, 1])
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_launch_group_straddles_buffers(name, cut_adj):
    segs = GROUPS[name]
    assert sum(segs) % 4 != 0 and len(segs) <= 32
    case = _group_case(segs)
    got, _ = gpu_chunk([_buf(*c) for c in case], P, gear=GEAR, cut_adj=cut_adj)
    for i, c in enumerate(case):
        assert_same(got[i], _ref(*c, cut_adj), f"{name} buffer {i} ({c[1]} B)")


def test_two_batches_two_streams_reuse_their_words():
    """Two DeviceBatches alternate on two streams, eight launches each, over the
    65- and 513-segment shapes; the outputs are cleared before every launch and
    every pass's cut lists are checked."""
    _lib.ensure_init(gear=GEAR, cut_convention=0)
    shapes = [[("random", 65 * SEG, 0), ("low_entropy", 513 * SEG - 7, SEG)],
              [("random", 513 * SEG, 2 * SEG), ("zeros", 65 * SEG - 7, 0)]]
    batches = []
    for sh in shapes:
        ts = [torch.from_numpy(np.ascontiguousarray(_buf(*c))).cuda() for c in sh]
        batches.append(device.DeviceBatch(ts, _opts(P)))
    streams = [torch.cuda.Stream() for _ in batches]
    torch.cuda.synchronize()
    for rep in range(8):
        for b, s in zip(batches, streams):
            with torch.cuda.stream(s):
                for c in b.cuts:
                    c.zero_()
                b.res.zero_()
            b.launch(s)
        for k, (b, sh) in enumerate(zip(batches, shapes)):
            cuts, _ = b.results()
            for i, c in enumerate(sh):
                assert_same(cuts[i].cpu().numpy().astype(np.uint64), _ref(*c, 0), f"pass {rep} batch {k} buffer {i}")


def test_sequential_rewrite_on_65_segments():
    """Debug mode 1: the buffer's last segment rewrites the cut list by the sequential walk."""
    device.set_debug_mode(1)
    nbytes = 65 * SEG - 7
    (got,), _ = gpu_chunk([_buf("random", nbytes)], P, gear=GEAR)
    assert_same(got, _ref("random", nbytes), "debug mode 1")
