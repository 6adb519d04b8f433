"""cdc_diff_emit_device against a Python executor of the same records
(diff_ref.execute): every byte of the destination compared, the bytes before,
between and after the records included.  A record under 2 KiB is one of up to
64 in a wave's unit (at most 8 KiB of output); a longer one goes in 16-KiB
pieces of 16-byte stores."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import diff_ref  # noqa: E402
from plakar_amd import _lib, diff  # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN_LEN = (2 << 20) + 77
LIT_LEN = 5000
FILL = 0xEE
P, L, N = diff_ref.PREFIX, diff_ref.LITERAL, diff_ref.NEWLINE


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(21)
    plain = rng.integers(0, 256, PLAIN_LEN, dtype=np.uint8)
    lit = rng.integers(0, 256, LIT_LEN, dtype=np.uint8)
    dev = torch.device("cuda", 0)
    return plain.tobytes(), lit.tobytes(), torch.from_numpy(plain).to(dev), torch.from_numpy(lit).to(dev)


def _records(specs, start=0, gaps=None):
    """specs: (len, flags, literal?) in output order; destinations back to
    back from `start`, gaps[i] bytes left out before record i."""
    rng = np.random.default_rng(len(specs))
    recs = np.zeros(len(specs), dtype=diff.EMIT_DTYPE)
    d = start
    for i, (ln, flags) in enumerate(specs):
        d += gaps[i] if gaps else 0
        cap = LIT_LEN if flags & L else PLAIN_LEN
        recs[i] = (int(rng.integers(0, cap - ln + 1)), d, ln, flags)
        d += ln + bool(flags & P) + bool(flags & N)
    return recs, d


def _check(sources, recs, end, margin=64):
    plain, lit, dplain, dlit = sources
    size = end + margin
    dst = torch.full((size,), FILL, dtype=torch.uint8, device=dplain.device)
    diff.diff_emit_device(dplain, dlit, recs, dst)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().tobytes()
    want = bytes(diff_ref.execute(recs, plain, lit, size, FILL))
    if got != want:
        at = next(i for i in range(size) if got[i] != want[i])
        rec = max((i for i in range(len(recs)) if int(recs[i]["dst_off"]) <= at), default=-1)
        raise AssertionError(f"byte {at} is {got[at]:#x}, not {want[at]:#x} (record {rec}: {recs[rec] if rec >= 0 else None})")


LENS = [0, 1, 15, 16, 17, 2047, 2048, 2049, 4097, 16384, 16385, 1 << 20]


@pytest.mark.parametrize("flags", [P | N | ord("+"), 0, L, P | ord("-"), N, L | P | N | ord(" ")])
def test_one_record_of_every_length_at_every_residue(sources, flags):
    """Each length alone, its destination at every residue mod 16 (the
    destination tensor is 256-byte aligned)."""
    for ln in LENS:
        if flags & L and ln > LIT_LEN:
            continue
        for res in (range(16) if ln < 20000 else (0, 1, 15)):
            recs, end = _records([(ln, flags)], start=32 + res)
            _check(sources, recs, end)


def test_lengths_interleaved_prefixed_and_literal(sources):
    specs = []
    for rep in range(3):
        for ln in LENS:
            specs.append((ln, P | N | ord("-+ "[rep])))
            specs.append((min(ln, 300), L))
            specs.append((ln, N if rep else 0))
    recs, end = _records(specs, start=5)
    _check(sources, recs, end)
    rng = np.random.default_rng(9)
    gaps = [int(g) for g in rng.integers(0, 40, len(specs))]
    recs, end = _records(specs, start=0, gaps=gaps)
    _check(sources, recs, end)


@pytest.mark.parametrize("n", [1, 64, 65, 10_000])
def test_many_short_records(sources, n):
    """n records of 0-120 bytes, a literal every tenth: units of 64 records
    and units that 8 KiB of output close."""
    rng = np.random.default_rng(n)
    specs = []
    for i in range(n):
        if i % 10 == 9:
            specs.append((int(rng.integers(0, 40)), L))
        else:
            specs.append((int(rng.integers(0, 121)), P | N | int(rng.choice([32, 43, 45]))))
    recs, end = _records(specs, start=int(rng.integers(0, 16)))
    _check(sources, recs, end)
    # long lines between short ones: a unit closes before each and opens after
    specs = [(int(rng.integers(1500, 2600)) if i % 5 == 0 else s[0], s[1] & ~L) for i, s in enumerate(specs[:200])]
    recs, end = _records(specs, start=3)
    _check(sources, recs, end)


def test_nothing_to_write_and_rejections(sources):
    plain, lit, dplain, dlit = sources
    dst = torch.full((256,), FILL, dtype=torch.uint8, device=dplain.device)
    diff.diff_emit_device(dplain, dlit, np.zeros(0, dtype=diff.EMIT_DTYPE), dst)
    recs, _ = _records([(0, 0), (0, L)], start=10)
    diff.diff_emit_device(dplain, dlit, recs, dst)
    recs, _ = _records([(100, P | N | 43), (100, N)], start=10)
    recs[1]["dst_off"] -= 1  # overlaps
    with pytest.raises(_lib.CdcError) as e:
        diff.diff_emit_device(dplain, dlit, recs, dst)
    assert e.value.status == _lib.CDC_E_INVALID
    recs, _ = _records([(100, P | N | 43), (100, N)], start=56)  # one byte past the end
    with pytest.raises(_lib.CdcError) as e:
        diff.diff_emit_device(dplain, dlit, recs, dst)
    assert e.value.status == _lib.CDC_E_INVALID
    with pytest.raises(_lib.CdcError) as e:  # the destination inside the plaintext
        diff.diff_emit_device(dplain, dlit, _records([(10, 0)])[0], dplain[1000:2000])
    assert e.value.status == _lib.CDC_E_INVALID
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())
