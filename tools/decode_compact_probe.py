"""Decode's worst case for k_dec_compact: a batch whose FIRST blob fails its
content checksum, so all 256 MiB after it are moved down, against the same
batch with a good first blob:  python tools/decode_compact_probe.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decode_ref as dr  # noqa: E402
from plakar_amd import decode  # noqa: E402

data = dr.rnd(1 << 20, 1)
stored = dr.frame_of_blocks([(True, data)], data)
good, content = dr.fixture_frames()["lz4f-0x64"]
bad = dr.corrupt_frames()["bad-content-checksum"]
for name, first in (("good", good), ("bad", bad)):
    blobs = [first] + [stored] * 256
    lens = np.array([len(b) for b in blobs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    base = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    out = torch.empty(len(content) + 256 * len(data), dtype=torch.uint8, device="cuda")
    best = None
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        oo, st = decode.decode_device(base, offs[:-1], lens, out, compressed=True)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    end = int(oo[-1])
    ok = (bytes(out[int(oo[1]):int(oo[1]) + 64].cpu().numpy()) == data[:64]
          and bytes(out[end - 64:end].cpu().numpy()) == data[-64:])
    print(name, "first status", int(st[0]), "moved MiB", 256, "call ms %.3f" % best, "intact", ok, flush=True)
