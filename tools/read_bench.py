"""Ranged reads (cdc_restore_ranges) beside what a caller had before them:
restore_files of the touched files and a slice on the host.

The sets are restore_bench.py's: C1 and C3 (bench.py's buffers) and
decode_bench.py's text-like bytes, each cut into 64 files, backed up with LZ4
(or --gzip) and AES-256-GCM.  Three cases, in one process and on one session:
  first4k  the first 4 KiB of every file;
  random   10,000 seeded random 64-KiB ranges;
  whole    every file as one whole-file range.
Each case runs --reps times as ranges and --reps times as restore_files +
slices, interleaved, after one warm-up run of each (the first run grows the
buffers); the window is the wall clock around the whole call, bytes on the
host at its end.  One JSON line per set: per case the walls of every run,
their medians and the ratio, the stage times and the work counters of the
median ranged run.

    python tools/read_bench.py [--gzip] [--sets c1,c3,text] [--size-mib 1024] [--reps 3]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FILES = 64
COUNTERS = ("batches", "segments", "distinct_blobs", "whole_blobs", "prefix_blobs", "verified_blobs", "encoded_bytes",
            "decoded_bytes", "skipped_bytes", "bytes")
STAGES = ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "d2h_s", "wall_s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,text")
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ranges", type=int, default=10_000)
    ap.add_argument("--gzip", action="store_true")
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a temporary one)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import decode_bench
    from plakar_amd import _lib, restore, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    compression = "GZIP" if a.gzip else "LZ4"
    size = a.size_mib << 20
    for name in a.sets.split(","):
        if name == "text":
            data = np.frombuffer(decode_bench.text_like(np, size), dtype=np.uint8)
        else:
            data = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0].cpu().numpy()
        work = tempfile.mkdtemp(prefix="read_bench_", dir=a.tmp)
        try:
            step = size // FILES
            paths = []
            for i in range(FILES):
                p = os.path.join(work, f"in{i:04d}")
                data[i * step:(i + 1) * step].tofile(p)
                paths.append(p)
            objs, packs, _ = snapshot.backup_files(paths, key=key, compression=compression)
            rng = np.random.default_rng(11)
            cases = {
                "first4k": [(i, 0, 4096) for i in range(FILES)],
                "random": [(int(f), int(o), 65536) for f, o in zip(rng.integers(0, FILES, a.ranges),
                                                                    rng.integers(0, step - 65536, a.ranges))],
                "whole": [(i, 0, step) for i in range(FILES)],
            }
            line = dict(set=name, compression=compression, files=FILES, file_bytes=step, reps=a.reps)
            with restore.RestoreSession(key=key, compression=compression) as s:
                for p in packs:
                    s.add_packfile(p)
                for case, ranges in cases.items():
                    touched = sorted({r[0] for r in ranges})
                    where = {f: k for k, f in enumerate(touched)}
                    sub = [objs[f] for f in touched]

                    def ranged():
                        t0 = time.perf_counter()
                        contents, statuses, st = s.read_ranges(objs, ranges)
                        wall = time.perf_counter() - t0
                        assert not any(statuses)
                        return wall, st, contents

                    def before():
                        t0 = time.perf_counter()
                        contents, statuses, st = s.run(sub)
                        got = [contents[where[f]][o:o + n] for f, o, n in ranges]
                        wall = time.perf_counter() - t0
                        assert not any(statuses)
                        return wall, st, got

                    _, _, got_r = ranged()   # warm-up of each, and the two against each other
                    _, _, got_b = before()
                    ok = got_r == got_b and all(
                        g == data[f * step + o:f * step + o + n].tobytes() for (f, o, n), g in list(zip(ranges, got_r))[::97])
                    del got_r, got_b
                    runs_r, runs_b = [], []
                    for _ in range(a.reps):
                        w, st, _ = ranged()
                        runs_r.append((w, st))
                        w, st, _ = before()
                        runs_b.append((w, st))
                    med_r = sorted(runs_r, key=lambda x: x[0])[len(runs_r) // 2]
                    med_b = sorted(runs_b, key=lambda x: x[0])[len(runs_b) // 2]
                    line[case] = dict(
                        ranges=len(ranges), equal=ok,
                        ranged_wall_s=[round(w, 6) for w, _ in runs_r], before_wall_s=[round(w, 6) for w, _ in runs_b],
                        ranged_median_s=statistics.median(w for w, _ in runs_r),
                        before_median_s=statistics.median(w for w, _ in runs_b),
                        before_over_ranged=statistics.median(w for w, _ in runs_b) / statistics.median(w for w, _ in runs_r),
                        ranged={k: med_r[1][k] for k in COUNTERS + STAGES},
                        before={k: med_b[1][k] for k in ("batches", "decoded_blobs", "encoded_bytes", "decoded_bytes", "bytes",
                                                         "read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "d2h_s",
                                                         "write_s", "wall_s")})
            print(json.dumps(line), flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
