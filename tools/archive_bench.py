"""Archive throughput: backup, then archive as tar and as tarball, of the C1 and
C3 buffers of bench.py cut into files and of the text-like buffer of
tools/decode_bench.py --gzip.

    python tools/archive_bench.py [--sets c1,c3,text] [--size-mib 256] [--file-mib 16] [--reps 3] [--out FILE]

One JSON line per set: GiB/s of tar stream (stream bytes / the pipeline's wall
time, the archive written to --tmp) for `tar` and `tarball` with
cdc_archive_stats (each stage's seconds) and the tar.gz bytes; beside them,
for the same tar bytes, one host thread of zlib.compressobj(6, wbits=31) (the
reference's shape: the whole tar stream through one gzip.NewWriter) with its
size, and restore of the same set in the same process.  --out appends the
lines to a file as well."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,text")
    ap.add_argument("--size-mib", type=int, default=256)
    ap.add_argument("--file-mib", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a temporary one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import decode_bench
    from plakar_amd import _lib, archive, restore, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    size = a.size_mib << 20
    for name in a.sets.split(","):
        if name == "text":
            data = np.frombuffer(decode_bench.text_like(np, size), dtype=np.uint8)
        else:
            data = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0].cpu().numpy()
        work = tempfile.mkdtemp(prefix="archive_bench_", dir=a.tmp)
        try:
            step = a.file_mib << 20
            paths = []
            for i in range(0, data.size, step):
                p = os.path.join(work, f"in{i // step:04d}")
                data[i:i + step].tofile(p)
                paths.append(p)
            objs, packs, _ = snapshot.backup_files(paths, key=key)
            ents = [archive.ArchiveEntry(f"set/{os.path.basename(p)}", o, mtime=1_700_000_000) for p, o in zip(paths, objs)]
            line = dict(set=name, reps=a.reps, files=len(paths))
            tar_path = os.path.join(work, "out.tar")
            for fmt in ("tar", "tarball"):
                out = tar_path if fmt == "tar" else os.path.join(work, "out.tar.gz")
                best = None
                with archive.ArchiveSession(key=key, format=fmt) as s:
                    for p in packs:
                        s.add_packfile(p)
                    for _ in range(a.reps + 1):  # the first run grows the buffers
                        _, statuses, st = s.run(ents, path=out)
                        assert not any(statuses)
                        if best is None or st["wall_s"] < best["wall_s"]:
                            best = st
                line[f"{fmt}_gibs"] = best["stream_bytes"] / best["wall_s"] / 2**30
                line.update({f"{fmt}_{k}": v for k, v in best.items() if k not in ("struct_size", "failed_entry")})
            with open(tar_path, "rb") as f:
                tar = f.read()
            with open(os.path.join(work, "out.tar.gz"), "rb") as f:
                line["tarball_round_trip_ok"] = zlib.decompress(f.read(), 31) == tar
            if not a.no_host:
                t0 = time.perf_counter()
                z = zlib.compressobj(6, wbits=31)
                n = 0
                for i in range(0, len(tar), 1 << 20):
                    n += len(z.compress(tar[i:i + (1 << 20)]))
                n += len(z.flush())
                host_s = time.perf_counter() - t0
                line.update(host_zlib6_one_thread_s=host_s, host_zlib6_gibs=len(tar) / host_s / 2**30, host_zlib6_bytes=n,
                            tarball_over_host=host_s / line["tarball_wall_s"])
            del tar
            dests = [os.path.join(work, f"out{i:05d}") for i in range(len(paths))]
            best = None
            with restore.RestoreSession(key=key) as s:
                for p in packs:
                    s.add_packfile(p)
                for _ in range(a.reps + 1):
                    _, statuses, st = s.run(objs, dests)
                    assert not any(statuses)
                    if best is None or st["wall_s"] < best["wall_s"]:
                        best = st
            line.update(restore_gibs=best["bytes"] / best["wall_s"] / 2**30, restore_wall_s=best["wall_s"])
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(text + "\n")
        finally:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
