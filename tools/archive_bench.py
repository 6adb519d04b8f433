"""Archive throughput: backup, then archive as tar and as tarball, of the C1 and
C3 buffers of bench.py cut into files and of the text-like buffer of
tools/decode_bench.py --gzip.

    python tools/archive_bench.py [--sets c1,c3,text] [--size-mib 256] [--file-mib 16] [--reps 3] [--out FILE]
    python tools/archive_bench.py --format zip [--sets c1,c3,text,small] ...

One JSON line per set: GiB/s of tar stream (stream bytes / the pipeline's wall
time, the archive written to --tmp) for `tar` and `tarball` with
cdc_archive_stats (each stage's seconds) and the tar.gz bytes; beside them,
for the same tar bytes, one host thread of zlib.compressobj(6, wbits=31) (the
reference's shape: the whole tar stream through one gzip.NewWriter) with its
size, and restore of the same set in the same process.  --out appends the
lines to a file as well.

--format zip: the same sets and `small` (the text-like buffer as files of
--small-kib KiB: 16,384 files of 16 KiB at the default size) as zip and, in the
same process, as tarball.  One JSON line per set: GiB/s of file bytes for zip
with its stage seconds and the archive's size, tarball beside it, one host
thread of zipfile.ZipFile(..., ZIP_DEFLATED, compresslevel=6) over the same
files (the reference's shape: one compress/flate writer over every file in
turn) with its size, and the deflate stage against a loop of one
GzipStream piece per entry over the same bytes on the device (five launches, a
readback and a synchronise per entry), timed once.

--level 1: tar.gz and zip are written with the wide match search
(cdc_archive_set_level), and level 0 runs beside it in the same process: its
GiB/s and archive size are the *_l0_* figures.  --level 9 (four candidates per
bucket and a lazy parse) runs levels 0 and 1 beside it: *_l0_* and *_l1_*."""
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


def lower_levels(level):
    """The levels that run beside --level in the same process."""
    return {0: (), 1: (0,), 9: (0, 1)}[level]


def zip_sets(a):
    import io
    import zipfile

    import numpy as np
    import torch

    import bench
    import decode_bench
    from plakar_amd import _lib, archive, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    size = a.size_mib << 20
    for name in (a.sets or "c1,c3,text,small").split(","):
        if name in ("text", "small"):
            data = np.frombuffer(decode_bench.text_like(np, size), dtype=np.uint8)
        else:
            data = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0].cpu().numpy()
        work = tempfile.mkdtemp(prefix="archive_bench_", dir=a.tmp)
        try:
            step = a.small_kib << 10 if name == "small" else a.file_mib << 20
            paths = []
            for i in range(0, data.size, step):
                p = os.path.join(work, f"in{i // step:06d}")
                data[i:i + step].tofile(p)
                paths.append(p)
            objs, packs, _ = snapshot.backup_files(paths, key=key)
            ents = [archive.ArchiveEntry(f"set/{os.path.basename(p)}", o, mtime=1_700_000_000) for p, o in zip(paths, objs)]
            line = dict(set=name, reps=a.reps, files=len(paths), file_bytes=int(data.size), level=a.level)
            for fmt in ("zip", "tarball"):
                out = os.path.join(work, "out.zip" if fmt == "zip" else "out.tar.gz")
                for lv in (lower_levels(a.level) + (a.level,)):  # --level's run last: its file is the one read back
                    best = None
                    with (archive.ZipSession(key=key, level=lv) if fmt == "zip"
                          else archive.ArchiveSession(key=key, format=fmt, level=lv)) as s:
                        for p in packs:
                            s.add_packfile(p)
                        for _ in range(a.reps + 1):  # the first run grows the buffers
                            _, statuses, st = s.run(ents, path=out)
                            assert not any(statuses)
                            if best is None or st["wall_s"] < best["wall_s"]:
                                best = st
                    if lv != a.level:  # level 0 beside --level 1: speed and size
                        line.update({f"{fmt}_l{lv}_gibs": data.size / best["wall_s"] / 2**30,
                                     f"{fmt}_l{lv}_output_bytes": best["output_bytes"]})
                        continue
                    line[f"{fmt}_gibs"] = data.size / best["wall_s"] / 2**30
                    line.update({f"{fmt}_{k}": v for k, v in best.items() if k not in ("struct_size", "failed_entry")})
            with zipfile.ZipFile(os.path.join(work, "out.zip")) as z:
                ok = z.testzip() is None and len(z.namelist()) == len(paths)
                for i in sorted({0, len(paths) // 2, len(paths) - 1}):
                    ok = ok and z.read(f"set/{os.path.basename(paths[i])}") == data[i * step:(i + 1) * step].tobytes()
            line["zip_round_trip_ok"] = bool(ok)
            # the deflate stage against one GzipStream piece per entry, over the same bytes on the device
            src = torch.from_numpy(data.copy()).to(dev)
            gz = torch.empty(archive.gzip_stream_bound(step), dtype=torch.uint8, device=dev)
            with archive.GzipStream() as gs:
                gs.piece_device(src, min(step, data.size), gz)  # grows the workspace
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(0, data.size, step):
                    gs.piece_device(src[i:], min(step, data.size - i), gz)
                loop_s = time.perf_counter() - t0
            del src, gz
            line.update(gzip_stream_loop_s=loop_s, loop_over_zip_deflate=loop_s / line["zip_deflate_s"])
            if not a.no_host:
                files = [data[i:i + step].tobytes() for i in range(0, data.size, step)]
                sink = io.BytesIO()
                t0 = time.perf_counter()
                with zipfile.ZipFile(sink, "w", zipfile.ZIP_DEFLATED, compresslevel=6) as z:
                    for p, b in zip(paths, files):
                        z.writestr(f"set/{os.path.basename(p)}", b)
                host_s = time.perf_counter() - t0
                line.update(host_zipfile6_one_thread_s=host_s, host_zipfile6_gibs=data.size / host_s / 2**30,
                            host_zipfile6_bytes=sink.getbuffer().nbytes, zip_over_host=host_s / line["zip_wall_s"])
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(text + "\n")
        finally:
            shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default=None, help="default c1,c3,text; with --format zip c1,c3,text,small")
    ap.add_argument("--format", default="tar", choices=["tar", "zip"], help="tar: tar and tarball; zip: zip beside tarball")
    ap.add_argument("--small-kib", type=int, default=16, help="the file size of the `small` set (--format zip)")
    ap.add_argument("--size-mib", type=int, default=256)
    ap.add_argument("--file-mib", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a temporary one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--level", type=int, default=0, choices=(0, 1, 9),
                    help="the match search of tar.gz and zip (1: a 32-KiB window; 9: and four candidates per bucket, a "
                         "lazy parse); the lower levels are then run beside it (*_l0_*, *_l1_*)")
    a = ap.parse_args()
    if a.format == "zip":
        return zip_sets(a)
    a.sets = a.sets or "c1,c3,text"
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
            line = dict(set=name, reps=a.reps, files=len(paths), level=a.level)
            tar_path = os.path.join(work, "out.tar")
            for fmt in ("tar", "tarball"):
                out = tar_path if fmt == "tar" else os.path.join(work, "out.tar.gz")
                for lv in (lower_levels(a.level) + (a.level,) if fmt == "tarball" else (a.level,)):  # --level's run last
                    best = None
                    with archive.ArchiveSession(key=key, format=fmt, level=lv) as s:
                        for p in packs:
                            s.add_packfile(p)
                        for _ in range(a.reps + 1):  # the first run grows the buffers
                            _, statuses, st = s.run(ents, path=out)
                            assert not any(statuses)
                            if best is None or st["wall_s"] < best["wall_s"]:
                                best = st
                    if lv != a.level:  # level 0 beside --level 1: speed and size
                        line.update({f"{fmt}_l{lv}_gibs": best["stream_bytes"] / best["wall_s"] / 2**30,
                                     f"{fmt}_l{lv}_output_bytes": best["output_bytes"]})
                        continue
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
