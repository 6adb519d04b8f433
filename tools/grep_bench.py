"""Grep throughput: backup, then grep, of 256 MiB of random bytes (bench.py's
C1), of zeros with 1 % random bytes (C3) and of text-like lines as 64 files,
and of text-like lines as files of 16 KiB; LZ4 + AES-256-GCM, and GZIP.

    python tools/grep_bench.py [--sets c1,c3,text,small] [--codecs LZ4,GZIP] [--size-mib 256] [--reps 3]
                               [--out profiles/grep_bench.json]

One JSON line per set, codec and query, every measurement in one process,
--reps runs each after one that grows the buffers; medians and (max - min) /
median of the runs:

  * GrepSession.run: wall seconds, GiB/s of file bytes, the median run's stage
    seconds and the stage that bounds it;
  * what a caller had before, alternated with it: restore_files, then
    bytes.find per pattern over every file on --threads host threads.

Queries: one 8-byte string planted 1,000 times; 32 strings (the planted one
and 31 that do not occur); one frequent single byte, so that nearly every
line matches; and, as a set of its own ("worst"), 4 MiB of one byte value
against 32 patterns of 256 such bytes.

Then the device calls alone over 1 GiB of resident text, hipEvents around
each: cdc_grep_device for each query, cdc_line_table_device, and a
device-to-device copy of the same bytes."""
import argparse
import concurrent.futures
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

STAGES = ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "table_s", "scan_s", "compact_s", "emit_s", "d2h_s")
PLANTED = b"Qx7#Zk9!"


def spread(runs):
    m = statistics.median(runs)
    return dict(median=m, spread=(max(runs) - min(runs)) / m if m else 0.0, runs=runs)


def queries():
    others = [b"%s-%02d" % (PLANTED[::-1], k) for k in range(31)]
    return {"planted": [PLANTED], "32 strings": [PLANTED] + others, "frequent byte": [b"e"]}


def plant(np, a, count, seed):
    rng = np.random.default_rng(seed)
    for at in rng.choice(a.size - 16, size=count, replace=False):
        a[at:at + len(PLANTED)] = np.frombuffer(PLANTED, dtype=np.uint8)
    return a


def host_find(contents, patterns, threads):
    def one(b):
        n = 0
        for p in patterns:
            i = b.find(p)
            while i >= 0:
                n += 1
                i = b.find(p, i + 1)
        return n
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        return sum(ex.map(one, contents))


def timed_ms(torch, fn, reps):
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="c1,c3,text,small,worst")
    ap.add_argument("--codecs", default="LZ4,GZIP")
    ap.add_argument("--size-mib", type=int, default=256)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--small-kib", type=int, default=16)
    ap.add_argument("--resident-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grep_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import decode_bench
    from diff_bench import lines_text
    from plakar_amd import _lib, diff, grep, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    out_lines = []
    for name in a.sets.split(","):
        size = (4 << 20) if name == "worst" else a.size_mib << 20
        if name in ("c1", "c3"):
            data = bench.make_buffers(torch, bench.WORKLOADS[name], 0, dev, size)[0].cpu().numpy().copy()
        elif name == "worst":
            data = np.full(size, ord("a"), dtype=np.uint8)
        else:
            data = lines_text(np, decode_bench, size)
        if name != "worst":
            plant(np, data, 1000, 7)
        step = a.small_kib << 10 if name == "small" else -(-size // (1 if name == "worst" else a.files))
        qs = {"one byte value": [b"a" * 256] * 32} if name == "worst" else queries()
        for codec in a.codecs.split(","):
            comp, k = (codec, key)
            work = tempfile.mkdtemp(prefix="grep_bench_", dir=a.tmp)
            try:
                paths = []
                for i in range(0, size, step):
                    p = os.path.join(work, f"f{i // step:06d}")
                    data[i:i + step].tofile(p)
                    paths.append(p)
                objs, packs, _ = snapshot.backup_files(paths, key=k, compression=comp)
                with grep.GrepSession(key=k, compression=comp, threads=a.threads) as s:
                    for p in packs:
                        s.add_packfile(p)
                    for qname, pats in qs.items():
                        line = dict(set=name, codec=codec, query=qname, reps=a.reps, files=len(paths), file_bytes=size,
                                    patterns=len(pats))
                        walls, stats, base = [], [], []
                        for r in range(a.reps + 1):  # the first run grows the buffers
                            res, st = s.run(objs, pats)
                            assert all(x["status"] == 0 for x in res)
                            t0 = time.perf_counter()
                            contents, statuses, _ = snapshot.restore_files(objs, packs, key=k, compression=comp)
                            t1 = time.perf_counter()
                            found = host_find(contents, pats, a.threads)
                            t2 = time.perf_counter()
                            assert found == sum(int(x["hits"]["nocc"].astype(np.uint64).sum()) for x in res) or \
                                any(x["matched"] > len(x["hits"]) for x in res), (found, qname)
                            del contents
                            if r:
                                walls.append(st["wall_s"])
                                stats.append(st)
                                base.append((t2 - t0, t1 - t0, t2 - t1))
                        med = stats[sorted(range(len(walls)), key=walls.__getitem__)[len(walls) // 2]]
                        line["grep_wall_s"] = spread(walls)
                        line["grep_gibs"] = size / line["grep_wall_s"]["median"] / 2**30
                        line.update({kk: v for kk, v in med.items() if not kk.endswith("_s")})
                        line["stages_s"] = {kk: med[kk] for kk in STAGES}
                        line["bound_by"] = max(STAGES, key=lambda kk: med[kk])
                        line["restore_then_find_s"] = spread([b[0] for b in base])
                        line["restore_s"] = spread([b[1] for b in base])
                        line["find_s"] = spread([b[2] for b in base])
                        line["times_sooner"] = line["restore_then_find_s"]["median"] / line["grep_wall_s"]["median"]
                        print(json.dumps(line), flush=True)
                        out_lines.append(line)
            finally:
                shutil.rmtree(work, ignore_errors=True)
    # ---- the device calls alone
    n = a.resident_mib << 20
    text = torch.from_numpy(plant(np, lines_text(np, decode_bench, n), 1000, 9)).to(dev)
    other = torch.empty_like(text)
    texts = [(i, min(n // 64, n - i)) for i in range(0, n, n // 64)]
    dev_line = dict(set="resident text", bytes=n, texts=len(texts), reps=a.reps)
    for qname, pats in queries().items():
        hits, lines, matched, _ = grep.grep_device(text, texts, pats)
        ms = timed_ms(torch, lambda: grep.grep_device(text, texts, pats, capacity=len(hits)), a.reps)
        dev_line[qname] = dict(ms=spread(ms), gibs=n / statistics.median(ms) * 1e3 / 2**30, hits=int(len(hits)),
                               lines=int(lines.sum()))
    ms = timed_ms(torch, lambda: other.copy_(text), a.reps)
    dev_line["d2d_copy"] = dict(ms=spread(ms), gibs=n / statistics.median(ms) * 1e3 / 2**30)
    recs, _ = diff.line_table_device(text, texts)
    ms = timed_ms(torch, lambda: diff.line_table_device(text, texts, capacity=recs.shape[0]), a.reps)
    dev_line["line_table"] = dict(ms=spread(ms), gibs=n / statistics.median(ms) * 1e3 / 2**30)
    print(json.dumps(dev_line), flush=True)
    out_lines.append(dev_line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(size_mib=a.size_mib, threads=a.threads, lines=out_lines), f, indent=1)


if __name__ == "__main__":
    main()
