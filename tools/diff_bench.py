"""Diff throughput: backup, then diff, of text-like files with 0.1 % of their
lines changed, as 64 pairs and as pairs of 16 KiB, and of one pair of random
bytes (bench.py's C1) with 10 bytes changed; all LZ4 + AES-256-GCM.

    python tools/diff_bench.py [--sets large,small,c1] [--size-mib 256] [--reps 3] [--out profiles/diff_bench.json]

One JSON line per set, every measurement in one process, --reps runs each after
one that grows the buffers; medians and (max - min) / median of the runs:

  * cdc_diff_files: wall seconds, GiB/s of file bytes (both sides), the median
    run's stage seconds, table_s as GiB/s of the file bytes it splits (twice:
    once for the count, once for the records) and emit_s as GiB/s of the text
    it writes, and the stage that bounds the set;
  * the baseline a caller had before: restore_files of both sides, then the Go
    split and Python's difflib on the host, over the first --baseline-mib of
    pairs (difflib is slow: the whole set would take minutes);
  * the second baseline: the same restore and split, ids from a dict, and the
    library's own cdc_diff_script, over the same pairs;
  * the kernels beside a device-to-device copy of the same bytes: the line
    table of the set's a-side, and cdc_diff_emit_device writing every line of
    64 MiB of it with a prefix, against cdc_assemble_device given the same
    records as segments (bodies only: it has no prefix or newline)."""
import argparse
import difflib
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

STAGES = ("read_s", "h2d_s", "decode_s", "verify_s", "assemble_s", "table_s", "ids_s", "match_s", "emit_s", "d2h_s")


def lines_text(np, decode_bench, n):
    """Text-like bytes with a newline for every eighth space: lines of about 50 bytes."""
    a = np.frombuffer(decode_bench.text_like(np, n), dtype=np.uint8).copy()
    sp = np.flatnonzero(a == 32)
    a[sp[7::8]] = 10
    return a


def change_lines(np, a, share, seed):
    """A copy with the first byte of `share` of the lines replaced."""
    rng = np.random.default_rng(seed)
    b = a.copy()
    starts = np.flatnonzero(a == 10) + 1
    starts = starts[starts < a.size]
    pick = rng.choice(starts, size=max(1, int(starts.size * share)), replace=False)
    b[pick] = np.where(a[pick] == 10, 10, ord("Z"))
    return b


def spread(runs):
    m = statistics.median(runs)
    return dict(median=m, spread=(max(runs) - min(runs)) / m if m else 0.0, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="large,small,c1")
    ap.add_argument("--size-mib", type=int, default=256, help="bytes of one side of the large and small sets")
    ap.add_argument("--pairs", type=int, default=64, help="pairs of the large set")
    ap.add_argument("--small-kib", type=int, default=16)
    ap.add_argument("--c1-mib", type=int, default=64)
    ap.add_argument("--baseline-mib", type=int, default=8, help="one side's bytes of the pairs the host baselines take")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import decode_bench
    import diff_ref
    from plakar_amd import _lib, diff, restore, snapshot
    _lib.ensure_init()
    dev = torch.device("cuda", 0)
    key = os.urandom(32)
    out_lines = []
    for name in a.sets.split(","):
        if name == "c1":
            size = a.c1_mib << 20
            da = bench.make_buffers(torch, bench.WORKLOADS["c1"], 0, dev, size)[0].cpu().numpy()
            db = da.copy()
            db[np.linspace(1000, size - 1000, 10).astype(np.int64)] ^= 0x55
            step = size
        else:
            size = a.size_mib << 20
            da = lines_text(np, decode_bench, size)
            db = change_lines(np, da, 0.001, 5)
            step = -(-size // a.pairs) if name == "large" else a.small_kib << 10
        work = tempfile.mkdtemp(prefix="diff_bench_", dir=a.tmp)
        try:
            paths = []
            for i in range(0, size, step):
                for side, d in (("a", da), ("b", db)):
                    p = os.path.join(work, f"{side}{i // step:06d}")
                    d[i:i + step].tofile(p)
                    paths.append(p)
            npairs = len(paths) // 2
            objs, packs, _ = snapshot.backup_files(paths, key=key)
            jobs = [(objs[2 * i], objs[2 * i + 1], f"a/{i}", f"b/{i}") for i in range(npairs)]
            line = dict(set=name, reps=a.reps, pairs=npairs, file_bytes=2 * size, chunks=sum(len(o.Chunks) for o in objs))
            walls, stats = [], []
            with diff.DiffSession(key=key, threads=a.threads) as s:
                for p in packs:
                    s.add_packfile(p)
                for r in range(a.reps + 1):  # the first run grows the buffers
                    res, st = s.run(jobs)
                    assert all(x["status"] == 0 for x in res), [x["status"] for x in res if x["status"]][:3]
                    if r:
                        walls.append(st["wall_s"])
                        stats.append(st)
            for i in (0, npairs // 2, npairs - 1)[:1 if name == "c1" else 3]:  # the text is difflib's
                lo = i * step
                want = diff_ref.expected_diff(da[lo:lo + step].tobytes(), db[lo:lo + step].tobytes(), b"a/%d" % i, b"b/%d" % i)
                assert res[i]["text"] == want, i
            med = stats[sorted(range(len(walls)), key=walls.__getitem__)[len(walls) // 2]]
            line["diff_wall_s"] = spread(walls)
            line["diff_gibs"] = 2 * size / line["diff_wall_s"]["median"] / 2**30
            line.update({k: v for k, v in med.items() if not k.endswith("_s")})
            line["stages_s"] = {k: med[k] for k in STAGES}
            line["stages_s_runs"] = {k: [x[k] for x in stats] for k in STAGES}
            line["bound_by"] = max(STAGES, key=lambda k: med[k])
            line["table_gibs"] = 2 * med["bytes"] / med["table_s"] / 2**30 if med["table_s"] else None
            line["emit_gibs"] = med["out_bytes"] / med["emit_s"] / 2**30 if med["emit_s"] else None
            # ---- the two host baselines over the first pairs
            nb = max(1, min(npairs, (a.baseline_mib << 20) // step))
            sub = [o for j in jobs[:nb] for o in j[:2]]
            t_lib, t_script = [], []
            with restore.RestoreSession(key=key) as s:
                for p in packs:
                    s.add_packfile(p)
                for r in range(a.reps + 1):
                    t0 = time.perf_counter()
                    contents, statuses, _ = s.run(sub)
                    texts = []
                    for i in range(nb):
                        la, lb = diff_ref.split_lines(contents[2 * i]), diff_ref.split_lines(contents[2 * i + 1])
                        texts.append(b"".join(difflib.diff_bytes(difflib.unified_diff, la, lb, b"a/%d" % i, b"b/%d" % i, n=3,
                                                                 lineterm=b"\n")))
                    dt = time.perf_counter() - t0
                    assert not any(statuses) and texts == [x["text"] for x in res[:nb]]
                    if r:
                        t_lib.append(dt)
                    t0 = time.perf_counter()
                    contents, statuses, _ = s.run(sub)
                    nops = 0
                    for i in range(nb):
                        la, lb = diff_ref.split_lines(contents[2 * i]), diff_ref.split_lines(contents[2 * i + 1])
                        ids = diff_ref.first_ids(la + lb)
                        nops += len(diff.diff_ops(ids[:len(la)], ids[len(la):], 3))
                    dt = time.perf_counter() - t0
                    if r:
                        t_script.append(dt)
                del contents
            base_bytes = 2 * min(nb * step, size)
            line.update(baseline_pairs=nb, baseline_bytes=base_bytes, restore_then_difflib_s=spread(t_lib),
                        restore_then_script_s=spread(t_script))
            line["restore_then_difflib_gibs"] = base_bytes / line["restore_then_difflib_s"]["median"] / 2**30
            line["restore_then_script_gibs"] = base_bytes / line["restore_then_script_s"]["median"] / 2**30
            line["diff_over_difflib"] = line["diff_gibs"] / line["restore_then_difflib_gibs"]
            line["diff_over_script"] = line["diff_gibs"] / line["restore_then_script_gibs"]
            # ---- the kernels beside a device-to-device copy
            kb = min(size, 64 << 20)
            src = torch.from_numpy(da[:kb].copy()).to(dev)
            dst = torch.empty_like(src)

            def timed(fn):
                out = []
                for r in range(a.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r:
                        out.append(time.perf_counter() - t0)
                return out

            recs, _ = diff.line_table_device(src, [(0, kb)])
            nl = int(recs.shape[0])
            t_table = timed(lambda: diff.line_table_device(src, [(0, kb)], capacity=nl))
            t_copy = timed(lambda: dst.copy_(src))
            r = recs.cpu().numpy().reshape(-1).view(diff.LINE_DTYPE).reshape(-1)
            plan = np.zeros(nl, dtype=diff.EMIT_DTYPE)
            plan["src_off"], plan["len"], plan["flags"] = r["off"], r["len"], 0x100 | 0x400 | ord("+")
            plan["dst_off"] = np.concatenate([[0], np.cumsum(r["len"].astype(np.uint64) + 2)[:-1]])
            out_bytes = int(r["len"].sum()) + 2 * nl
            big = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
            lit = torch.zeros(16, dtype=torch.uint8, device=dev)
            t_emit = timed(lambda: diff.diff_emit_device(src, lit, plan, big))
            segs = np.stack([plan["src_off"], plan["len"].astype(np.uint64), plan["dst_off"] + 1], axis=1)
            t_asm = timed(lambda: restore.assemble_device(src, segs, big))
            gib = lambda n, runs: n / statistics.median(runs) / 2**30  # noqa: E731
            line["kernels"] = dict(bytes=kb, lines=nl, emit_out_bytes=out_bytes,
                                   table_gibs=gib(kb, t_table), table_s=spread(t_table),
                                   d2d_copy_gibs=gib(kb, t_copy), d2d_copy_s=spread(t_copy),
                                   emit_gibs=gib(out_bytes, t_emit), emit_s=spread(t_emit),
                                   assemble_same_records_gibs=gib(out_bytes - 2 * nl, t_asm), assemble_same_records_s=spread(t_asm))
            del src, dst, big
            print(json.dumps(line), flush=True)
            out_lines.append(line)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(size_mib=a.size_mib, threads=a.threads, sets=out_lines), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
