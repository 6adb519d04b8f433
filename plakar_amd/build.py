"""Build libplakar_cdc.so (HIP, gfx950) in-tree and the CPU oracle (test infrastructure).

    python -m plakar_amd.build            # both
    python -m plakar_amd.build --lib-only

hipcc cross-compiles for gfx950 without a GPU, so this runs in the build
container; the built .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_DIR = os.path.join(HERE, "_lib")
LIB = os.path.join(LIB_DIR, "libplakar_cdc.so")
SOURCES = [os.path.join(HERE, "csrc", f) for f in ("cdc_kernels.hip", "cdc_digest.hip", "cdc_api.cpp",
                                                    "cdc_packer.cpp", "cdc_collector.cpp",
                                                    "cdc_encode.hip", "cdc_zip.hip", "cdc_decode.hip", "cdc_sha256.cpp",
                                                    "cdc_backup.cpp",
                                                    "cdc_restore.hip", "cdc_restore.cpp", "cdc_transcode.hip",
                                                    "cdc_archive.cpp", "cdc_check.cpp", "cdc_diff.hip", "cdc_diff.cpp",
                                                    "cdc_sync.cpp", "cdc_stored.cpp", "cdc_state.hip", "cdc_state.cpp",
                                                    "cdc_grep.hip", "cdc_grep.cpp", "cdc_blobsrc.cpp", "cdc_reader.cpp")]
HEADERS = [os.path.join(HERE, "csrc", f) for f in ("cdc_internal.h", "cdc_hostmem.h", "cdc_crypto_dev.h", "lz4_walk.h",
                                                   "inflate_walk.h", "deflate_enc.h", "cdc_encode_dev.h", "restore_plan.h", "read_plan.h",
                                                   "transcode_plan.h", "archive_plan.h", "zip_plan.h", "cdc_locator.h", "check_plan.h",
                                                   "sha_blocks.h", "hybrid_model.h", "diff_plan.h", "sync_plan.h", "stored_plan.h", "cdc_stored.h",
                                                   "state_plan.h", "cdc_state.h", "sweep_plan.h", "grep_plan.h", "cdc_hostutil.h", "cdc_blobsrc.h",
                                                   "cdc_reader.h")] + \
          [os.path.join(ROOT, "include", "plakar_cdc.h")]
ARCH = os.environ.get("PLAKAR_CDC_ARCH", "gfx950")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def resources_path(lib=None):
    """The compiler's per-kernel resource remarks of a built library."""
    return os.path.splitext(lib or LIB)[0] + ".resources.txt"


def build_lib(force=False, verbose=True, out=None, defines=()):
    """Build the library (out: another path for an experiment variant,
    defines: extra -D flags for it).

    The compiler's kernel-resource-usage remarks (registers, spills and
    private-segment bytes of every kernel) are kept next to the library in
    resources_path(); tests/test_kernel_resources.py holds k_resolve and
    k_scan to their private-segment bounds with them."""
    target = out or LIB
    remarks = resources_path(target)
    if not force and not defines and not _stale(target, SOURCES + HEADERS) and os.path.exists(remarks):
        return target
    os.makedirs(os.path.dirname(target), exist_ok=True)
    tmp = target + ".tmp"
    cmd = ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function",
           "-Rpass-analysis=kernel-resource-usage",
           "-o", tmp] + [f"-D{d}" for d in defines] + SOURCES
    if verbose:
        print("[plakar_amd.build]", " ".join(cmd), flush=True)
    # the remarks come on stderr, between any warnings: the remark lines go to
    # the file, everything else is passed on
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    kept = [ln for ln in r.stderr.splitlines(True) if "[-Rpass-analysis=kernel-resource-usage]" in ln]
    sys.stderr.write("".join(ln for ln in r.stderr.splitlines(True)
                             if "[-Rpass-analysis=kernel-resource-usage]" not in ln))
    if r.returncode:
        raise subprocess.CalledProcessError(r.returncode, cmd)
    with open(remarks + ".tmp", "w") as f:
        f.writelines(kept)
    os.replace(remarks + ".tmp", remarks)
    os.replace(tmp, target)
    return target


def build_oracle(verbose=True):
    """Compile oracle/ (CPU checker; never linked into the product)."""
    cmd = ["make", "-s", "-C", os.path.join(ROOT, "oracle")]
    if verbose:
        print("[plakar_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return os.path.join(ROOT, "oracle", "_build", "liboracle.so")


def build_ctests(verbose=True):
    """Compile the C-level boundary test (tests/c/abi_threads.c) against the
    library and the CPU oracle (its checker) into tests/_build/."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "abi_threads")
    src = [os.path.join(ROOT, "tests", "c", "abi_threads.c"), os.path.join(ROOT, "oracle", "fastcdc_oracle.c")]
    if not _stale(exe, src + [LIB] + HEADERS):
        return exe
    cmd = ["gcc", "-O2", "-std=gnu11", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe] + src + \
          ["-L", LIB_DIR, "-lplakar_cdc", "-Wl,-rpath,$ORIGIN/../../plakar_amd/_lib", "-lpthread"]
    if verbose:
        print("[plakar_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return exe


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)
    if "--lib-only" not in sys.argv:
        build_oracle()
        build_ctests()
