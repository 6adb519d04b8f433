"""The readers' host-only layer (plakar_amd/csrc/cdc_blobsrc.h, cdc_hostutil.h)
under AddressSanitizer and UBSan: the stand-alone program tests/c/blobsrc_check.cpp
gathers seeded span lists from packfiles in memory and on disk, loses two files,
counts its open descriptors, looks checksums up and hands off between threads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def blobsrc_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blobsrc") / "blobsrc_check")
    csrc = os.path.join(ROOT, "plakar_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe,
           os.path.join(ROOT, "tests", "c", "blobsrc_check.cpp"), os.path.join(csrc, "cdc_blobsrc.cpp"),
           os.path.join(csrc, "cdc_sha256.cpp")]
    subprocess.run(cmd, check=True)
    return exe


def test_gather_resolve_and_handoff_under_sanitizers(blobsrc_check_exe):
    """150 span lists at 1, 2 and 8 threads and once with the read skipped, a
    deleted and a truncated packfile at each thread count, 300 lookups; no
    descriptor left open, no sanitizer report and no broken promise."""
    r = subprocess.run([blobsrc_check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) gathers, (\d+) lost blobs, (\d+) resolves, handoff ok, ok", r.stdout)
    assert m and int(m.group(1)) == 150 * 4 + 3 and int(m.group(2)) > 10 and int(m.group(3)) == 300, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
