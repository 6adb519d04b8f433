"""The host-memory header's part that needs no GPU: cdc::Carver
(plakar_amd/csrc/cdc_hostmem.h) lays regions out exactly as the carving lambda
it replaced, judged by the stand-alone sanitizer program tests/c/carve_check.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carver_matches_the_lambda_it_replaced(tmp_path):
    exe = str(tmp_path / "carve_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "c", "carve_check.cpp")]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[0].startswith("2000 lists, ") and r.stdout.rstrip().endswith("ok"), r.stdout[-1000:]
