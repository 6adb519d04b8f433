"""The compiler's resource report of the chunking kernels (no GPU needed).

plakar_amd.build keeps hipcc's kernel-resource-usage remarks next to the
library.  k_resolve once carried a copy of its whole by-value Batch argument
(1,864 bytes) in every lane's private memory because one out-of-line helper
took the argument by reference; these bounds keep that from
coming back unnoticed.
"""
import os
import re

import pytest

from plakar_amd import build

# an eighth of sizeof(Batch): no copy of the launch descriptor hides under it
RESOLVE_PRIVATE_MAX = 256
SCAN_PRIVATE_MAX = 12  # k_scan's two spilled registers and its flat-scratch bookkeeping


def _kernels():
    path = build.resources_path()
    if not os.path.exists(path):
        pytest.skip(f"{path} is absent: the library was not built by plakar_amd.build here")
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
            if not m:
                continue
            key, _, val = m.group(1).partition(":")
            if key.strip() == "Function Name":
                cur = out.setdefault(val.strip(), {})
            elif cur is not None:
                cur[key.strip()] = val.strip()
    return out


def _kernel(name):
    """The entry of cdc::<name>(Batch, DevParams, Workspace)."""
    mangled = f"_ZN3cdc{len(name)}{name}ENS_5BatchENS_9DevParamsENS_9WorkspaceE"
    ks = _kernels()
    assert mangled in ks, f"{name} is not in the resource report ({len(ks)} kernels listed)"
    return ks[mangled]


def test_resolve_keeps_no_copy_of_the_launch_descriptor():
    k = _kernel("k_resolve")
    assert int(k["ScratchSize [bytes/lane]"]) < RESOLVE_PRIVATE_MAX


def test_resolve_spills_no_vector_registers():
    assert int(_kernel("k_resolve")["VGPRs Spill"]) == 0


def test_scan_private_segment_has_not_grown():
    assert int(_kernel("k_scan")["ScratchSize [bytes/lane]"]) <= SCAN_PRIVATE_MAX
