"""The grid caps that tests/test_grid_wrap.py sizes its cases by, read out of
plakar_amd/csrc and compared with the values mirrored there (no GPU needed).
A case of test_grid_wrap.py has about 2 * cap + 70 items; with a larger cap it
would still pass, without ever sending a wave round its loop again.  So a
changed cap fails here, with the cases to resize."""
import os
import re

import pytest

import test_grid_wrap as gw

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plakar_amd", "csrc")

# the launches that apply the caps: the expression each grid is cut to
LAUNCHES = {
    "cdc_diff.hip": [r"device_cus\(device\)\)\s*\*\s*kBlocksPerCU\b",       # grid_for: k_line_*, a wave per item
                     r"device_cus\(device\)\)\s*\*\s*kEmitBlocksPerCU\b"],  # k_diff_emit
    "cdc_restore.hip": [r"J\.ntiles,\s*uint64_t\(cdc::device_cus\(device\)\)\s*\*\s*kBlocksPerCU\b"],  # k_assemble
    "cdc_digest.hip": [r"/\s*kHistWaves,\s*uint64_t\(cus\)\s*\*\s*kHistBlocksPerCU\b",  # k_chunk_hist
                       r"/\s*kEntWaves,\s*kEntMaxBlocks\)"],                            # k_chunk_entropy
}


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, name):
    """The value of `constexpr <type> ... name = <integer expression>`."""
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", text)
    assert m, f"no constexpr {name}"
    expr = re.sub(r"(\d)[uUlL]+\b", r"\1", m.group(1)).strip()
    assert re.fullmatch(r"[\d\s<>*+()xXa-fA-F]+", expr), f"{name} = {m.group(1)!r} is not an integer expression"
    return int(eval(expr, {"__builtins__": {}}))  # digits, shifts, products and sums only


@pytest.mark.parametrize("name,const", [(n, c) for n, cs in gw.MIRRORED.items() for c in cs])
def test_a_cap_is_what_the_wrap_tests_mirror(name, const):
    want, cases = gw.MIRRORED[name][const]
    got = _constant(_source(name), const)
    assert got == want, (f"{name}: {const} is {got}, tests/test_grid_wrap.py mirrors {want}: set it there and resize "
                         f"{cases}, so that they still pass twice the cap")


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_the_launches_still_apply_these_caps(name):
    text = _source(name)
    for pattern in LAUNCHES[name]:
        assert re.search(pattern, text), (f"{name}: no launch cuts its grid by /{pattern}/ any more: mirror the new "
                                          f"cap in tests/test_grid_wrap.py and resize the cases of {sorted(gw.MIRRORED[name])}")


def test_the_mirror_names_cases_that_exist():
    assert gw.MIRRORED["cdc_diff.hip"]["kEmitBlocksPerCU"][0] == gw.kEmitBlocksPerCU
    assert gw.MIRRORED["cdc_digest.hip"]["kHistBlocksPerCU"][0] == gw.kHistBlocksPerCU
    assert gw.MIRRORED["cdc_digest.hip"]["kEntMaxBlocks"][0] == gw.kEntMaxBlocks
    for name, consts in gw.MIRRORED.items():
        for const, (value, cases) in consts.items():
            assert isinstance(value, int) and value > 0 and cases.startswith("test_"), (name, const)
            for case in cases.split(", "):
                assert callable(getattr(gw, case)), f"{case} is not a case of tests/test_grid_wrap.py"
