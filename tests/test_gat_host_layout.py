"""CPU tier of the GAT family's host-side dispatch layer (csrc/host_gat.h): each helper exists once in the sources, and
the one launch-geometry rule is the one the GPU suites model (test_gat_launch_geometry.py: _cpg, _grid), for valid and
invalid knob values alike.  The geometry is read from tests/host/gat_geometry.hip, a stand-alone program that includes
the header, brings its own tuning() and is built with the host-side address and undefined-behaviour sanitizers."""
import functools
import glob
import os
import re
import subprocess

from test_gat_launch_geometry import FAST_HD, MAX_ROW_BLOCKS, _cpg, _grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "custom_op_benchmark_amd", "csrc")
FAMILY = ("gat.hip", "gatv2.hip", "gat_attention.hip", "gat_edge_attention.hip", "gatv2_attention.hip",
          "gatv2_edge_attention.hip", "host_gat.h", "host_gat_attn_ops.h", "host_gatv2_attn_ops.h")
OPS_HEADERS = ("host_gat_attn_ops.h", "host_gatv2_attn_ops.h")
OLD_NAMES = ("gv2attn_check", "gatv2_check_plan", "gv2attn_fast_ok", "gatv2_fast_ok", "GO_DISPATCH_GV2ATTN",
             "GO_DISPATCH_GATV2", "gv2attn_cpg", "gatv2_cpg", "gat_attn_cpg", "gv2attn_grid_of", "edge_aligned")
N_CHUNKS = (0, 1, 15, 16, 17, 4095, 4096, 10 ** 6, 8192 * 16 * 3 + 1)
CAPS = (-1, 0, 1, 3, 16)
GROUPS = (16, 32, 64)
N_CUS = (1, 256)


@functools.lru_cache(maxsize=None)
def _sources():
    paths = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))
    return {os.path.basename(p): open(p).read() for p in paths}


def test_the_hd_switch_exists_once_and_holds_the_fast_pairs():
    holders = [n for n, text in _sources().items() if "case 1064:" in text]
    assert holders == ["host_gat.h"]
    cases = re.findall(r"case (\d+): \{ constexpr int H = (\d+), D = (\d+);", _sources()["host_gat.h"])
    assert all(int(c) == 1000 * int(h) + int(d) for c, h, d in cases)
    assert sorted((int(h), int(d)) for _, h, d in cases) == sorted(FAST_HD) and len(cases) == len(FAST_HD)


def test_the_id_bound_is_written_in_the_header_and_in_gat_hip_only():
    assert set(FAMILY) <= set(_sources())
    holders = {n for n in FAMILY if "0x7fffffffLL" in _sources()[n]}
    assert holders <= {"host_gat.h", "gat.hip"}


def test_no_private_copy_of_a_helper_is_left():
    for name in OLD_NAMES:
        assert [n for n, text in _sources().items() if name in text] == [], name
    assert "host_gat_attn.h" not in _sources()


def test_a_launch_is_written_once_for_both_edge_forms_and_both_dtypes():
    for name in OPS_HEADERS:
        assert re.search(r"if constexpr \(EDGE\)\s+(hipLaunchKernelGGL|go_launch)", _sources()[name]) is None, name
        assert "go_launch(" in _sources()[name] and "arg_if<EDGE>(" in _sources()[name], name
    assert [n for n in FAMILY if "go(0.f)" in _sources()[n]] == []


@functools.lru_cache(maxsize=None)
def _geometry_lines():
    """the output of tests/host/gat_geometry.hip, built into a fresh temporary directory and run once"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gat_geometry")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "--cuda-host-only",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        os.path.join(ROOT, "tests", "host", "gat_geometry.hip"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [ln.split() for ln in r.stdout.splitlines()]


def test_cpg_and_grid_follow_the_one_rule():
    got = {tuple(map(int, f[1:5])): (int(f[5]), int(f[6])) for f in _geometry_lines() if f[0] == "cpg"}
    assert set(got) == {(n_cu, G, cap, n) for n_cu in N_CUS for G in GROUPS for cap in CAPS for n in N_CHUNKS}
    for (n_cu, G, cap, n), (cpg, grid) in got.items():
        assert cpg == _cpg(n, n_cu, G, cap), (n_cu, G, cap, n)
        assert grid == _grid(n, cpg, G), (n_cu, G, cap, n)


def test_the_row_pass_stays_under_the_block_cap_and_moves_cpg_only_for_it():
    rows = [tuple(map(int, f[1:])) for f in _geometry_lines() if f[0] == "row"]
    assert {r[:3] for r in rows} == {(n_cu, cap, n) for n_cu in N_CUS for cap in CAPS for n in N_CHUNKS}
    raised = 0
    for n_cu, cap, n, cpg, grid, row_cpg, row_blocks in rows:
        assert (cpg, grid) == (_cpg(n, n_cu, 16, cap), _grid(n, _cpg(n, n_cu, 16, cap)))
        assert row_blocks <= MAX_ROW_BLOCKS and row_blocks == _grid(n, row_cpg)
        if grid <= MAX_ROW_BLOCKS:
            assert (row_cpg, row_blocks) == (cpg, grid)
        else:
            assert row_cpg > cpg
            raised += 1
    assert raised > 0       # the cases reach the clause that raises cpg
