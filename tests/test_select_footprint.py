"""Compile-time footprint of the corner-selection kernel (no GPU needed).

One 1024-thread selection workgroup per image runs for a long, latency-bound time; the point of its packed LDS
layout and its register budget is that a workgroup of the response kernel (K1), of describe_tile_kernel or of the
matcher still fits on the same compute unit.  The figures are read from the compiler's own resource remarks for
gfx950, with the co-resident kernels' figures taken from the same compile, so the property cannot regress
silently with the next compiler or edit."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "visual-slam_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
# the flags of visual-slam_amd/csrc/Makefile
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
PER_FILE = {"detect.hip": ["-fno-slp-vectorize"], "match.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"], "describe.hip": []}

LDS_PER_CU = 160 * 1024     # gfx950
VGPRS_PER_LANE = 512        # unified vector + accumulator file of one SIMD
VGPR_GRANULE = 8
SELECT_WAVES_PER_SIMD = 4   # 1024 threads = 16 waves over 4 SIMDs


def _alloc(k):
    """Registers a wave of kernel k occupies: accumulator registers start at the next multiple of 4 after the
    vector registers, the total is rounded up to the allocation granule."""
    n = k["VGPRs"]
    if k["AGPRs"]:
        n = -(-n // 4) * 4 + k["AGPRs"]
    return -(-n // VGPR_GRANULE) * VGPR_GRANULE


def _compile(name, tmp_path):
    asm = tmp_path / (name + ".s")
    r = subprocess.run([HIPCC, *FLAGS, *PER_FILE[name], "-I", str(ROOT / "include"), "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(asm), str(CSRC / name)],
                       check=True, capture_output=True, text=True, timeout=900)
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0].replace(" ", "")] = int(m.group(2))
    meta = asm.read_text().split("amdhsa.kernels:")[1]
    for block in meta.split("- .agpr_count:")[1:]:
        kname = re.search(r"\.name:\s+(\S+)", block).group(1)
        if kname in kernels:
            kernels[kname]["threads"] = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1))
    return kernels


def _pick(kernels, needle):
    got = {n: k for n, k in kernels.items() if needle in n and "threads" in k}
    assert got, "no kernel named *%s*" % needle
    return got


@pytest.fixture(scope="module")
def footprint(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("footprint")
    det, des, mat = (_compile(n, tmp) for n in ("detect.hip", "describe.hip", "match.hip"))
    sel = _pick(det, "select_kernelILb0E")
    sel_global = _pick(det, "select_kernelILb1E")
    assert len(sel) == 1 and len(sel_global) == 1
    out = {"select": next(iter(sel.values())), "select_global": next(iter(sel_global.values())),
           "k1": _pick(det, "min_eig_response_kernelILb0E"),      # the instances of the pass (no response image stored)
           "describe": _pick(des, "describe_tile_kernel"), "matcher": _pick(mat, "hamming_mx_kernel")}
    for name in ("select", "select_global"):
        print(name, out[name])
    for name in ("k1", "describe", "matcher"):
        for n, k in out[name].items():
            print(name, n, k, "alloc", _alloc(k))
    return out


def test_select_workgroup_is_the_whole_workgroup(footprint):
    assert footprint["select"]["threads"] == 1024 and footprint["select_global"]["threads"] == 1024


def test_select_lds_leaves_room_for_any_kernel_of_the_pass(footprint):
    others = [k["LDSSize"] for g in ("k1", "describe", "matcher") for k in footprint[g].values()]
    assert footprint["select"]["LDSSize"] + max(others) <= LDS_PER_CU, (footprint["select"]["LDSSize"], max(others))


@pytest.mark.parametrize("other", ["k1", "describe"])
def test_select_registers_leave_room_for_a_workgroup(footprint, other):
    sel = SELECT_WAVES_PER_SIMD * _alloc(footprint["select"])
    for name, k in footprint[other].items():
        waves = -(-k["threads"] // 256)   # waves per SIMD of one workgroup
        assert sel + waves * _alloc(k) <= VGPRS_PER_LANE, (name, _alloc(footprint["select"]), waves, _alloc(k))


def test_select_does_not_spill(footprint):
    assert footprint["select"]["ScratchSize"] == 0
    assert footprint["select_global"]["ScratchSize"] == 0
