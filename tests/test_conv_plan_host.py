"""CPU: the conv launch planner (loco-edit_amd/csrc/conv_plan.hip, host code only) compiled with plain g++ and swept over
precisions, shapes, batches, lanes, statistics requests, norm-cotangent requests and shortcuts by tests/c/conv_plan_check.cpp:
workspace fits, epilogue statistics only where the kernels take them, disjoint lane rows of the kept partials, the norm-cotangent
term only where the epilogue has it, tail splits that cover the batch, profile names that match the planned tile, and the two
recorded decisions pinned to their values."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_conv_plan_invariants(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip(f"HIP headers not found under {ROCM}/include")
    exe = str(tmp_path / "conv_plan_check")
    cmd = [gxx, "-O2", "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include"]
    cmd += [os.path.join(ROOT, "loco-edit_amd", "csrc", "conv_plan.hip"), os.path.join(ROOT, "tests", "c", "conv_plan_check.cpp"),
            "-o", exe]
    subprocess.run(cmd, check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
