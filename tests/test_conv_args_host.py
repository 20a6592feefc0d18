"""CPU: the ConvArgs constructor of the passes (loco-edit_amd/csrc/engine_internal.h `conv_args`, host code only) compiled with
plain g++ under AddressSanitizer / UBSan as a stand-alone program, tests/c/conv_args_check.cpp: a forward, a transposed and a
1x1 launch on non-square views of different levels, every byte against the field list the passes used to spell out.  The
sanitizer runtimes are linked statically, so the program runs the same whatever else the process environment preloads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_conv_args_fills_what_the_field_list_filled(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip(f"HIP headers not found under {ROCM}/include")
    exe = str(tmp_path / "conv_args_check")
    subprocess.run([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", os.path.join(ROOT, "tests", "c", "conv_args_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "conv_args_check: ok", r.stdout + r.stderr
