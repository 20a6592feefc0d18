"""CPU: the LDS carve-up of the encoders' streamed attention kernel (loco-edit_amd/csrc/enc_attn_lds.h `enc_attn_lds_floats`, plain
C++) compiled with g++ under AddressSanitizer / UBSan as a stand-alone program, tests/c/enc_attn_lds_check.cpp: for every head
width 1..128 and table size 0..64 the count of the SAM kernel's formula, and at size 0 the count of the CLIP kernel's, both
restated there -- so the 64 KiB refusals of loco_sam_create and loco_clipvis_create fire where they fired before.  The sanitizer
runtimes are linked statically, so the program runs the same whatever else the process environment preloads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_enc_attn_lds_floats_equals_both_former_formulas(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path / "enc_attn_lds_check")
    subprocess.run([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "enc_attn_lds_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "enc_attn_lds_check: ok", r.stdout + r.stderr
