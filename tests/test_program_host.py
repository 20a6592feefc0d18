"""CPU: the U-Net program (loco-edit_amd/csrc/program.hip, host code only) compiled with plain g++ and built for every preset
by tests/c/program_check.cpp from the bytes hip.c_cfg would hand to loco_create:

- layout / ordering invariants the passes rely on, asserted in C++ for every config (tensor ranges and alignment, overlap only
  as a concatenation and its parts, inputs written before they are read, consumer norms, disjoint statistics blocks and
  {S, xhat} cache ranges, unique parameter names);
- the ordered (name, shape) parameter list equals config.param_shapes (the Python restatement the checkpoints are loaded by);
- the program equals, field by field, the one the engine built before the program moved into its own unit: counters and a
  64-bit hash of the canonical dump in tests/golden/program_digest.json (a config without an entry fails: a new preset is added
  to the digest deliberately);
- every configuration the builder refuses is refused with its message.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

import loco_edit_amd  # noqa: F401
from loco_edit_amd import config as K
from loco_edit_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

CONFIGS = {n: getattr(K, n) for n in dir(K) if isinstance(getattr(K, n), K.UNetConfig)}
CONFIGS["IF_I_L_UNET"] = K.if_stage1_config("L")
CONFIGS["IF_I_XL_UNET"] = K.if_stage1_config("XL")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip(f"HIP headers not found under {ROCM}/include")
    exe = str(tmp_path_factory.mktemp("program") / "program_check")
    subprocess.run([gxx, "-O1", "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                    os.path.join(ROOT, "loco-edit_amd", "csrc", "program.hip"), os.path.join(ROOT, "tests", "c", "program_check.cpp"),
                    "-o", exe], check=True)
    return exe


def run_check(exe, tmp_path, cfgs, dump=None):
    """cfgs: {name: LocoCfg}.  Returns (returncode, {name: record}, stdout); record = counters + "param_list", or rc + "message"."""
    path = tmp_path / "configs.txt"
    path.write_text("".join(f"{n} {bytes(c).hex()}\n" for n, c in cfgs.items()))
    r = subprocess.run([exe, str(path)] + ([dump] if dump else []), capture_output=True, text=True, timeout=300)
    recs, cur = {}, None
    for line in r.stdout.splitlines():
        p = line.split()
        if p[0] == "CFG":
            rc = int(p[2].split("=")[1])
            if rc == 0:
                cur = {k: (v if k == "hash" else int(v)) for k, v in (x.split("=") for x in p[2:])}
                cur["param_list"] = []
            else:
                cur = {"rc": rc, "message": " ".join(p[3:])}
            recs[p[1]] = cur
        elif p[0] == "P":
            cur["param_list"].append((p[1], tuple(int(x) for x in p[2:])))
    return r.returncode, recs, r.stdout + r.stderr


@pytest.fixture(scope="module")
def records(check_exe, tmp_path_factory):
    rc, recs, out = run_check(check_exe, tmp_path_factory.mktemp("presets"), {n: hip.c_cfg(c, 8) for n, c in CONFIGS.items()})
    bad = [l for l in out.splitlines() if l.startswith("BAD")]
    assert rc == 0 and not bad, "\n".join(bad[:40]) or out[-4000:]
    return recs


def test_every_preset_builds_and_keeps_the_invariants(records):
    assert len(CONFIGS) >= 30
    assert set(records) == set(CONFIGS)
    for n, r in records.items():
        assert r["rc"] == 0, (n, r)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_parameter_list_matches_config_param_shapes(name, records):
    cfg = CONFIGS[name]
    host_side = ("encoder_proj.", "encoder_pooling.")       # applied to the prompt states before the engine (load_state_dict skips them)
    want = [(k, tuple(v)) for k, v in K.param_shapes(cfg).items() if not (cfg.encoder_dim > 0 and k.startswith(host_side))]
    assert records[name]["param_list"] == want


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_program_matches_the_recorded_digest(name, records):
    with open(os.path.join(ROOT, "tests", "golden", "program_digest.json")) as f:
        golden = json.load(f)
    assert name in golden, f"{name} has no entry in tests/golden/program_digest.json"
    got = {k: v for k, v in records[name].items() if k not in ("rc", "param_list")}
    assert got == golden[name], "program differs: run program_check with the config name as second argument to print the dump"


def test_published_parameter_counts(records):
    for name, n in (("CELEBA_DDPM", 113_673_219), ("SD15_UNET", 859_520_964), ("SD21_BASE_UNET", 865_910_724),
                    ("SD_VAE_DECODER", 49_490_199), ("SD_VAE_ENCODER", 34_163_664)):
        assert records[name]["elements"] == n, name


def _with(base, **kw):
    c = hip.c_cfg(base, 8)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


REFUSALS = {
    "max_batch": (_with(K.TINY_DDPM, max_batch=0), "bad config"),
    "levels": (_with(K.TINY_DDPM, num_levels=9), "bad config"),
    "arch": (_with(K.TINY_DDPM, arch=4), "arch must be 0 (Ho-DDPM), 1 (guided-diffusion family), 2 (latent decoder) or 3 (latent encoder)"),
    "resolution_pow2": (_with(K.TINY_DDPM, resolution=48), "resolution must be a power of two with >= 8x8 at the coarsest level"),
    "resolution_small": (_with(K.TINY_DDPM, resolution=8), "resolution must be a power of two with >= 8x8 at the coarsest level"),
    "ch": (_with(K.TINY_DDPM, ch=48), "ch must be a multiple of 32"),
    "act": (_with(K.TINY_ADM, act=2), "act must be 0 (SiLU) or 1 (GELU)"),
    "act_family": (_with(K.TINY_DDPM, act=1), "act / res_scale / added_kv belong to the guided-diffusion family (arch 1)"),
    "res_scale_family": (_with(K.TINY_DDPM, res_scale=0.5), "act / res_scale / added_kv belong to the guided-diffusion family (arch 1)"),
    "added_kv_family": (_with(K.TINY_DECODER, added_kv=1), "act / res_scale / added_kv belong to the guided-diffusion family (arch 1)"),
    "added_kv_context": (_with(K.TINY_IF, context_len=0),
                         "added_kv needs context_dim (a multiple of gn_groups) and context_len > 0 and transformer_depth = 0"),
    "added_kv_groups": (_with(K.TINY_IF, context_dim=K.TINY_IF.context_dim + 1),
                        "added_kv needs context_dim (a multiple of gn_groups) and context_len > 0 and transformer_depth = 0"),
}
# "resampling ResBlock with a channel change is not supported" stays in build_program as a guard on the builders themselves:
# they give a resampling block the channel count of its input, so no configuration reaches it.


def test_refusals(check_exe, tmp_path):
    assert len(K.TINY_DDPM.ch_mult) >= 2 and K.TINY_DDPM.resolution >= 16 and K.TINY_IF.added_kv
    rc, recs, out = run_check(check_exe, tmp_path, {n: c for n, (c, _) in REFUSALS.items()})
    assert rc == 0, out[-4000:]
    for n, (_, msg) in REFUSALS.items():
        assert recs[n] == {"rc": -2, "message": msg}, (n, recs[n])


def test_a_wrong_struct_is_reported_not_read(check_exe, tmp_path):
    class Short(C.Structure):
        _fields_ = [("struct_size", C.c_int32)]
    rc, recs, _ = run_check(check_exe, tmp_path, {"short": Short(4)})
    assert rc == 1 and recs["short"]["rc"] == -9
