"""CPU: the U-Net program for the two latent-consistency presets (config.LCM_DREAMSHAPER_V7_UNET, config.TINY_LCM), checked as
tests/test_program_host.py checks every other preset -- the C++ invariants, the ordered parameter list against
config.param_shapes, counters and the 64-bit hash of the canonical dump -- against their own record,
tests/golden/program_digest_lcm.json.  The program of each differs from its base preset (SD15_UNET, TINY_LDM) by one
parameter, time_embed.cond_proj.weight, and by nothing else; a negative or misplaced time_cond_proj_dim is refused."""
import json
import os

import pytest

import loco_edit_amd  # noqa: F401
from loco_edit_amd import config as K
from loco_edit_amd import hip
from test_program_host import check_exe, run_check  # noqa: F401  (check_exe: the module-scoped fixture that builds the checker)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"LCM_DREAMSHAPER_V7_UNET": K.LCM_DREAMSHAPER_V7_UNET, "TINY_LCM": K.TINY_LCM}
BASES = {"LCM_DREAMSHAPER_V7_UNET": K.SD15_UNET, "TINY_LCM": K.TINY_LDM}


@pytest.fixture(scope="module")
def records(check_exe, tmp_path_factory):
    cfgs = {n: hip.c_cfg(c, 8) for n, c in CONFIGS.items()}
    cfgs.update({"base:" + n: hip.c_cfg(c, 8) for n, c in BASES.items()})
    rc, recs, out = run_check(check_exe, tmp_path_factory.mktemp("lcm_presets"), cfgs)
    bad = [l for l in out.splitlines() if l.startswith("BAD")]
    assert rc == 0 and not bad, "\n".join(bad[:40]) or out[-4000:]
    return recs


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_lcm_presets_build_match_param_shapes_and_their_digest(name, records):
    r = records[name]
    assert r["rc"] == 0
    assert r["param_list"] == [(k, tuple(v)) for k, v in K.param_shapes(CONFIGS[name]).items()]
    with open(os.path.join(ROOT, "tests", "golden", "program_digest_lcm.json")) as f:
        golden = json.load(f)
    assert {k: v for k, v in r.items() if k not in ("rc", "param_list")} == golden[name]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_lcm_presets_differ_from_their_base_by_cond_proj_only(name, records):
    r, b = records[name], records["base:" + name]
    cfg = CONFIGS[name]
    extra = ("time_embed.cond_proj.weight", (cfg.ch, cfg.time_cond_proj_dim))
    assert [p for p in r["param_list"] if p != extra] == b["param_list"]
    i = r["param_list"].index(extra)
    assert r["param_list"][i - 1][0] == "time_embed.2.bias"                     # listed where the time embedding's layers are
    assert r["elements"] == b["elements"] + cfg.ch * cfg.time_cond_proj_dim and r["params"] == b["params"] + 1
    for k in ("tensors", "ops", "per_sample", "stats_per_sample", "sx_total"):   # the memory plan and the op list are the base's
        assert r[k] == b[k], k
    assert records["LCM_DREAMSHAPER_V7_UNET"]["elements"] == 859_602_884


def test_lcm_presets_are_reached_by_name_and_by_import():
    from loco_edit_amd.config import LCM_DREAMSHAPER_V7_UNET, TINY_LCM
    assert LCM_DREAMSHAPER_V7_UNET is K.LCM_DREAMSHAPER_V7_UNET and TINY_LCM is getattr(K, "TINY_LCM")
    assert TINY_LCM.time_cond_proj_dim == 10 and LCM_DREAMSHAPER_V7_UNET.time_cond_proj_dim == 256
    with pytest.raises(AttributeError):
        K.NO_SUCH_PRESET


def test_time_cond_proj_dim_refusals(check_exe, tmp_path):
    msg = "time_cond_proj_dim must be >= 0 and belongs to the guided-diffusion family (arch 1)"
    cases = {}
    for n, base, v in (("negative", K.TINY_LCM, -1), ("ddpm", K.TINY_DDPM, 10), ("decoder", K.TINY_DECODER, 10)):
        c = hip.c_cfg(base, 8)
        c.time_cond_proj_dim = v
        cases[n] = c
    rc, recs, out = run_check(check_exe, tmp_path, cases)
    assert rc == 0, out[-4000:]
    for n in cases:
        assert recs[n] == {"rc": -2, "message": msg}, (n, recs[n])
