"""CPU: the host side of the latent-consistency path (loco_edit_amd.tloco_lcm, define_argparser, checkpoints, config): the
scheduler's timestep tables, scalings and step coefficients, the guidance-scale embedding, the routing of the two shipped LCM
scripts, the parameter counts and the diffusers key map with `time_embedding.cond_proj`."""
import json
import math
import os

import numpy as np
import pytest
import torch

import loco_edit_amd  # noqa: F401
import lcm_restatement as R
from loco_edit_amd import checkpoints, config, define_argparser
from loco_edit_amd.tloco_lcm import LCMScheduler, guidance_scale_embedding, lcm_timesteps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ("main_T2I_LCM_null_space_projection.sh", "main_T2I_LCM_null_space_projection_nonsemantic.sh")

TABLES = {
    ("linspace", 4): [999, 759, 499, 259],
    ("stride", 4): [999, 759, 519, 279],
    ("linspace", 8): [999, 879, 759, 639, 499, 379, 259, 139],
    ("stride", 8): [999, 879, 759, 639, 519, 399, 279, 159],
}


@pytest.mark.parametrize("rule", ["linspace", "stride"])
@pytest.mark.parametrize("n", [1, 2, 4, 8, 50])
def test_timestep_tables(rule, n):
    got = lcm_timesteps(n, rule)
    s = LCMScheduler(rule=rule)
    s.set_timesteps(n)
    assert s.timesteps.tolist() == got == R.timesteps(n, rule)
    if (rule, n) in TABLES:
        assert got == TABLES[(rule, n)]
    if n in (1, 2, 50):       # the two rules agree
        assert got == lcm_timesteps(n, "stride" if rule == "linspace" else "linspace")
        assert got == {1: [999], 2: [999, 499], 50: list(range(999, 0, -20))}[n]
    assert all(a > b for a, b in zip(got, got[1:])) and len(got) == n


def test_timestep_rule_is_checked():
    with pytest.raises(ValueError):
        lcm_timesteps(4, "karras")
    with pytest.raises(ValueError):
        LCMScheduler(rule="")
    with pytest.raises(ValueError):
        lcm_timesteps(51, "linspace")


def test_scalings_against_float64():
    s = LCMScheduler()
    for t in (999, 759, 499, 259, 19, 0):
        c_skip, c_out = s.scalings(t)
        st = t * 10.0
        ref = (0.25 / (st * st + 0.25), st / math.sqrt(st * st + 0.25))
        assert (c_skip, c_out) == (float(np.float32(ref[0])), float(np.float32(ref[1])))      # float64, rounded once
        assert ref == pytest.approx(R.scalings(t), rel=1e-15)
    assert s.scalings(499)[0] == pytest.approx(1.004e-8, rel=1e-3)
    assert s.scalings(19)[0] == pytest.approx(6.925e-6, rel=1e-3)
    assert s.scalings(0) == (1.0, 0.0)
    lo = LCMScheduler(timestep_scaling=0.001)
    assert lo.scalings(499) == pytest.approx((0.501, 0.706), abs=1e-3)


def test_alpha_table_and_step_coefficients():
    s = LCMScheduler(rule="linspace")
    s.set_timesteps(4)
    assert torch.equal(s.alphas_cumprod, R.alphas_cumprod())
    ab = s.alphas_cumprod
    assert s.step_coeffs(999) == (0, float(ab[999]), float(ab[759]), False)
    assert s.step_coeffs(499) == (2, float(ab[499]), float(ab[259]), False)
    i, at, at_prev, last = s.step_coeffs(259)
    assert (i, at, at_prev, last) == (3, float(ab[259]), 1.0, True)      # final_alpha_cumprod; no noise behind the last index
    with pytest.raises(ValueError):
        s.step_coeffs(519)                                               # not in this table


def test_no_noise_on_the_last_index():
    """step() hands the engine no noise on the last index (a given noise is dropped there) and at_prev = 1."""
    calls = []

    class Eng:
        def lcm_step(self, x, eps, at, at_prev, c_skip, c_out, noise):
            calls.append((at, at_prev, c_skip, c_out, noise))
            return x, x
    s = LCMScheduler(engine=Eng(), rule="stride")
    s.set_timesteps(4)
    x = torch.zeros(1, 4, 2, 2)
    s.step(x, 279, x, noise=torch.ones_like(x))
    s.step(x, 519, x, noise=torch.ones_like(x))
    s.step(x, 999, x)
    assert calls[0][1] == 1.0 and calls[0][4] is None
    assert calls[1][1] == float(s.alphas_cumprod[279]) and torch.equal(calls[1][4], torch.ones_like(x))
    assert calls[2][4] is not None and calls[2][4].shape == x.shape      # drawn
    assert calls[0][2:4] == s.scalings(279)


@pytest.mark.parametrize("dim", [10, 256, 11])
def test_guidance_scale_embedding(dim):
    w = 6.5
    got = guidance_scale_embedding(w, dim)
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32) * -(torch.log(torch.tensor(10000.0)) / (half - 1)))
    a = torch.tensor(w, dtype=torch.float32) * 1000.0 * f
    ref = torch.cat([torch.sin(a), torch.cos(a)] + ([torch.zeros(1)] if dim % 2 else []))
    assert got.dtype == torch.float32 and tuple(got.shape) == (dim,)
    assert torch.equal(got, ref) and torch.equal(got, R.guidance_embedding(w, dim))
    ref64 = torch.cat([torch.sin(a.double()), torch.cos(a.double())])
    assert (got[:2 * half].double() - ref64).abs().max() < 1e-6


def _argv(name):
    with open(os.path.join(ROOT, "tests", "golden", "script_args.json")) as f:
        return json.load(f)[name]


@pytest.mark.parametrize("script", SCRIPTS)
def test_preset_refuses_the_bare_lists_and_routes_them_with_the_flag(script, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    argv = _argv(script) + ["--device", "cpu"]
    with pytest.raises(NotImplementedError) as e:
        define_argparser.preset(define_argparser.parse_args(argv))
    assert "--lcm_timesteps" in str(e.value) and "[999, 759, 499, 259]" in str(e.value) and "[999, 759, 519, 279]" in str(e.value)
    for rule in ("linspace", "stride"):
        a = define_argparser.preset(define_argparser.parse_args(argv + ["--lcm_timesteps", rule]))
        assert a.is_LCM and not a.is_stable_diffusion and not a.is_DeepFloyd_IF_diffusion
        assert a.exp == "LCM-Random-with_prompt" and a.lcm_timesteps == rule
        assert a.unet_config is config.LCM_DREAMSHAPER_V7_UNET and a.vae_config is config.SD_VAE_DECODER
        assert (a.c_in, a.image_size, a.num_inference_steps, a.edit_t_idx) == (4, 64, 4, 2)
        assert not a.use_yh_custom_scheduler            # the shipped lists say False: none of the SD asserts apply
    with pytest.raises(SystemExit):
        define_argparser.parse_args(argv + ["--lcm_timesteps", "karras"])
    b = define_argparser.preset(define_argparser.parse_args(argv + ["--lcm_timesteps", "linspace", "--unet_preset", "tiny_lcm",
                                                                    "--vae_preset", "tiny_decoder"]))
    assert b.unet_config is config.TINY_LCM and b.vae_config is config.TINY_DECODER and (b.c_in, b.image_size) == (4, 16)


def test_parameter_counts():
    count = lambda c: sum(int(np.prod(s)) for s in config.param_shapes(c).values())
    assert count(config.SD15_UNET) == 859_520_964
    assert count(config.LCM_DREAMSHAPER_V7_UNET) == 859_520_964 + 320 * 256 == 859_602_884
    assert count(config.TINY_LCM) == count(config.TINY_LDM) + 32 * 10
    sh = config.param_shapes(config.TINY_LCM)
    assert sh["time_embed.cond_proj.weight"] == (32, 10) and "time_embed.cond_proj.bias" not in sh
    assert list(config.param_shapes(config.TINY_LDM)) == [k for k in sh if k != "time_embed.cond_proj.weight"]
    assert config.synth_params(config.TINY_LCM, 0)["time_embed.cond_proj.weight"].shape == (32, 10)
    assert config.LCM_DREAMSHAPER_V7_UNET == config.UNetConfig(**{**config.SD15_UNET.__dict__, "time_cond_proj_dim": 256})


def test_key_map_round_trip_with_cond_proj():
    cfg = config.TINY_LCM
    sd = {k: torch.from_numpy(v) for k, v in config.synth_params(cfg, 0).items()}
    hf = checkpoints.ldm_to_hf_unet2d_condition(sd, cfg)
    assert "time_embedding.cond_proj.weight" in hf and "time_embedding.linear_1.weight" in hf and "time_embedding.linear_2.bias" in hf
    assert torch.equal(hf["time_embedding.cond_proj.weight"], sd["time_embed.cond_proj.weight"])
    back = checkpoints.hf_unet2d_condition_to_ldm(hf, cfg)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # the fault this replaces: cond_proj.weight used to land on time_embed.2.weight
    assert torch.equal(back["time_embed.2.weight"], sd["time_embed.2.weight"])
    assert tuple(back["time_embed.cond_proj.weight"].shape) == (32, 10)
    # a configuration without the guidance input refuses the LCM file
    with pytest.raises(ValueError, match="time_cond_proj_dim"):
        checkpoints.hf_unet2d_condition_to_ldm(hf, config.TINY_LDM)
    # and a plain SD file keeps its mapping exactly
    plain = {k: torch.from_numpy(v) for k, v in config.synth_params(config.TINY_LDM, 0).items()}
    hf_plain = checkpoints.ldm_to_hf_unet2d_condition(plain, config.TINY_LDM)
    assert "time_embedding.cond_proj.weight" not in hf_plain
    back_plain = checkpoints.hf_unet2d_condition_to_ldm(hf_plain, config.TINY_LDM)
    assert set(back_plain) == set(plain) and all(torch.equal(back_plain[k], plain[k]) for k in plain)


def test_restated_step_and_fold_identity():
    """The helper's own algebra: the folded bias reproduces emb + cond_proj(w_emb) ahead of the first dense layer."""
    g = torch.Generator().manual_seed(3)
    p = {k: torch.from_numpy(v) for k, v in config.synth_params(config.TINY_LCM, 0).items()}
    w_emb = R.guidance_embedding(6.5, 10)
    q = R.fold_cond(p, w_emb)
    emb = torch.randn(5, 32, generator=g, dtype=torch.float64)
    W0, b0, Wc = p["time_embed.0.weight"].double(), p["time_embed.0.bias"].double(), p["time_embed.cond_proj.weight"].double()
    want = torch.nn.functional.linear(emb + Wc @ w_emb.double(), W0, b0)
    got = torch.nn.functional.linear(emb, W0, q["time_embed.0.bias"].double())
    assert (want - got).abs().max() < 1e-6
    x, e, nz = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
    prev, den = R.lcm_step(x, e, 0.3, 0.6, 1.0, 0.0, nz)
    assert torch.equal(den, x) and torch.allclose(prev, math.sqrt(0.6) * x + math.sqrt(0.4) * nz)
