"""CPU: the h-space restatement (tests/hspace_oracle.py) and the Program's tap.

- cutting the oracle's forward pass at the bottleneck changes nothing: h_to_e(get_h(x)) and forward_dh(x, None) equal the
  oracle's unet_forward / unet_forward_adm exactly;
- the restatement equals what the reference's own get_h / get_h_to_e / forward(u) computed (tests/golden/hspace_tiny_ddpm.pt,
  written by tests/make_golden_hspace.py), rel-L2 <= 1e-6 in float32;
- build_program records the tap: h_t / h_last_op name the output of the middle block's last op, which is the first part of the
  first up-path concatenation; the latent decoder and encoder have none.  (The host unit is compiled with plain g++ and driven
  by tests/c/program_tap.cpp, the way tests/test_conv_plan_host.py drives the planner.)
"""
import os
import shutil
import subprocess

import pytest
import torch

import loco_edit_amd  # noqa: F401
import loco_oracle as orc
from loco_edit_amd import config as K
from loco_edit_amd import hip

import hspace_oracle as hso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("name", ["TINY_DDPM", "TINY_ADM", "TINY_ADM_PLAIN"])
def test_cut_at_the_bottleneck_is_the_oracle_forward(name):
    cfg = getattr(K, name)
    p = orc.to_torch(K.synth_params(cfg, 0))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, cfg.in_channels, cfg.resolution, cfg.resolution, generator=g)
    t = torch.tensor(601)
    with torch.no_grad():
        want = orc.denoiser(p, cfg, x, t)
        h = hso.get_h(p, cfg, x, t)
        assert torch.equal(hso.h_to_e(p, cfg, x, t, h), want)
        assert torch.equal(hso.forward_dh(p, cfg, x, t, None), want)
        assert torch.equal(hso.forward_dh(p, cfg, x, t, torch.zeros_like(h).reshape(1, -1)), want)
        xb = torch.cat([x, 0.5 * x.flip(-1)])
        assert torch.equal(hso.forward_dh(p, cfg, xb, t, None), orc.denoiser(p, cfg, xb, t))
    nlev = len(cfg.ch_mult)
    assert tuple(h.shape) == (1, cfg.ch * cfg.ch_mult[-1], cfg.resolution >> (nlev - 1), cfg.resolution >> (nlev - 1))


def test_cut_at_the_bottleneck_is_the_oracle_forward_conditioned():
    """The DeepFloyd-IF switches: prompt states in the attention blocks, the pooled embedding added to the time embedding, GELU,
    the residual scale, resampling ResBlocks."""
    cfg = K.TINY_IF
    p = orc.to_torch(K.synth_params(cfg, 2))
    g = torch.Generator().manual_seed(11)
    states = torch.randn(1, cfg.context_len, cfg.encoder_dim, generator=g)
    x = torch.randn(2, 3, cfg.resolution, cfg.resolution, generator=g)
    t = torch.tensor(417.0)
    with torch.no_grad():
        ctx, aug = orc.if_text_conditioning(p, cfg, states)
        want = orc.unet_forward_adm(p, cfg, x, t, emb_add=aug, context=ctx)
        assert torch.equal(hso.forward_dh(p, cfg, x, t, None, context=ctx, emb_add=aug), want)
        h = hso.get_h(p, cfg, x[:1], t, context=ctx, emb_add=aug)
        assert torch.equal(hso.h_to_e(p, cfg, x[:1], t, h, context=ctx, emb_add=aug),
                           orc.unet_forward_adm(p, cfg, x[:1], t, emb_add=aug, context=ctx))


def test_restatement_runs_in_float64():
    cfg = K.TINY_DDPM
    p = {k: v.double() for k, v in orc.to_torch(K.synth_params(cfg, 0)).items()}
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    t = torch.tensor(601)
    with torch.no_grad():
        h = hso.get_h(p, cfg, x, t)
        e = hso.h_to_e(p, cfg, x, t, h)
        p32 = orc.to_torch(K.synth_params(cfg, 0))
        e32 = orc.unet_forward(p32, cfg, x.float(), t)
    assert h.dtype == torch.float64 and e.dtype == torch.float64
    assert rel(e32, e) < 1e-5


def test_restatement_matches_the_reference_fixture(golden):
    g = golden("hspace_tiny_ddpm")
    cfg = K.TINY_DDPM
    p = orc.to_torch(K.synth_params(cfg, 0))
    t = torch.tensor(g["t"])
    with torch.no_grad():
        h = hso.get_h(p, cfg, g["x"], t)
        assert rel(h, g["h"]) <= 1e-6
        assert rel(hso.get_h(p, cfg, g["xb"], t), g["hb"]) <= 1e-6
        assert rel(hso.h_to_e(p, cfg, g["x"], t, g["h"]), g["e_at_h"]) <= 1e-6
        assert rel(hso.h_to_e(p, cfg, g["x"], t, g["h"] + g["delta"]), g["e_at_h_delta"]) <= 1e-6
        assert rel(hso.forward_dh(p, cfg, g["xb"], t, g["delta"].reshape(2, -1)), g["forward_u"]) <= 1e-6
        assert rel(hso.forward_dh(p, cfg, g["xb"], t, None), g["forward"]) <= 1e-6
    # the shift reaches the output: the two recorded forwards differ
    assert rel(g["forward_u"], g["forward"]) > 1e-3
    # the recorded solves: k rows, separated singular values, the reference's orientation
    n_in, n_h, k = g["x"][0].numel(), g["h"][0].numel(), g["k"]
    for name, rows in (("enc", n_in), ("dec", n_h), ("x0dec", n_h)):
        r = g[name]
        assert tuple(r["v0"].shape) == (rows, k) and tuple(r["u"].shape) == (n_h, k) and tuple(r["vT"].shape) == (k, n_in)
        s = r["s"].double()
        assert ((s[:-1] - s[1:]) / s[:-1] >= 0.01).all()
    # x0 = (x - sqrt(1 - at) eps) / sqrt(at): same h-space directions, singular values scaled by sqrt(1 - at) / sqrt(at)
    c = ((1 - g["at"]) / g["at"]) ** 0.5
    assert torch.allclose(g["x0dec"]["s"], c * g["dec"]["s"], rtol=1e-3)


def test_jacobian_target_flag_is_refused_where_it_would_be_ignored(monkeypatch):
    from loco_edit_amd.define_argparser import parse_args
    monkeypatch.delenv("LOCO_SOLVER", raising=False)
    base = ["--model_name", "CelebA_HQ_HF", "--dataset_name", "Random"]
    assert parse_args(base).jacobian_target == "x0"
    assert parse_args(base + ["--jacobian_target", "h", "--run_edit_null_space_projection", "True"]).jacobian_target == "h"
    with pytest.raises(ValueError, match="run_edit_null_space_projection only"):
        parse_args(base + ["--jacobian_target", "h", "--group_edit_null_space_projection", "True"])
    with pytest.raises(ValueError, match="unconditional"):
        parse_args(["--model_name", "stabilityai/stable-diffusion-2-1-base", "--jacobian_target", "h",
                    "--run_edit_null_space_projection", "True"])
    with pytest.raises(ValueError, match="power iteration"):
        parse_args(base + ["--jacobian_target", "h", "--run_edit_null_space_projection", "True", "--solver", "krylov"])
    monkeypatch.delenv("LOCO_SOLVER", raising=False)     # (--solver sets it for the process)


@pytest.fixture(scope="module")
def taps(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip(f"HIP headers not found under {ROCM}/include")
    d = tmp_path_factory.mktemp("tap")
    exe = str(d / "program_tap")
    subprocess.run([gxx, "-O1", "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                    os.path.join(ROOT, "loco-edit_amd", "csrc", "program.hip"), os.path.join(ROOT, "tests", "c", "program_tap.cpp"),
                    "-o", exe], check=True)
    names = ["CELEBA_DDPM", "FFHQ_P2", "TINY_DDPM", "TINY_ADM", "TINY_IF", "TINY_LDM", "TINY_DECODER", "TINY_ENCODER", "SD_VAE_DECODER",
             "SD_VAE_ENCODER"]
    path = d / "configs.txt"
    path.write_text("".join(f"{n} {bytes(hip.c_cfg(getattr(K, n), 8)).hex()}\n" for n in names))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        assert f[0] == "TAP"
        out[f[1]] = dict(x.split("=", 1) for x in f[2:])
    assert set(out) == set(names)
    return out


@pytest.mark.parametrize("name,last,nxt", [("CELEBA_DDPM", "mid.block_2", "up."), ("TINY_DDPM", "mid.block_2", "up."),
                                           ("FFHQ_P2", "middle_block.2", "output_blocks.0.0"),
                                           ("TINY_ADM", "middle_block.2", "output_blocks.0.0"),
                                           ("TINY_IF", "middle_block.2", "output_blocks.0.0"),
                                           ("TINY_LDM", "middle_block.2", "output_blocks.0.0")])
def test_program_tap_is_the_middle_blocks_last_output(taps, name, last, nxt):
    cfg, r = getattr(K, name), taps[name]
    nlev = len(cfg.ch_mult)
    C, R = cfg.ch * cfg.ch_mult[-1], cfg.resolution >> (nlev - 1)
    assert r["op"] == last and r["next"].startswith(nxt)
    assert int(r["h_t"]) >= 0 and r["out"] == r["h_t"]              # h_t is the tensor that op writes
    assert int(r["h_last_op"]) >= 0
    assert r["shape"] == f"{C},{R},{R}" and int(r["n_h"]) == C * R * R
    assert r["cat_a_of_next_in"] == "1"                              # ... and the first part of the first up-path concatenation


@pytest.mark.parametrize("name", ["TINY_DECODER", "TINY_ENCODER", "SD_VAE_DECODER", "SD_VAE_ENCODER"])
def test_latent_autoencoder_has_no_tap(taps, name):
    assert taps[name] == {"h_t": "-1", "h_last_op": "-1", "n_h": "0"}
