"""Normalisation numerics under large activation offsets, against a float64 oracle.

Every other parity test runs on synth_params(cfg, 0), whose norm inputs are nearly zero-mean.  Here the weights carry
checkpoint-like channel offsets (tests/norm_offsets.py: max |mean| / std of the conv-fed norm inputs >= 50 "moderate",
>= 1000 "severe", asserted on the CPU by tests/test_norm_offsets_regime.py), where a statistics route that subtracts
mean * sum(d) from sum(x d) loses digits.  The fp32 oracle is no longer a truth there, so the GPU's forward, J V and U^T J
(batch / primal of 1: split-K nearly everywhere; k = 1 and k = 5 probes: the tail-probe split) are compared with the
oracle in float64, and the GPU's error e_gpu is bounded by the error of fp32 arithmetic itself, e_ref = rel(fp32 oracle,
float64) on the same inputs:
  f32, bf16x3: e_gpu <= max(4 e_ref, today's bar)   (bar: TOL[prec] of tests/test_gpu_parity.py; 1.5 TOL for U^T J of the
               denoisers and 5 TOL for the J products of the decoder / SpatialTransformer U-Net, as their parity tests)
  f16:         finite, and each fused statistics route within 2 e(standalone) + 1e-3 of float64 (one f16 product per MAC
               cannot follow fp32 once raw convs read offset inputs: the mode's precision, not a route's error)
Every statistics route meets the bound on its own, one engine per setting: all fusions on, and LOCO_FUSE_LIN /
LOCO_FUSE_STATS / LOCO_FUSE_COT = 0 one at a time."""
import pytest
import torch

import norm_offsets as no
from loco_edit_amd.config import MID_DDPM, TINY_ADM, TINY_DDPM, TINY_DECODER, TINY_LDM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f32": 2e-5, "bf16x3": 1e-4}
CFGS = {"tiny": TINY_DDPM, "mid": MID_DDPM, "tiny_adm": TINY_ADM, "tiny_decoder": TINY_DECODER, "tiny_ldm": TINY_LDM}
ROUTES = [("fused", None), ("LIN=0", "LOCO_FUSE_LIN"), ("STATS=0", "LOCO_FUSE_STATS"), ("COT=0", "LOCO_FUSE_COT")]
LEVELS = ("moderate", "severe")
OUTS = ("fwd", "jv5", "jv1", "vjp5", "vjp1")


def _bar(cfg, prec, out):
    if out == "fwd":
        return TOL[prec]
    if cfg.arch == "dec" or getattr(cfg, "transformer_depth", 0) > 0:
        return 5 * TOL[prec]
    return TOL[prec] * (1.5 if out.startswith("vjp") else 1.0)


def _split(r):
    return {"fwd": r["fwd"], "jv5": r["jv"], "jv1": r["jv"][:1], "vjp5": r["vjp"], "vjp1": r["vjp"][:1]}


def _gpu_legs(eng, cs):
    x = cs["x"].to(DEV)
    fwd = eng.unet_forward(x, cs["t"]).reshape(1, -1)
    eng.pmp_primal(x, cs["t"], cs["at"], cs["mask"].to(DEV), use_et=True)
    V, U = cs["V"].to(DEV), cs["U"].to(DEV)
    out = {"fwd": fwd, "jv5": eng.pmp_jvp(V), "jv1": eng.pmp_jvp(V[:1].contiguous()),
           "vjp5": eng.pmp_vjp(U), "vjp1": eng.pmp_vjp(U[:1].contiguous())}
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("name", list(CFGS))
def test_statistics_routes_under_large_offsets_vs_float64(name, monkeypatch):
    from loco_edit_amd.hip import LocoEngine
    cfg = CFGS[name]
    cs = no.case(cfg)
    prm = {lv: no.offset_params(cfg, lv) for lv in LEVELS}
    ref64, e_ref = {}, {}
    for lv in LEVELS:
        r64 = _split(no.reference(cfg, prm[lv], cs, torch.float64))
        r32 = _split(no.reference(cfg, prm[lv], cs, torch.float32))
        ref64[lv] = r64
        e_ref[lv] = {k: no.rel(r32[k], r64[k]) for k in OUTS}
    e = {}      # (route, level, prec) -> {out: e_gpu}
    finite = True
    for route, env in ROUTES:
        if env:
            monkeypatch.setenv(env, "0")
        for lv in LEVELS:      # (an engine's parameters load once)
            eng = LocoEngine(cfg, max_batch=8, device=torch.device(DEV))
            eng.load_state_dict(prm[lv])
            if cs["ctx"] is not None:
                eng.set_context(cs["ctx"].to(DEV).contiguous())
            for prec in (("f32",) if env is None else ()) + ("bf16x3", "f16"):
                eng.set_precision(prec)
                got = _gpu_legs(eng, cs)
                finite = finite and all(bool(torch.isfinite(v).all()) for v in got.values())
                e[(route, lv, prec)] = {k: no.rel(got[k], ref64[lv][k]) for k in OUTS}
            del eng
            torch.cuda.empty_cache()
        if env:
            monkeypatch.delenv(env)
    fails = []
    print(f"\n[{name}] e_gpu / e_ref per output (e_gpu = rel-L2 vs the float64 oracle; e_ref = the fp32 oracle's)")
    for (route, lv, prec), eg in e.items():
        print(f"  {lv:8s} {prec:6s} {route:8s} " + "  ".join(
            f"{k} {eg[k]:.1e}/{e_ref[lv][k]:.1e}={eg[k] / max(e_ref[lv][k], 1e-30):5.1f}" for k in OUTS))
        for k in OUTS:
            if prec in TOL:
                val, lim, what = eg[k], max(4 * e_ref[lv][k], _bar(cfg, prec, k)), route
            elif route != "fused":      # f16: the fused route against the standalone one of the same switch
                val, lim, what = e[("fused", lv, prec)][k], 2 * eg[k] + 1e-3, "fused vs " + route
            else:
                continue
            if not val <= lim:
                fails.append(f"{lv} {prec} {what} {k}: {val:.2e} > {lim:.2e}")
    assert finite, "non-finite GPU output"
    # Open finding: TINY_ADM at the severe level in bf16x3 is ~13x the fp32 error in EVERY route, the forward included (f32:
    # 0.8x; the four routes agree within 5 %).  Not a statistics route: the split-bf16 arithmetic of the guided-diffusion
    # U-Net on offset activations.  Kept as a strict expected failure so the bound is not loosened and a fix shows up here.
    known = [f for f in fails if name == "tiny_adm" and f.startswith("severe bf16x3 ")]
    assert not [f for f in fails if f not in known], "\n".join(fails)
    if name == "tiny_adm":
        assert known, "the TINY_ADM severe bf16x3 legs now meet the float64 bound: drop the expected failure"
        pytest.xfail("TINY_ADM severe bf16x3 exceeds max(4 e_ref, TOL) in all routes:\n" + "\n".join(known))
