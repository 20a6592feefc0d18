"""Checkpoint-like weights for the normalisation tests: `synth_params` plus large activation offsets.

`synth_params` draws conv / linear biases of 0.05 N, so every GroupNorm and LayerNorm input the other tests see is nearly
zero-mean.  Trained checkpoints carry channel offsets that are large next to a group's spread (the Stable Diffusion VAE
decoder is the known extreme), which is where a statistics route that forms sum(x d) - mean sum(d) loses its digits.
`offset_params` adds, to the bias of every conv feeding a norm directly, an offset that is constant within each of that
norm's groups (+-c, varying from group to group), and a constant c to the stem conv's bias, which the residual stream then
carries into every block (so the raw convs read offset inputs too).  Deterministic: no random draws.

Per architecture (parameter names of config.param_shapes):
  ddpm / dec: `*.conv1` -> `*.norm2`;                               stem `conv_in`
  adm:        `*.in_layers.2` -> `*.out_layers.0`;                  stem `input_blocks.0.0`
  LDM transformer (adm with transformer_depth): `*.proj_in` -> the block's first LayerNorm (one group: all channels).
`regime` hooks F.group_norm / F.layer_norm during a forward of the oracle and reports |mean| / std per norm.
"""
from __future__ import annotations

import contextlib
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

import loco_oracle as orc
from loco_edit_amd.config import synth_params

# offset scale c per level: "moderate" reaches max |mean| / std >= 50 over the norms fed by a conv,
# "severe" >= 1000 (asserted by tests/test_norm_offsets_regime.py, not assumed)
# and the fp32 oracle's own error against float64 grows >= 10x from c = 0 to "severe"
LEVELS = {"zero": 0.0, "moderate": 10.0, "severe": 250.0}


def _group_offsets(C: int, G: int, c: float) -> np.ndarray:
    """[C] offsets, constant within each of G contiguous groups: c * (+1, -1.5, +2, -1, +1.5, -2, ...)."""
    mag = (1.0, 1.5, 2.0)
    per = np.array([c * mag[g % 3] * (1.0 if g % 2 == 0 else -1.0) for g in range(G)], dtype=np.float64)
    return np.repeat(per, C // G)


def _conv_fed_norms(cfg, names):
    """(producer bias, consumer norm weight or None for a LayerNorm over all channels) pairs of the architecture."""
    arch = getattr(cfg, "arch", "ddpm")
    pairs = []
    for n in names:
        if arch in ("ddpm", "dec") and n.endswith(".conv1.bias"):
            pairs.append((n, n[:-len(".conv1.bias")] + ".norm2.weight"))
        elif arch == "adm" and n.endswith(".in_layers.2.bias"):
            pairs.append((n, n[:-len(".in_layers.2.bias")] + ".out_layers.0.weight"))
        elif arch == "adm" and n.endswith(".proj_in.bias"):
            pairs.append((n, None))
    return pairs


def conv_fed_norm_names(cfg, p) -> set:
    """Names of the norms whose input is a conv output (the ones the offsets are built for)."""
    out = set()
    for _, nw in _conv_fed_norms(cfg, list(p)):
        if nw is not None:
            out.add(nw[:-len(".weight")])
    if getattr(cfg, "transformer_depth", 0) > 0:
        out |= {n[:-len(".weight")] for n in p if n.endswith(".transformer_blocks.0.norm1.weight")}
    return out


def offset_params(cfg, level: str, seed: int = 0) -> Dict[str, np.ndarray]:
    """synth_params(cfg, seed) with the offsets of LEVELS[level] (zero: the same arrays)."""
    p = synth_params(cfg, seed)
    c = LEVELS[level]
    if c == 0:
        return p
    G = cfg.gn_groups
    out = dict(p)
    for bn, nw in _conv_fed_norms(cfg, list(p)):
        C = p[bn].shape[0]
        off = _group_offsets(C, G, c) if nw is not None else np.full(C, c)
        out[bn] = (p[bn].astype(np.float64) + off).astype(np.float32)
    stem = "conv_in.bias" if "conv_in.bias" in p else "input_blocks.0.0.bias"
    out[stem] = (p[stem].astype(np.float64) + c).astype(np.float32)
    return out


@contextlib.contextmanager
def regime(p: Dict[str, torch.Tensor]):
    """Within the block, every F.group_norm / F.layer_norm call whose weight is one of p's tensors records
    max over (sample, group) of |mean| / std of its input into the yielded dict, keyed by the norm's name."""
    names = {id(v): k[:-len(".weight")] for k, v in p.items() if k.endswith(".weight")}
    seen: Dict[str, float] = {}
    gn0, ln0 = F.group_norm, F.layer_norm

    def note(w, x):
        name = names.get(id(w))
        if name is None:
            return
        x = x.detach().double()
        m, s = x.mean(-1), x.std(-1, unbiased=False)
        seen[name] = max(seen.get(name, 0.0), float((m.abs() / s.clamp_min(1e-30)).max()))

    def gn(x, G, weight=None, bias=None, eps=1e-5):
        note(weight, x.reshape(x.shape[0], G, -1))
        return gn0(x, G, weight, bias, eps)

    def ln(x, shape, weight=None, bias=None, eps=1e-5):
        note(weight, x.reshape(-1, int(np.prod(shape))))
        return ln0(x, shape, weight, bias, eps)
    F.group_norm, F.layer_norm = gn, ln
    try:
        yield seen
    finally:
        F.group_norm, F.layer_norm = gn0, ln0


def to_torch(params, dtype=torch.float32) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype) for k, v in orc.to_torch(params).items()}


# ------------------------------------------------------------------ the products the GPU tests compare, on the CPU
T_IDX = 40          # timestep index of the 100-step schedule (the parity tests' linearisation point)


def case(cfg, seed: int = 3):
    """Seeded inputs of one leg: x [1, C, R, R], t, at, output mask, V [5, n], cotangents U [5, n_out] (masked),
    context states or None.  The operator is eps for every architecture: the x0 estimate (x - sqrt(1 - at) eps) / sqrt(at)
    carries an identity term that would dilute the network's error."""
    s = orc.Scheduler()
    s.set_timesteps(100)
    t = float(s.timesteps[T_IDX]); at = float(s.alpha_at(s.timesteps[T_IDX]))
    gen = torch.Generator().manual_seed(seed)
    R, Ro = cfg.resolution, cfg.out_resolution
    x = torch.randn(1, cfg.in_channels, R, R, generator=gen)
    mask = torch.zeros(cfg.out_ch, Ro, Ro, dtype=torch.bool); mask[:, Ro // 3:Ro // 2, Ro // 4:Ro // 2] = True
    V = torch.randn(5, cfg.n, generator=gen)
    U = torch.randn(5, cfg.n_out, generator=gen) * mask.reshape(1, -1)
    ctx = torch.randn(cfg.context_len, cfg.context_dim, generator=gen) if cfg.context_dim else None
    return dict(x=x, t=t, at=at, mask=mask, V=V, U=U, ctx=ctx)


def operator(cfg, p, cs):
    """x -> the network output (eps; the decoder's image) whose Jacobian products the engine computes with use_et."""
    t = torch.tensor(cs["t"])
    if cfg.arch == "dec":
        return lambda x: orc.decoder_forward(p, cfg, x)
    if cfg.arch == "adm":
        ctx = None if cs["ctx"] is None else cs["ctx"].to(next(iter(p.values())).dtype)
        return lambda x: orc.unet_forward_adm(p, cfg, x, t, context=ctx)
    return lambda x: orc.unet_forward(p, cfg, x, t)


def reference(cfg, params, cs, dtype):
    """forward [1, n_out], J V [5, n_out] (masked) and U^T J [5, n] of the oracle in `dtype`."""
    p = to_torch(params, dtype)
    f = operator(cfg, p, cs)
    x = cs["x"].to(dtype)
    m = cs["mask"].reshape(1, -1).to(dtype)
    with torch.no_grad():
        y = f(x).reshape(1, -1)
    V = cs["V"].to(dtype)
    JV = torch.stack([torch.func.jvp(f, (x,), (v.view_as(x),))[1].reshape(-1) for v in V]) * m
    xx = x.clone().requires_grad_(True)
    out = f(xx).reshape(-1)
    U = cs["U"].to(dtype)
    UJ = torch.stack([torch.autograd.grad(out, xx, u, retain_graph=True)[0].reshape(-1) for u in U])
    return dict(fwd=y, jv=JV, vjp=UJ)


def rel(a, b) -> float:
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
