"""CPU restatement of the latent-consistency path (tests of loco_edit_amd.tloco_lcm; not a test module itself).

Written from the published ``LCMScheduler`` / ``LatentConsistencyModelPipeline`` / ``UNet2DConditionModel`` of diffusers (not
installed here; the reference pins a version that predates them -- unpinned), on top of the oracle's networks:

* the scheduler's formulas in float64;
* the U-Net with ``timestep_cond`` through the identity  linear(emb + c, W, b) = linear(emb, W, b + W c):
  ``orc.unet_forward_adm`` with ``time_embed.0.bias`` replaced by ``b + W0 (Wc w_emb)`` formed in float64 -- no copy of the
  network;
* ``x0_hat(z) = decoder((c_skip z + c_out (z - sigma eps(z)) / sqrt(a)) / 0.18215)`` on ``orc.decoder_forward``.
"""
import math

import torch

import loco_oracle as orc

LATENT_SCALE = 0.18215


# ------------------------------------------------------------------ scheduler
def timesteps(n, rule, original=50, train=1000):
    """linspace: the descending training timesteps indexed at floor(i * 50 / n); stride: origin[::-(50 // n)][:n]."""
    k = train // original
    origin = [j * k - 1 for j in range(1, original + 1)]
    if rule == "stride":
        return origin[::-(original // n)][:n]
    desc = origin[::-1]
    return [desc[(i * original) // n] for i in range(n)]


def alphas_cumprod():
    """scaled_linear 0.00085 .. 0.012 over 1000 steps, float32 (the table of every SD v1 pipeline)."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def scalings(t, timestep_scaling=10.0, sigma_data=0.5):
    """(c_skip, c_out) in float64."""
    s = float(t) * timestep_scaling
    return sigma_data ** 2 / (s ** 2 + sigma_data ** 2), s / math.sqrt(s ** 2 + sigma_data ** 2)


def lcm_step(x, eps, at, at_prev, c_skip, c_out, noise=None):
    """-> (prev, denoised) in the dtype of x (float64 inputs: the truth; float32 inputs: torch's own composition)."""
    at, at_prev = torch.as_tensor(at, dtype=x.dtype), torch.as_tensor(at_prev, dtype=x.dtype)
    c_skip, c_out = torch.as_tensor(c_skip, dtype=x.dtype), torch.as_tensor(c_out, dtype=x.dtype)
    x0 = (x - (1 - at).sqrt() * eps) / at.sqrt()
    den = c_out * x0 + c_skip * x
    prev = den if noise is None else at_prev.sqrt() * den + (1 - at_prev).sqrt() * noise
    return prev, den


def guidance_embedding(w, dim):
    """get_guidance_scale_embedding: w * 1000, half = dim // 2, exp(arange(half) * -log(10000) / (half - 1)), [sin, cos],
    zero pad for odd dim; float32."""
    w = torch.tensor([float(w)], dtype=torch.float32) * 1000.0
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32) * -(torch.log(torch.tensor(10000.0)) / (half - 1)))
    a = w[:, None] * f[None, :]
    e = torch.cat([torch.sin(a), torch.cos(a)], dim=1)
    if dim % 2 == 1:
        e = torch.nn.functional.pad(e, (0, 1))
    return e[0]


# ------------------------------------------------------------------ networks
def fold_cond(p, w_emb):
    """Parameters of the U-Net with `timestep_cond` = w_emb folded into the first dense layer's bias (formed in float64)."""
    q = dict(p)
    W0, b0, Wc = p["time_embed.0.weight"].double(), p["time_embed.0.bias"].double(), p["time_embed.cond_proj.weight"].double()
    q["time_embed.0.bias"] = (b0 + W0 @ (Wc @ w_emb.double())).to(p["time_embed.0.bias"].dtype)
    return q


class LCMRestatement:
    def __init__(self, p, cfg, dp, dcfg, w, steps=4, rule="linspace", timestep_scaling=10.0):
        self.p, self.cfg, self.dp, self.dcfg = p, cfg, dp, dcfg
        self.w_emb = guidance_embedding(w, cfg.time_cond_proj_dim)
        self.pc = fold_cond(p, self.w_emb)
        self.ts = timesteps(steps, rule)
        self.ab = alphas_cumprod()
        self.timestep_scaling = timestep_scaling

    def eps(self, z, ctx, t):
        return orc.unet_forward_adm(self.pc, self.cfg, z, torch.tensor(float(t)), context=ctx)

    def coeffs(self, t):
        c_skip, c_out = scalings(t, self.timestep_scaling)
        return float(self.ab[int(t)]), c_skip, c_out

    def denoised(self, z, ctx, t):
        at, c_skip, c_out = self.coeffs(t)
        return lcm_step(z, self.eps(z, ctx, t), at, 1.0, c_skip, c_out)[1]

    def decode(self, z_scaled):
        return orc.decoder_forward(self.dp, self.dcfg, z_scaled)

    def x0_hat(self, z, ctx, t, mask=None, flatten=False):
        x0 = self.decode(self.denoised(z, ctx, t) / LATENT_SCALE)
        if mask is not None:
            return x0[:, mask]
        return x0.reshape(x0.shape[0], -1) if flatten else x0

    @torch.no_grad()
    def forward_loop(self, z, ctx, noise, t_start_idx=0, t_end_idx=-1):
        """LCMforwardsteps with the noise of every step given: -> (latents, t, t_idx) at t_end_idx, else
        (latents, denoised, image in [0, 1])."""
        den = None
        for i, t in enumerate(self.ts):
            if i < t_start_idx:
                continue
            if i != t_start_idx and i == t_end_idx:
                return z, t, i
            at, c_skip, c_out = self.coeffs(t)
            last = i == len(self.ts) - 1
            at_prev = 1.0 if last else float(self.ab[self.ts[i + 1]])
            z, den = lcm_step(z, self.eps(z, ctx, t), at, at_prev, c_skip, c_out, None if last else noise[i])
        return z, den, (self.decode(den / LATENT_SCALE) / 2 + 0.5).clamp(0, 1)

    def pullback(self, z, ctx, t, pca_rank, v0, n_iter, mask):
        """edit.py:283-369 with V0 injected and a fixed iteration count."""
        c, hh, ww = z.shape[1:]
        n = c * hh * ww
        a = torch.tensor(0.0)
        v = torch.linalg.qr(v0.float())[0].T.reshape(-1, c, hh, ww)
        for _ in range(n_iter):
            g = lambda al: self.x0_hat(z + al * v, ctx, t, mask=mask)
            u = torch.func.jacfwd(g, argnums=0, randomness="error")(a).detach()
            g2 = lambda z_: torch.einsum("bl,il->b", u, self.x0_hat(z_, ctx, t, mask=mask))
            v_ = torch.autograd.functional.jacobian(g2, z).reshape(-1, n).float()
            _, s, v = torch.linalg.svd(v_, full_matrices=False)
            v = v.reshape(-1, c, hh, ww)
        return u.reshape(u.shape[0], -1).T.detach(), s.sqrt().detach(), v.reshape(-1, n).detach()

    def delta_zt_via_grad(self, z, ctx_for, ctx_edit, t, mask):
        """edit.py:250-280: the image difference through the VJP of the EDIT-prompt Jacobian, unit rows."""
        with torch.no_grad():
            d = self.x0_hat(z, ctx_edit, t) - self.x0_hat(z, ctx_for, t)
        dflat = d[:, mask]
        g = lambda v: torch.sum(dflat * self.x0_hat(v, ctx_edit, t, mask=mask))
        v_ = torch.autograd.functional.jacobian(g, z).reshape(-1, z[0].numel())
        return v_ / v_.norm(dim=1, keepdim=True)
