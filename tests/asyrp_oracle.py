"""Plain torch restatement of the Asyrp block f_t (csrc/asyrp.hip), of its Adam step, of the directional CLIP
loss and of the asymmetric DDIM step (loco_edit_amd/asyrp.py), for float64 and fp32 CPU runs.  Gradients come from torch
autograd; ``block_backward`` restates them by hand (the formulas the HIP unit implements) and tests/test_asyrp_oracle_host.py
holds the two against each other.  Nothing here reads the HIP library.

    a1 = swish(GroupNorm32(h; g1, b1));   y1 = W1 a1 + c1 + (Wt swish(e) + ct)[:, None, None]
    a2 = swish(GroupNorm32(y1; g2, b2));  dh = s (W2 a2 + c2)
"""
import torch
import torch.nn.functional as F

PARAMS = ("g1", "b1", "W1", "c1", "Wt", "ct", "g2", "b2", "W2", "c2")
GROUPS = 32


def swish(x):
    return x * torch.sigmoid(x)


def swish_der(x):
    sg = torch.sigmoid(x)
    return sg * (1 + x * (1 - sg))


def param_shapes(C, E):
    return {"g1": (C,), "b1": (C,), "W1": (C, C), "c1": (C,), "Wt": (C, E), "ct": (C,), "g2": (C,), "b2": (C,), "W2": (C, C), "c2": (C,)}


def random_params(C, E, seed, dtype=torch.float32):
    """Every parameter away from its initial value (gains near 1, W2 / c2 non-zero), so that no gradient is trivially zero."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in param_shapes(C, E).items():
        r = torch.randn(s, generator=gen, dtype=torch.float64)
        if k in ("g1", "g2"):
            v = 1 + 0.2 * r
        elif len(s) == 2:
            v = r / s[1] ** 0.5
        else:
            v = 0.3 * r
        sd[k] = v.to(torch.float32).to(dtype)      # fp32 values in either dtype: both runs and the device start from the same numbers
    return sd


def block_forward(p, h, e, s=1.0, eps=1e-6):
    """dh [B, C, H, W] in the dtype of the arguments."""
    C = h.shape[1]
    a1 = swish(F.group_norm(h, GROUPS, p["g1"], p["b1"], eps))
    tb = p["Wt"] @ swish(e) + p["ct"]
    y1 = torch.einsum("oc,bchw->bohw", p["W1"], a1) + p["c1"].view(1, C, 1, 1) + tb.view(1, C, 1, 1)
    a2 = swish(F.group_norm(y1, GROUPS, p["g2"], p["b2"], eps))
    return s * (torch.einsum("oc,bchw->bohw", p["W2"], a2) + p["c2"].view(1, C, 1, 1))


def block_grads(p, h, e, g_dh, s=1.0, eps=1e-6):
    """(dh, g_h, {name: gradient}) for the cotangent g_dh, by autograd."""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    hh = h.detach().clone().requires_grad_(True)
    dh = block_forward(q, hh, e, s, eps)
    grads = torch.autograd.grad(dh, [hh] + [q[k] for k in PARAMS], grad_outputs=g_dh)
    return dh.detach(), grads[0], dict(zip(PARAMS, grads[1:]))


def _gn_parts(x, gamma, beta, eps):
    B, C = x.shape[:2]
    xg = x.reshape(B, GROUPS, -1)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xh = ((xg - mean) * rstd).reshape(x.shape)
    y = gamma.view(1, C, 1, 1) * xh + beta.view(1, C, 1, 1)
    return xh, rstd, y


def _gn_swish_backward(ga, x, gamma, beta, eps):
    """Cotangents (g_x, g_gamma, g_beta) of a = swish(GroupNorm32(x; gamma, beta)) for the cotangent ga of a."""
    B, C = x.shape[:2]
    xh, rstd, y = _gn_parts(x, gamma, beta, eps)
    d = swish_der(y) * ga
    z = (gamma.view(1, C, 1, 1) * d).reshape(B, GROUPS, -1)
    xhg = xh.reshape(B, GROUPS, -1)
    m1 = z.mean(dim=2, keepdim=True)
    m2 = (z * xhg).mean(dim=2, keepdim=True)
    gx = (rstd * (z - m1 - xhg * m2)).reshape(x.shape)
    return gx, (d * xh).sum(dim=(0, 2, 3)), d.sum(dim=(0, 2, 3))


def block_backward(p, h, e, g_dh, s=1.0, eps=1e-6):
    """(g_h, {name: gradient}) by the hand-written formulas of csrc/asyrp.hip."""
    C = h.shape[1]
    a1 = swish(F.group_norm(h, GROUPS, p["g1"], p["b1"], eps))
    se = swish(e)
    y1 = torch.einsum("oc,bchw->bohw", p["W1"], a1) + (p["c1"] + p["Wt"] @ se + p["ct"]).view(1, C, 1, 1)
    a2 = swish(F.group_norm(y1, GROUPS, p["g2"], p["b2"], eps))
    g = {}
    go = s * g_dh
    g["c2"] = go.sum(dim=(0, 2, 3))
    g["W2"] = torch.einsum("bohw,bchw->oc", go, a2)
    ga2 = torch.einsum("oc,bohw->bchw", p["W2"], go)
    gy1, g["g2"], g["b2"] = _gn_swish_backward(ga2, y1, p["g2"], p["b2"], eps)
    g["c1"] = gy1.sum(dim=(0, 2, 3))
    g["ct"] = g["c1"].clone()
    g["Wt"] = torch.outer(g["c1"], se)
    g["W1"] = torch.einsum("bohw,bchw->oc", gy1, a1)
    ga1 = torch.einsum("oc,bohw->bchw", p["W1"], gy1)
    gh, g["g1"], g["b1"] = _gn_swish_backward(ga1, h, p["g1"], p["b1"], eps)
    return gh, g


class Adam:
    """torch.optim.Adam's arithmetic (no weight decay, no amsgrad) on a dict of tensors, in their dtype."""

    def __init__(self, params, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        self.p = {k: v.detach().clone() for k, v in params.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.lr, self.beta1, self.beta2, self.eps, self.t = lr, beta1, beta2, eps, 0

    def step(self, grads):
        self.t += 1
        bc1, bc2 = 1 - self.beta1 ** self.t, 1 - self.beta2 ** self.t
        for k, g in grads.items():
            self.m[k] = self.beta1 * self.m[k] + (1 - self.beta1) * g
            self.v[k] = self.beta2 * self.v[k] + (1 - self.beta2) * g * g
            self.p[k] = self.p[k] - (self.lr / bc1) * self.m[k] / (self.v[k].sqrt() / bc2 ** 0.5 + self.eps)
        return self.p


def train_quadratic(p0, h, e, target, steps, lr, s=1.0, eps=1e-6):
    """`steps` Adam steps on L = 0.5 |f_t(h, e) - target|^2 (the cotangent of dh is dh - target); returns the parameters."""
    opt = Adam(p0, lr)
    for _ in range(steps):
        dh = block_forward(opt.p, h, e, s, eps)
        _, _, grads = block_grads(opt.p, h, e, (dh - target).detach(), s, eps)
        opt.step(grads)
    return opt.p


DIR_EPS = 1e-7


def directional_loss(emb_edit, emb_src, text_src, text_tgt):
    """1 - <d / (|d| + DIR_EPS), dt / |dt|> with d = emb_edit - emb_src, dt = text_tgt - text_src; differentiable for d != 0."""
    d, dt = emb_edit - emb_src, (text_tgt - text_src).to(emb_edit.dtype)
    return 1 - (d / (d.norm() + DIR_EPS)) @ (dt / dt.norm())


def asym_step(x, eps_edit, eps_src, at, at_next):
    """x_t' = sqrt(a') P_t(eps_edit) + sqrt(1 - a') eps_src, P_t(e) = (x - sqrt(1 - a) e) / sqrt(a)."""
    x0 = (x - (1 - at) ** 0.5 * eps_edit) / at ** 0.5
    return at_next ** 0.5 * x0 + (1 - at_next) ** 0.5 * eps_src


def time_vector(cfg, t, dtype=torch.float64):
    """The sinusoid of the denoiser's own first stage at width cfg.temb_ch (oracle/loco_oracle.py's two conventions)."""
    import loco_oracle as orc
    fn = orc.timestep_embedding if cfg.arch == "ddpm" else orc.timestep_embedding_adm
    return fn(torch.tensor([float(t)], dtype=torch.float64), cfg.temb_ch, torch.float64)[0].to(dtype)


def chain_step(net_p, cfg, vsd, vcfg, block_p, x, t, at, at_next, text_src, text_tgt, clip_weight, rec_weight, dtype=torch.float64):
    """One training step of loco_edit_amd/asyrp.py under autograd, every tensor in `dtype`: tests/hspace_oracle.py (the network to and
    from h) -> the losses through tests/clip_grad_oracle.py -> this file's block.  Returns (loss, l_dir, l_rec, {name: d loss / d
    parameter}, x_t' of the asymmetric step, dh)."""
    import clip_grad_oracle as cgo
    import hspace_oracle as hso
    net = {k: v.to(dtype) for k, v in net_p.items()}
    q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in block_p.items()}
    x, tt = x.to(dtype), torch.tensor(float(t))
    with torch.no_grad():
        eps = hso.forward_dh(net, cfg, x, tt, None)
        h = hso.get_h(net, cfg, x, tt)
    dh = block_forward(q, h, time_vector(cfg, t, dtype), 1.0, cfg.gn_eps)
    eps_edit = hso.h_to_e(net, cfg, x, tt, h + dh)
    x0_edit = (x - (1 - at) ** 0.5 * eps_edit) / at ** 0.5
    x0_src = (x - (1 - at) ** 0.5 * eps) / at ** 0.5
    pv = cgo.preprocess_windows(torch.cat([x0_edit, x0_src]), None, vcfg.image_size, vcfg.image_mean, vcfg.image_std).to(dtype)
    emb = cgo.clip_vision_embeds(vsd, vcfg, pv, dtype)
    l_dir = directional_loss(emb[0], emb[1].detach(), text_src.to(dtype), text_tgt.to(dtype))
    l_rec = (x0_edit - x0_src).abs().mean()
    loss = clip_weight * l_dir + rec_weight * l_rec
    grads = torch.autograd.grad(loss, [q[k] for k in PARAMS])
    x_next = asym_step(x, eps_edit.detach(), eps, at, at_next)
    return loss.detach(), l_dir.detach(), l_rec.detach(), dict(zip(PARAMS, grads)), x_next, dh.detach()


def rel_err(a, ref64):
    """max |a - ref| / max |ref| in double."""
    return float((a.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))
