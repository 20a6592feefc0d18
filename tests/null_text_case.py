"""The one null-text inversion case tests/test_gpu_null_text.py and tests/test_null_text_host.py share: `TINY_LDM` under
guidance 7.5, three decode steps of the 100-step schedule, a 4-point trajectory built from seeded latents (each point the
conditional-branch DDIM step of the one before plus 1 % seeded noise, which is what an inverted trajectory looks like from
the decode side), 3 inner steps; and the float64 / fp32 host runs of the optimiser restated in tests/context_grad_oracle.py.
Computed once per session (about two seconds on the host); treat as read-only."""
import functools

import torch

import context_grad_oracle as cgo
import loco_oracle as orc
from loco_edit_amd.config import TINY_LDM, synth_params
from loco_edit_amd.tloco_sd import SDScheduler

SEED, W, INNER, LR, EARLY_STOP = 3, 7.5, 3, 1e-2, 1e-5
FOR_STEPS, T0_IDX, STEPS = 100, 30, 3


@functools.lru_cache(maxsize=None)
def build():
    cfg = TINY_LDM
    params = synth_params(cfg, 0)
    sch = SDScheduler()
    sch.set_timesteps(FOR_STEPS)
    ts = sch.timesteps[T0_IDX:T0_IDX + STEPS]
    alphas = [(sch.alpha_at(t), sch.alpha_at(sch.timesteps_next[sch.index_of(t)])) for t in ts]
    g = torch.Generator().manual_seed(SEED)
    cond = torch.randn(1, cfg.context_len, cfg.context_dim, generator=g)
    null = torch.randn(1, cfg.context_len, cfg.context_dim, generator=g)
    edit = torch.randn(1, cfg.context_len, cfg.context_dim, generator=g)
    p64 = {k: v.double() for k, v in orc.to_torch(params).items()}
    traj = [torch.randn(1, cfg.in_channels, cfg.resolution, cfg.resolution, generator=g)]
    with torch.no_grad():
        for i, t in enumerate(ts):
            e = orc.unet_forward_adm(p64, cfg, traj[-1].double(), torch.tensor(float(t), dtype=torch.float64), context=cond[0].double())
            zp, _ = cgo.ddim_prev(traj[-1].double(), e, *alphas[i])
            traj.append((zp + 0.01 * torch.randn(traj[0].shape, generator=g).double()).float())
    run = lambda dt: cgo.null_text_restatement(cfg, params, traj, [float(t) for t in ts], alphas, null, cond, W, INNER, LR, EARLY_STOP, dt)
    e64, z64, l64, g64 = run(torch.float64)
    e32, z32, l32, _ = run(torch.float32)
    flat = lambda ls: torch.tensor([x for li in ls for x in li], dtype=torch.float64)
    return {"cfg": cfg, "params": params, "timesteps": ts, "traj": traj, "cond": cond, "null": null, "edit": edit,
            "embs64": e64, "zbar64": z64, "losses64": l64, "grads64": g64,
            "yard_embs": cgo.rel(e32, e64), "yard_zbar": cgo.rel(z32, z64), "yard_losses": cgo.rel(flat(l32), flat(l64)),
            "flat": flat}
