"""h-space PCA baselines on the device: global PCA of the bottleneck ``h`` over many samples and local PCA of ``h`` around
one ``x_t`` (the reference's ``inv_jac_xt`` / ``local_pca_xt`` / ``global_pca_xt``, ``models/ddpm/diffusion.py:347-482``).

The reference moves every ``h`` to the CPU and calls ``torch.pca_lowrank`` there; here the samples go from ``get_h`` straight
into the store of ``hip.LocoPca`` and the randomized PCA (csrc/pca.hip) runs on the card that produced them.  The algorithm
is ``torch.pca_lowrank``'s family with CholeskyQR2 as the orthonormalisation; the random test matrix is drawn here from the
caller's generator, so a result is a deterministic function of the samples and the generator's state.
"""
from __future__ import annotations

from typing import Optional

import torch

from .hip import LocoPca


def draw_omega(d: int, q: int, generator: Optional[torch.Generator], device) -> torch.Tensor:
    """The Gaussian test matrix ``[d, q]`` (fp32) from ``generator`` (on its own device; ``None``: the global CPU generator)."""
    gdev = generator.device if generator is not None else torch.device("cpu")
    return torch.randn(d, q, generator=generator, device=gdev, dtype=torch.float32).to(device)


def pca_lowrank_device(H_or_store, q: int, niter: int = 2, generator: Optional[torch.Generator] = None, center: bool = True):
    """``(s [q], V [D, q], mean [D])`` of a sample matrix ``H [N, D]`` (a device tensor, fp32) or of a ``LocoPca`` store that
    already holds the rows.  ``s`` are the singular values of the centred matrix as ``torch.pca_lowrank`` returns them (no
    ``1 / sqrt(N - 1)``); the columns of ``V`` have their entry of largest magnitude positive."""
    if isinstance(H_or_store, LocoPca):
        store = H_or_store
    else:
        H = H_or_store
        if not isinstance(H, torch.Tensor) or H.dim() != 2:
            raise ValueError("pca_lowrank_device: expected a sample matrix [N, D] or a LocoPca store")
        if not H.is_cuda:
            raise ValueError("pca_lowrank_device: the sample matrix must be a device tensor (there is no CPU path)")
        if H.dtype != torch.float32:
            raise ValueError(f"pca_lowrank_device: expected torch.float32, got {H.dtype}")
        if H.shape[0] < 2:
            raise ValueError("pca_lowrank_device: need at least two samples")
        store = LocoPca(H.shape[0], H.shape[1], min(int(q), LocoPca.Q_LIMIT) if q >= 1 else 1, device=H.device)
        store.add_rows(H)
    omega = draw_omega(store.d, int(q), generator, store.device)
    return store.fit(int(q), int(niter), omega, center=center)


def sample_h(engine, xs: torch.Tensor, t: float, store: Optional[LocoPca] = None, q_max: int = 1) -> LocoPca:
    """``get_h`` of every row of ``xs [N, C, R, R]``, ``engine.max_batch`` rows at a time, appended to ``store`` (created for
    exactly N rows when ``None``)."""
    n = xs.shape[0]
    if store is None:
        store = LocoPca(n, engine.n_h, q_max, device=engine.device)
    mb = engine.max_batch
    for b0 in range(0, n, mb):
        xb = xs[b0:b0 + mb].to(device=engine.device, dtype=torch.float32).contiguous()
        store.add_rows(engine.get_h(xb, float(t)).reshape(xb.shape[0], -1))
    return store


def normalize_wrt_batch(x: torch.Tensor) -> torch.Tensor:
    """x / (||x|| + 1e-6) per sample (the reference's helper of the same name)."""
    nrm = x.reshape(x.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (x.dim() - 1)))
    return x / (nrm + 1e-6)


@torch.no_grad()
def decode_with_dh(ed, xt: torch.Tensor, t_start_idx: int, dh: Optional[torch.Tensor], performance_boosting: bool = False,
                   noises=None) -> torch.Tensor:
    """DDIM decode of ``xt [B, C, R, R]`` from step ``t_start_idx`` of ``ed``'s forward schedule to x0 with ``dh [B, n_h]`` added
    to the bottleneck at every remaining step (``None``: the same loop over the plain forward).  The schedule and the eta rule
    are those of ``EditUncondDiffusion.DDIMforwardsteps``: eta = 1 from ``performance_boosting_t_idx`` on when
    ``performance_boosting``, else 0; ``noises`` ({step index: tensor}) injects the eta = 1 draws.  With eta = 0 a frame decoded
    alone is bit-identical to its row of a batch (see the loop)."""
    eng, sch = ed.engine, ed.scheduler
    sch.set_timesteps(ed.for_steps, device=ed.device)
    timesteps = sch.timesteps
    xt = xt.to(device=ed.device, dtype=torch.float32).contiguous()
    if dh is not None:
        dh = dh.to(device=ed.device, dtype=torch.float32).reshape(xt.shape[0], -1).contiguous()
    mb = eng.max_batch
    pb = ed.performance_boosting_t_idx
    for i, t in enumerate(timesteps):
        if i < t_start_idx:
            continue
        eta = 1.0 if (performance_boosting and pb <= i and pb != len(timesteps) - 1) else 0.0
        nz = None
        if eta != 0:
            nz = (torch.randn_like(xt) if noises is None else noises[i].to(device=ed.device, dtype=torch.float32)).contiguous()
        t_next = sch.timesteps_next[sch.index_of(t)]
        at, at_next = sch.alpha_at(t), sch.alpha_at(t_next)
        out = torch.empty_like(xt)
        for b0 in range(0, xt.shape[0], mb):
            # every launch carries exactly max_batch rows (a short chunk repeats its last row): the engine picks its conv
            # tiling by the batch size, so only then is a frame's arithmetic the same alone and inside a walk
            idx = torch.arange(b0, b0 + mb, device=xt.device).clamp_max(xt.shape[0] - 1)
            b = min(mb, xt.shape[0] - b0)
            xb = xt[idx].contiguous()
            et = eng.unet_forward(xb, float(t), dh=None if dh is None else dh[idx].contiguous())
            out[b0:b0 + b] = eng.sched_step(xb, et, at, at_next, eta, None if nz is None else nz[idx].contiguous())[0][:b]
        xt = out
    return xt
