"""Writes tests/golden/hspace_pca_tiny_ddpm.pt (local case) and tests/golden/hspace_pca_tiny_ddpm_global.pt (global case):
what the reference's own ``local_pca_xt`` / ``inv_jac_xt`` / ``global_pca_xt`` (models/ddpm/diffusion.py:347-482) compute on
TINY_DDPM with synth_params(cfg, 0), t = 601.  Run on a machine that has the reference checkout (it is imported through
oracle/make_golden.py); the tests only read the fixtures.  Two files because together they exceed the size limit of a
committed file.

Local: N = 12 samples around the x of tests/golden/hspace_tiny_ddpm.pt (seed 3), memory_bound 4, pca_rank 11.  Recorded: the
noise the function drew (the generator is re-seeded and the reference's randn_like repeated), the sample matrix H [12, n_h]
recomputed from that noise, and (u, s, vT).
Global: 13 inputs, pca_rank 12.  Recorded: x, H, u, s.

With q = N - 1 the range finder of torch.pca_lowrank spans the whole centred row space, so its answer is the exact SVD
whatever it drew: the script checks s against the float64 SVD of H and prints the figure.  Neighbouring singular values on
this model differ by 0.6 - 4 %: ``gap_rows`` marks the rows whose gaps to both neighbours are >= 1 %, and further seeds are
tried until at least the first three rows qualify.

    python tests/make_golden_hspace_pca.py
"""
import contextlib
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import loco_edit_amd  # noqa: E402,F401
import make_golden as mg  # noqa: E402
from loco_edit_amd.config import TINY_DDPM, synth_params  # noqa: E402

T, X_SEED = 601, 3
N_LOCAL, MB, Q_LOCAL = 12, 4, 11
N_GLOBAL, Q_GLOBAL = 13, 12


def gap_rows(s):
    """Row i qualifies when s[i] is >= 1 % away from both neighbours (the last row has none below it)."""
    s = s.double()
    rel = (s[:-1] - s[1:]) / s[:-1]
    up = torch.cat([torch.tensor([True]), rel >= 0.01])
    down = torch.cat([rel >= 0.01, torch.tensor([True])])
    return up & down


def svd_check(H, s, u):
    Hd = H.double()
    U, S, Vh = torch.linalg.svd(Hd - Hd.mean(dim=0), full_matrices=False)
    q = s.numel()
    s_err = float(((s.double() - S[:q]) / S[:q]).abs().max())
    cos = ((u.double() * Vh[:q].T).sum(dim=0)).abs()
    return s_err, cos


def normalize_wrt_batch(x):
    return x / (x.view(x.size(0), -1).norm(dim=-1).view(-1, 1, 1, 1) + 1e-6)


def quiet(fn, **kw):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(**kw)


def main():
    _, _, _, PullBackDDPM = mg.import_reference()
    cfg = TINY_DDPM
    model = mg.ref_model(PullBackDDPM, cfg, synth_params(cfg, 0))
    shape = (cfg.in_channels, cfg.resolution, cfg.resolution)
    x = torch.randn(1, *shape, generator=torch.Generator().manual_seed(X_SEED))
    t = torch.tensor(T)

    for seed in range(32):
        torch.manual_seed(seed)
        noise = torch.cat([torch.randn(MB, *shape) for _ in range(N_LOCAL // MB)])
        torch.manual_seed(seed)
        u, s, vT = quiet(model.local_pca_xt, x=x, t=t, op='mid', block_idx=0, memory_bound=MB, num_pca_samples=N_LOCAL,
                         pca_rank=Q_LOCAL, pca_device='cpu', return_x_direction=True, perturb_h=1e-1)
        ok = gap_rows(s)
        if bool(ok[:3].all()):
            break
    else:
        raise SystemExit("local: no seed in 0..31 separates the first three singular values by 1 %")
    with torch.no_grad():
        H = torch.cat([model.get_h(x + normalize_wrt_batch(noise[i:i + MB]), t, op='mid', block_idx=0) for i in range(0, N_LOCAL, MB)])
    H = H.reshape(N_LOCAL, -1).float().clone()
    s_err, cos = svd_check(H, s, u)
    print(f"local: seed {seed}, s = {[round(float(v), 4) for v in s]}\n  gap rows {ok.tolist()}\n  s vs float64 SVD {s_err:.2e}, "
          f"min |cos| {float(cos.min()):.7f}; u {tuple(u.shape)}, vT {tuple(vT.shape)}")
    local = {"x": x, "t": T, "seed": seed, "memory_bound": MB, "pca_rank": Q_LOCAL, "perturb_h": 1e-1, "noise": noise, "H": H,
             "u": u.detach().clone(), "s": s.detach().clone(), "vT": vT.detach().clone(), "gap_rows": ok}
    path = os.path.join(ROOT, "tests", "golden", "hspace_pca_tiny_ddpm.pt")
    torch.save(local, path)
    print("wrote", path, os.path.getsize(path), "bytes")

    for seed in range(32):
        xs = torch.randn(N_GLOBAL, *shape, generator=torch.Generator().manual_seed(100 + seed))
        torch.manual_seed(seed)
        u, s = quiet(model.global_pca_xt, x=xs, t=t, op='mid', block_idx=0, memory_bound=MB, pca_rank=Q_GLOBAL, pca_device='cpu')
        ok = gap_rows(s)
        if bool(ok[:3].all()):
            break
    else:
        raise SystemExit("global: no seed in 0..31 separates the first three singular values by 1 %")
    with torch.no_grad():
        H = model.get_h(xs, t, op='mid', block_idx=0).reshape(N_GLOBAL, -1).float().clone()
    s_err, cos = svd_check(H, s, u)
    print(f"global: seed {seed}, s = {[round(float(v), 4) for v in s]}\n  gap rows {ok.tolist()}\n  s vs float64 SVD {s_err:.2e}, "
          f"min |cos| {float(cos.min()):.7f}; u {tuple(u.shape)}")
    glob = {"x": xs, "t": T, "seed": seed, "memory_bound": MB, "pca_rank": Q_GLOBAL, "H": H, "u": u.detach().clone(),
            "s": s.detach().clone(), "gap_rows": ok}
    path = os.path.join(ROOT, "tests", "golden", "hspace_pca_tiny_ddpm_global.pt")
    torch.save(glob, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
