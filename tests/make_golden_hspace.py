"""Writes tests/golden/hspace_tiny_ddpm.pt: what the reference's own h-space functions (models/ddpm/diffusion.py:145-345,
484-707) compute on TINY_DDPM with synth_params(cfg, 0), x seeded, t = 601.  Run on a machine that has the reference checkout
(it is imported through oracle/make_golden.py); the tests only read the fixture.

Recorded: get_h; get_h_to_e at h and at h + delta; forward(u) for B = 2; (u, s, vT) of local_encoder_pullback_xt,
local_decoder_pullback_xt and local_x0_decoder_pullback_xt at k = 3 and exactly 3 iterations, each with the Gaussian V0 the
function drew (the generator is re-seeded and the reference's randn repeated).  Neighbouring singular values must differ by
>= 1 % (a nearly degenerate pair has no direction of its own to compare): the next seed is tried otherwise.

    python tests/make_golden_hspace.py
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
import loco_oracle as orc  # noqa: E402
import make_golden as mg  # noqa: E402
from loco_edit_amd.config import TINY_DDPM, synth_params  # noqa: E402

K, N_ITER, T, X_SEED = 3, 3, 601, 3


def separated(s):
    s = s.double()
    return bool(((s[:-1] - s[1:]) / s[:-1] >= 0.01).all())


def solve(fn, n_rows, seed, **kw):
    """fn with the generator seeded; returns (v0 [n_rows, K] as the function drew it, (u, s, vT))."""
    torch.manual_seed(seed)
    v0 = torch.randn(n_rows, K)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn(op='mid', block_idx=0, pca_rank=K, chunk_size=K, min_iter=10, max_iter=N_ITER, convergence_threshold=0, **kw)
    return v0, tuple(o.detach().clone() for o in out)


def main():
    _, _, _, PullBackDDPM = mg.import_reference()
    cfg = TINY_DDPM
    model = mg.ref_model(PullBackDDPM, cfg, synth_params(cfg, 0))
    g = torch.Generator().manual_seed(X_SEED)
    x = torch.randn(1, cfg.in_channels, cfg.resolution, cfg.resolution, generator=g)
    xb = torch.cat([x, torch.randn(1, cfg.in_channels, cfg.resolution, cfg.resolution, generator=g)])
    t = torch.tensor(T)
    at = orc.Scheduler().alpha_at(t).float()
    out = {"x": x, "xb": xb, "t": T, "at": float(at), "k": K, "n_iter": N_ITER}
    with torch.no_grad():
        h = model.get_h(x, t, op='mid', block_idx=0)
        out["h"] = h.clone()
        out["hb"] = model.get_h(xb, t, op='mid', block_idx=0).clone()
        delta = 0.5 * torch.randn(2, *h.shape[1:], generator=g)
        out["delta"] = delta
        out["e_at_h"] = model.get_h_to_e(x, t, input_h=h, op='mid', block_idx=0).clone()
        out["e_at_h_delta"] = model.get_h_to_e(x, t, input_h=h + delta, op='mid', block_idx=0).clone()     # k = 2 rows, one x
        out["forward_u"] = model.forward(xb, t, u=delta.reshape(2, -1), op='mid', block_idx=0).clone()      # B = 2
        out["forward"] = model.forward(xb, t).clone()
    n_in, n_h = x[0].numel(), h[0].numel()
    for name, fn, rows, kw in (("enc", model.local_encoder_pullback_xt, n_in, dict(x=x, t=t)),
                               ("dec", model.local_decoder_pullback_xt, n_h, dict(x=x, t=t)),
                               ("x0dec", model.local_x0_decoder_pullback_xt, n_h, dict(x=x, t=t, at=at))):
        for seed in range(16):
            v0, (u, s, vT) = solve(fn, rows, seed, **kw)
            if separated(s):
                break
        else:
            raise SystemExit(f"{name}: no seed in 0..15 separates the singular values by 1 %")
        print(f"{name}: seed {seed}, s = {[round(float(v), 4) for v in s]}, u {tuple(u.shape)}, vT {tuple(vT.shape)}")
        out[name] = {"seed": seed, "v0": v0, "u": u, "s": s, "vT": vT}
    path = os.path.join(ROOT, "tests", "golden", "hspace_tiny_ddpm.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
