"""CPU: the float64 restatement of the device PCA (tests/pca_oracle.py) against torch.linalg.svd, torch.pca_lowrank and the
reference's own h-space PCA functions (tests/golden/hspace_pca_tiny_ddpm*.pt, written by tests/make_golden_hspace_pca.py), and
a float64 restatement of ``inv_jac_xt`` by autograd through tests/hspace_oracle.py against the fixture's ``vT``.

Bars: the oracle at niter = 2 on a geometric spectrum reproduces the top KEEP = 5 singular pairs of the centred matrix to 1e-9
(s relative, 1 - |cos|): what the range finder leaves after 2 niter + 1 = 5 applications is (sigma_{q+1} / sigma_5)^5 squared,
5e-13 for 0.7^i at q = 12.  The fixtures hold fp32 results of torch.pca_lowrank on D = 4096 columns: s to sqrt(D) 2^-24
= 3.8e-6 (they are 5e-7 - 6e-7 from the float64 SVD), rows with >= 1 % gaps to |cos| >= 0.999999.
"""
import os

import pytest
import torch

import loco_oracle as orc
from loco_edit_amd.config import TINY_DDPM, synth_params

import hspace_oracle as hso
import pca_oracle as po

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEEP = 5
# (N, D, q), ratio of the spectrum 10 * ratio^i, column offset
CASES = [((96, 320, 8), 0.5, 100.0), ((70, 200, 12), 0.7, 100.0)]
FIXTURE_S_BAR = 4096 ** 0.5 * 2.0 ** -24


def case_matrix(shape, ratio, offset):
    N, D, _ = shape
    return po.graded_matrix(N, D, min(N - 1, D), 10.0, ratio, offset, seed=N)


def omega_of(D, q, seed=5):
    return torch.randn(D, q, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("shape,ratio,offset", CASES)
def test_oracle_against_svd(shape, ratio, offset):
    N, D, q = shape
    H = case_matrix(shape, ratio, offset).double()
    s, V, mean = po.pca_lowrank_oracle(H, q, 2, omega_of(D, q))
    Hc = H - H.mean(dim=0)
    _, S, Vh = torch.linalg.svd(Hc, full_matrices=False)
    s_rel = float(((s[:KEEP] - S[:KEEP]) / S[:KEEP]).abs().max())
    one_minus_cos = float((1 - po.cos_columns(V[:, :KEEP], Vh[:KEEP].T)).abs().max())
    print(f"{shape}: s rel {s_rel:.1e}, 1 - |cos| {one_minus_cos:.1e}")
    assert s_rel <= 1e-9 and one_minus_cos <= 1e-9
    assert torch.equal(mean, H.mean(dim=0))
    assert float((V.T @ V - torch.eye(q, dtype=torch.float64)).abs().max()) < 1e-12
    idx = V.abs().argmax(dim=0)
    assert bool((V[idx, torch.arange(q)] > 0).all())           # the sign rule


def test_oracle_equals_pca_lowrank_at_full_rank():
    H = case_matrix((70, 200, 12), 0.7, 100.0)[:14].double()
    q = 13
    s, V, _ = po.pca_lowrank_oracle(H, q, 2, omega_of(200, q))
    torch.manual_seed(0)
    _, S, W = torch.pca_lowrank(H, q=q, center=True, niter=2)
    assert float(((s - S) / S).abs().max()) <= 1e-10
    assert float((1 - po.cos_columns(V[:, :3], W[:, :3])).abs().max()) <= 1e-9


def test_oracle_uncentred_and_refusals():
    H = case_matrix((70, 200, 12), 0.7, 0.0).double()
    s, V, mean = po.pca_lowrank_oracle(H, 12, 2, omega_of(200, 12), center=False)
    S = torch.linalg.svdvals(H)
    assert float(((s[:KEEP] - S[:KEEP]) / S[:KEEP]).abs().max()) <= 1e-9 and not mean.any()
    with pytest.raises(ValueError, match="exceeds"):
        po.pca_lowrank_oracle(H[:8], 8, 2, omega_of(200, 8))
    g = torch.Generator().manual_seed(1)
    low = (torch.randn(70, 3, generator=g, dtype=torch.float64) @ torch.randn(3, 200, generator=g, dtype=torch.float64)).float()
    with pytest.raises(po.RankError, match="numerical rank"):
        po.pca_lowrank_oracle(low, 8, 2, omega_of(200, 8).float())


@pytest.mark.parametrize("name,niter", [("hspace_pca_tiny_ddpm", 2), ("hspace_pca_tiny_ddpm_global", 5)])
def test_oracle_reproduces_fixture(name, niter):
    fx = torch.load(os.path.join(GOLD, name + ".pt"))
    H, q = fx["H"].double(), fx["pca_rank"]
    assert H.shape[0] == q + 1 and bool(fx["gap_rows"][:3].all())
    s, V, _ = po.pca_lowrank_oracle(H, q, niter, omega_of(H.shape[1], q))
    s_rel = float(((s - fx["s"].double()) / s).abs().max())
    cos = po.cos_columns(V, fx["u"])[fx["gap_rows"]]
    print(f"{name}: s rel {s_rel:.1e}, min |cos| over {int(fx['gap_rows'].sum())} gap rows {float(cos.min()):.9f}")
    assert s_rel <= FIXTURE_S_BAR
    assert float(cos.min()) >= 0.999999


def test_inv_jac_xt_restatement_against_fixture():
    """The reference differentiates || h + delta u - get_h(x) || at x: -J^T u / (|J^T u| + 1e-6), sign included."""
    fx = torch.load(os.path.join(GOLD, "hspace_pca_tiny_ddpm.pt"))
    cfg = TINY_DDPM
    p = {k: v.double() for k, v in orc.to_torch(synth_params(cfg, 0)).items()}
    t = torch.tensor(float(fx["t"]))
    x = fx["x"].double()
    with torch.no_grad():
        h0 = hso.get_h(p, cfg, x, t).reshape(-1)
    xr = x.clone().requires_grad_(True)
    h = hso.get_h(p, cfg, xr, t).reshape(-1)
    rows = []
    for i in range(fx["u"].shape[1]):
        target = h0 + fx["perturb_h"] * fx["u"][:, i].double()
        g = torch.autograd.grad((target - h).norm(), xr, retain_graph=True)[0].reshape(-1)
        rows.append(g / (g.norm() + 1e-6))
    vT = torch.stack(rows)
    cos = (vT * fx["vT"].double()).sum(dim=1) / (vT.norm(dim=1) * fx["vT"].double().norm(dim=1))
    print(f"signed cos: min {float(cos.min()):.9f}")
    assert float(cos.min()) >= 0.999999
