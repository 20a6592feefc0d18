"""MI355X: the device PCA unit alone (csrc/pca.hip through hip.LocoPca) against float64 and against its restatement
tests/pca_oracle.py with the same omega.

Shapes: (N, D, q) = (70, 200, 12) and (96, 320, 8) with a column offset of 100 (no multiple of a tile), and one long
contraction (1030, 136, 8) whose row split has several parts and a tail.  Bars:
  - centred store and mean: within 1 ulp of fp32 of the float64 value of the same fp32 input;
  - Gram: |dG_ij| <= 1e-12 sqrt(G_ii G_jj) (products of two fp32 values are exact in double; L 2^-53 of summation remains);
  - Hc Omega (and Hc^T Q): relative error <= 1e-5 at offset 100 (the rank-one correction form misses this by a factor 30 - 80);
  - fit: the error of the fp32 CPU run of the oracle against its float64 run is measured here on every case of the file, for s
    (relative) and for 1 - |cos| of the KEEP columns; the largest is the yardstick and the HIP result stays within 4 x it (the
    margin this project gives its exact-fp32 units for another summation order);
  - bit identity between calls and between appends in chunks of 5 / 7 / all; refusals by their messages.
"""
import os

import pytest
import torch

import pca_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEEP = 5
NITER = 2
CASES = {"70x200q12": ((70, 200, 12), 0.7), "96x320q8": ((96, 320, 8), 0.5), "1030x136q8": ((1030, 136, 8), 0.5)}
FIXTURES = {"hspace_pca_tiny_ddpm": 2, "hspace_pca_tiny_ddpm_global": 5}


def LocoPca(*a, **k):
    from loco_edit_amd.hip import LocoPca as cls
    return cls(*a, **k)


class Case:
    """One sample matrix with its omega and both oracle runs: computed once, shared, never written to."""

    def __init__(self, H, q, niter, gap_rows=None, want=None):
        self.H, self.q, self.niter = H, q, niter
        N, D = H.shape
        self.omega = torch.randn(D, q, generator=torch.Generator().manual_seed(5))
        self.s64, self.V64, self.mean64 = po.pca_lowrank_oracle(H.double(), q, niter, self.omega)
        self.s32, self.V32, _ = po.pca_lowrank_oracle(H, q, niter, self.omega)
        self.keep = torch.arange(q)[:KEEP] if gap_rows is None else torch.arange(q)[gap_rows][:KEEP]
        self.want = want
        self.s_err32 = float(((self.s32.double() - self.s64) / self.s64).abs().max())
        self.cos_err32 = float((1 - po.cos_columns(self.V32[:, self.keep], self.V64[:, self.keep])).abs().max())


_CASES = {}


def cases():
    if not _CASES:
        for tag, ((N, D, q), ratio) in CASES.items():
            _CASES[tag] = Case(po.graded_matrix(N, D, min(N - 1, D), 10.0, ratio, 100.0, seed=N), q, NITER)
        for name, niter in FIXTURES.items():
            fx = torch.load(os.path.join(GOLD, name + ".pt"))
            _CASES[name] = Case(fx["H"], fx["pca_rank"], niter, gap_rows=fx["gap_rows"], want=fx)
    return _CASES


def yardstick():
    """(s, 1 - |cos|): the largest fp32-oracle error over the file's cases."""
    cs = cases().values()
    return max(c.s_err32 for c in cs), max(c.cos_err32 for c in cs)


def store_of(H, q_max, chunk=None, n_max=None):
    st = LocoPca(n_max or H.shape[0], H.shape[1], q_max, device=torch.device(DEV))
    Hd = H.to(DEV)
    chunk = chunk or H.shape[0]
    for r0 in range(0, H.shape[0], chunk):
        st.add_rows(Hd[r0:r0 + chunk].contiguous())
    return st


def ulp32(ref64):
    """Spacing of fp32 at |ref| (double)."""
    _, e = torch.frexp(ref64.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref64), e - 24)


# ------------------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("tag", sorted(CASES))
def test_centred_store(tag):
    c = cases()[tag]
    st = store_of(c.H, c.q, chunk=7)
    assert st.rows == c.H.shape[0]
    Hc, mean = st.centered()
    H64 = c.H.double()
    mu = H64.mean(dim=0)
    ref = H64 - mu
    d = (Hc.cpu().double() - ref).abs()
    print(f"{tag}: centred store worst {float((d / ulp32(ref)).max()):.2f} ulp, mean worst {float(((mean.cpu().double() - mu).abs() / ulp32(mu)).max()):.2f} ulp")
    assert bool((d <= ulp32(ref)).all())
    assert bool(((mean.cpu().double() - mu).abs() <= ulp32(mu)).all())
    raw, zero = st.centered(center=False)
    assert torch.equal(raw.cpu(), c.H) and not zero.any()


@pytest.mark.parametrize("L,q", [(70, 12), (200, 12), (96, 8), (320, 8), (1030, 8), (136, 8), (1030, 33)])
def test_gram(L, q):
    st = LocoPca(1030, 320, 64, device=torch.device(DEV))
    Y = torch.randn(L, q, generator=torch.Generator().manual_seed(L + q)) * 3 + 1
    G = st.gram(Y.to(DEV)).cpu()
    ref = Y.double().T @ Y.double()
    scale = ref.diagonal().sqrt()
    err = float(((G - ref).abs() / (scale[:, None] * scale[None, :])).max())
    print(f"gram L={L} q={q}: {err:.1e}")
    assert err <= 1e-12
    assert torch.equal(G, G.T)


@pytest.mark.parametrize("route", ["split", "gemm"])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_products(tag, route):
    c = cases()[tag]
    st = store_of(c.H, c.q)
    st.set_route(route)
    Hc64 = c.H.double() - c.H.double().mean(dim=0)
    got = st.project(c.omega.to(DEV)).cpu().double()
    ref = Hc64 @ c.omega.double()
    e1 = float((got - ref).norm() / ref.norm())
    rank_one = (c.H @ c.omega - torch.ones(c.H.shape[0], 1) @ (c.H.mean(dim=0, keepdim=True) @ c.omega)).double()
    Q = torch.randn(c.H.shape[0], c.q, generator=torch.Generator().manual_seed(9))
    got_t = st.project(Q.to(DEV), transpose=True).cpu().double()
    ref_t = Hc64.T @ Q.double()
    e2 = float((got_t - ref_t).norm() / ref_t.norm())
    print(f"{tag} {route} [{st.routes()}]: Hc Omega {e1:.1e} (rank-one form on the CPU: {float((rank_one - ref).norm() / ref.norm()):.1e}), Hc^T Q {e2:.1e}")
    assert e1 <= 1e-5 and e2 <= 1e-5
    if route == "split":
        st.set_route("auto")                      # these grids do not fill the chip: the default is the split kernel
        assert torch.equal(st.project(c.omega.to(DEV)).cpu().double(), got)


# ------------------------------------------------------------------------------------------------------------------ fit
@pytest.mark.parametrize("route", ["split", "gemm"])
@pytest.mark.parametrize("tag", sorted(CASES) + sorted(FIXTURES))
def test_fit_against_oracle(tag, route):
    c = cases()[tag]
    s_bar, cos_bar = (4 * v for v in yardstick())
    st = store_of(c.H, c.q, chunk=5)
    st.set_route(route)
    s, V, mean = st.fit(c.q, c.niter, c.omega.to(DEV))
    s, V, mean = s.cpu(), V.cpu(), mean.cpu()
    assert tuple(s.shape) == (c.q,) and tuple(V.shape) == (c.H.shape[1], c.q) and tuple(mean.shape) == (c.H.shape[1],)
    s_err = float(((s.double() - c.s64) / c.s64).abs().max())
    cos_err = float((1 - po.cos_columns(V[:, c.keep], c.V64[:, c.keep])).abs().max())
    print(f"{tag} {route}: s rel {s_err:.1e} (fp32 oracle {c.s_err32:.1e}, bar {s_bar:.1e}), 1 - |cos| {cos_err:.1e} "
          f"(fp32 oracle {c.cos_err32:.1e}, bar {cos_bar:.1e})")
    assert s_err <= s_bar and cos_err <= cos_bar
    assert bool((s[:-1] >= s[1:]).all())
    # the sign rule, and signs equal to the oracle's on the kept columns
    idx = V.abs().argmax(dim=0)
    assert bool((V[idx, torch.arange(c.q)] > 0).all())
    assert bool(((V[:, c.keep].double() * c.V64[:, c.keep]).sum(dim=0) > 0).all())
    assert bool(((mean.double() - c.mean64).abs() <= ulp32(c.mean64)).all())
    if c.want is not None:                         # what the reference's own function returned for this H
        fx = c.want
        fs = float(((s.double() - fx["s"].double()) / fx["s"].double()).abs().max())
        cos = po.cos_columns(V, fx["u"])[fx["gap_rows"]]
        print(f"  fixture: s rel {fs:.1e}, min |cos| over the gap rows {float(cos.min()):.9f}")
        assert fs <= s_bar and float(cos.min()) >= 0.999999


def test_fit_uncentred():
    c = cases()["70x200q12"]
    H = c.H - 100.0
    s64, V64, _ = po.pca_lowrank_oracle(H.double(), c.q, NITER, c.omega, center=False)
    st = store_of(H, c.q)
    s, V, mean = st.fit(c.q, NITER, c.omega.to(DEV), center=False)
    s_bar, cos_bar = (4 * v for v in yardstick())
    assert float(((s.cpu().double() - s64) / s64).abs().max()) <= s_bar
    assert float((1 - po.cos_columns(V.cpu()[:, :KEEP], V64[:, :KEEP])).abs().max()) <= cos_bar
    assert not mean.any()


@pytest.mark.parametrize("tag", ["70x200q12", "1030x136q8"])
def test_bit_identity(tag):
    c = cases()[tag]
    om = c.omega.to(DEV)
    st = store_of(c.H, c.q)
    first = [o.clone() for o in st.fit(c.q, NITER, om)]
    again = st.fit(c.q, NITER, om)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for chunk in (5, 7):
        other = store_of(c.H, c.q, chunk=chunk, n_max=c.H.shape[0] + 3)       # another capacity too
        assert all(torch.equal(a, b) for a, b in zip(first, other.fit(c.q, NITER, om)))
    st.reset()
    assert st.rows == 0
    st.add_rows(c.H.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(first, st.fit(c.q, NITER, om)))


def test_rank_deficiency_is_an_error():
    g = torch.Generator().manual_seed(1)
    low = (torch.randn(70, 3, generator=g, dtype=torch.float64) @ torch.randn(3, 200, generator=g, dtype=torch.float64)).float()
    st = store_of(low, 8)
    om = torch.randn(200, 8, generator=g).to(DEV)
    with pytest.raises(RuntimeError, match=r"numerical rank \d+ is below q = 8"):
        st.fit(8, NITER, om)
    s, V, mean = st.fit(2, NITER, om[:, :2].contiguous())          # the handle is usable afterwards, nothing holds a NaN
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(V).all()) and bool(torch.isfinite(mean).all())
    s64 = po.pca_lowrank_oracle(low.double(), 2, NITER, om[:, :2].cpu())[0]
    assert float(((s.cpu().double() - s64) / s64).abs().max()) <= 4 * yardstick()[0]


def test_refusals():
    from loco_edit_amd.hip import LocoPca as cls
    dev = torch.device(DEV)
    H = torch.randn(10, 24, generator=torch.Generator().manual_seed(0)).to(DEV)
    st = cls(12, 24, 12, device=dev)
    st.add_rows(H)
    om = lambda q: torch.randn(24, q, generator=torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(RuntimeError, match=r"q = 10 exceeds min\(N - 1, D\) = 9"):
        st.fit(10, 1, om(10))
    st.fit(10, 1, om(10), center=False)
    with pytest.raises(RuntimeError, match=r"q = 11 exceeds min\(N, D\) = 10"):
        st.fit(11, 1, om(11), center=False)
    with pytest.raises(RuntimeError, match=r"10 \+ 3 rows need 1248 bytes.*12 rows \(1152 bytes\)"):
        st.add_rows(torch.zeros(3, 24, device=DEV))
    with pytest.raises(RuntimeError, match=r"width 25 \(100 bytes each\).*width 24 \(96 bytes each\)"):
        st.add_rows(torch.zeros(1, 25, device=DEV))
    assert st.rows == 10
    with pytest.raises(ValueError, match="expected torch.float32, got torch.float64"):
        st.add_rows(torch.zeros(1, 24, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="expected a tensor on cuda:0, got one on cpu"):
        st.add_rows(torch.zeros(1, 24))
    with pytest.raises(ValueError, match=r"omega: expected shape \(24, 4\), got \(24, 5\)"):
        st.fit(4, 1, om(5))
    with pytest.raises(ValueError, match="omega: expected torch.float32"):
        st.fit(4, 1, om(4).double())
    with pytest.raises(ValueError, match="omega: expected a tensor on cuda:0"):
        st.fit(4, 1, om(4).cpu())
    with pytest.raises(RuntimeError, match=r"q = 13 is outside \[1, 12\]"):
        cls(20, 24, 12, device=dev).fit(13, 1, om(13))
    with pytest.raises(ValueError, match="above the unit's limit of 512"):
        cls(600, 600, 513, device=dev)
    wide = cls(4, 520, 512, device=dev)
    with pytest.raises(RuntimeError, match=r"q = 513 is outside \[1, 512\]"):
        wide.fit(513, 1, torch.zeros(520, 513, device=DEV))
    with pytest.raises(RuntimeError, match="the store is empty"):
        wide.centered()
    with pytest.raises(ValueError, match="route must be one of"):
        st.set_route("bf16x3")


def test_pca_lowrank_device_wrapper():
    from loco_edit_amd import hspace_pca
    c = cases()["96x320q8"]
    g = torch.Generator().manual_seed(11)
    s, V, mean = hspace_pca.pca_lowrank_device(c.H.to(DEV), c.q, NITER, g)
    omega = torch.randn(320, c.q, generator=torch.Generator().manual_seed(11))
    st = store_of(c.H, c.q)
    want = st.fit(c.q, NITER, omega.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip((s, V, mean), want))
    g2 = torch.Generator().manual_seed(11)
    assert all(torch.equal(a, b) for a, b in zip(hspace_pca.pca_lowrank_device(st, c.q, NITER, g2), want))
    with pytest.raises(ValueError, match="device tensor"):
        hspace_pca.pca_lowrank_device(c.H, c.q, NITER, g)
    with pytest.raises(ValueError, match="expected torch.float32"):
        hspace_pca.pca_lowrank_device(c.H.double().to(DEV), c.q, NITER, g)
