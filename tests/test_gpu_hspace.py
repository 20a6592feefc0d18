"""MI355X: the h-space tap (loco_h_dims, loco_unet_get_h, loco_unet_forward_dh, loco_pmp_primal_tap and the tap products of
loco_pmp_jvp / loco_pmp_vjp) against the float64 restatement tests/hspace_oracle.py, and the three pullback solvers against what
the reference's own functions computed (tests/golden/hspace_tiny_ddpm.pt).

Bars (those of test_gpu_parity.py / test_gpu_latent.py): forwards rel-L2 <= 2e-5 (f32) / 2e-4 (bf16x3); Jacobian products 5 x
that; |<JV, U> - <V, J^T U>| <= 1e-4 |JV| |U| per row, U independent of JV; solvers s rtol 1e-3 and row-wise |cos| >= 0.999.
"""
import os

import pytest
import torch

import loco_oracle as orc
from loco_edit_amd.config import TINY_ADM, TINY_DDPM, TINY_DECODER, synth_params

import hspace_oracle as hso

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECS = ["f32", "bf16x3"]
FWD = {"f32": 2e-5, "bf16x3": 2e-4}
JAC = {p: 5 * v for p, v in FWD.items()}
CFGS = {"tiny_ddpm": TINY_DDPM, "tiny_adm": TINY_ADM}
T = 601.0


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def new_engine(cfg, max_batch):
    from loco_edit_amd.hip import LocoEngine
    e = LocoEngine(cfg, max_batch=max_batch, device=torch.device(DEV))
    e.load_state_dict(synth_params(cfg, 0))
    return e


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(tag, max_batch, prec):
        if (tag, max_batch) not in cache:
            cache[(tag, max_batch)] = new_engine(CFGS[tag], max_batch)
        cache[(tag, max_batch)].set_precision(prec)
        return cache[(tag, max_batch)]
    return get


class Truth:
    """Float64 restatement of one configuration at a fixed (x, t): computed once, shared, never written to."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.p = {k: v.double() for k, v in orc.to_torch(synth_params(cfg, 0)).items()}
        g = torch.Generator().manual_seed(3)
        R, C = cfg.resolution, cfg.in_channels
        self.x = torch.randn(1, C, R, R, generator=g)
        self.xb = torch.cat([self.x, torch.randn(2, C, R, R, generator=g)])
        self.t = torch.tensor(T)
        sch = orc.Scheduler()
        self.at = float(sch.alpha_at(torch.tensor(int(T))))
        with torch.no_grad():
            self.hb = hso.get_h(self.p, cfg, self.xb.double(), self.t)
        self.h = self.hb[:1]
        self.n, self.n_h = self.x[0].numel(), self.h[0].numel()
        self.dh = [s * torch.randn(3, self.n_h, generator=g) for s in (0.1, 1.0, 5.0)]
        with torch.no_grad():
            self.eps_dh = [hso.forward_dh(self.p, cfg, self.xb.double(), self.t, d.double()) for d in self.dh]
            self.eps = hso.forward_dh(self.p, cfg, self.xb.double(), self.t, None)
        self.V_in = torch.randn(5, self.n, generator=g)        # probes in x_t space
        self.V_h = torch.randn(5, self.n_h, generator=g)       # probes in h space
        self.U_h = torch.randn(5, self.n_h, generator=g)       # cotangents in h space
        self.U_out = torch.randn(5, self.n, generator=g)       # cotangents in output space
        self.mask = torch.zeros(C, R, R, dtype=torch.bool)
        self.mask[:, 9:22, 5:19] = True
        self._cache = {}

    def enc(self):
        """(J V_in [5, n_h], J^T U_h [5, n]) of J = d h / d x_t."""
        if "enc" not in self._cache:
            x = self.x.double()
            f = lambda x_: hso.get_h(self.p, self.cfg, x_, self.t)
            JV = torch.stack([torch.func.jvp(f, (x,), (v.double().reshape(x.shape),))[1].reshape(-1) for v in self.V_in])
            xr = x.clone().requires_grad_(True)
            h = f(xr)
            JtU = torch.stack([torch.autograd.grad((h.reshape(-1) * u.double()).sum(), xr, retain_graph=True)[0].reshape(-1)
                               for u in self.U_h])
            self._cache["enc"] = (JV.detach(), JtU.detach())
        return self._cache["enc"]

    def dec(self, masked, use_et):
        """(J V_h [5, n], J^T U_out [5, n_h]) of J = mask . c . d eps / d h."""
        key = ("dec", masked, use_et)
        if key not in self._cache:
            c = 1.0 if use_et else -((1 - self.at) ** 0.5) / self.at ** 0.5
            m = self.mask.reshape(-1).double() if masked else torch.ones(self.n, dtype=torch.float64)
            x = self.x.double()
            f = lambda h_: (c * m * hso.h_to_e(self.p, self.cfg, x, self.t, h_).reshape(-1))
            h0 = self.h.double()
            JV = torch.stack([torch.func.jvp(f, (h0,), (v.double().reshape(h0.shape),))[1] for v in self.V_h])
            hr = h0.clone().requires_grad_(True)
            e = f(hr)
            JtU = torch.stack([torch.autograd.grad((e * u.double()).sum(), hr, retain_graph=True)[0].reshape(-1) for u in self.U_out])
            self._cache[key] = (JV.detach(), JtU.detach())
        return self._cache[key]


_TRUTH = {}


def truth(tag):
    if tag not in _TRUTH:
        _TRUTH[tag] = Truth(CFGS[tag])
    return _TRUTH[tag]


# ---------------------------------------------------------------------------------------------------------- 1. forwards
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_batch", [2, 4])
@pytest.mark.parametrize("tag", sorted(CFGS))
def test_get_h_and_forward_dh(tag, max_batch, prec, engines):
    tr, eng = truth(tag), engines(tag, max_batch, prec)
    tol = FWD[prec]
    assert eng.h_shape == tuple(tr.h.shape[1:]) and eng.n_h == tr.n_h
    B = min(3, max_batch)
    xb = tr.xb[:B].contiguous().to(DEV)
    h1 = eng.get_h(xb[:1].contiguous(), T)
    assert tuple(h1.shape) == tuple(tr.h.shape)
    print(f"get_h B=1 {rel(h1, tr.h):.2e}")
    assert rel(h1, tr.h) < tol
    hB = eng.get_h(xb, T)
    print(f"get_h B={B} {rel(hB, tr.hb[:B]):.2e}")
    assert rel(hB, tr.hb[:B]) < tol
    plain = eng.unet_forward(xb, T)
    assert rel(plain, tr.eps[:B]) < tol
    for d, want in zip(tr.dh, tr.eps_dh):
        got = eng.unet_forward(xb, T, dh=d[:B].contiguous().to(DEV))
        print(f"forward_dh |dh|={float(d.norm()):.1f} {rel(got, want[:B]):.2e} (shift moved eps by {rel(want[:B], tr.eps[:B]):.2e})")
        assert rel(got, want[:B]) < tol
        assert rel(want[:B], tr.eps[:B]) > 10 * tol            # the case can tell a shift that was not applied
    zero = eng.unet_forward(xb, T, dh=torch.zeros(B, tr.n_h, device=DEV))
    assert torch.equal(zero, eng.unet_forward(xb, T, dh=None))
    assert torch.equal(zero, plain)
    # a forward invalidates the cached primal, as loco_unet_forward does
    eng.pmp_primal(xb[:1].contiguous(), T, tr.at, None, tap="enc")
    eng.get_h(xb[:1].contiguous(), T)
    with pytest.raises(RuntimeError, match="has not been called"):
        eng.pmp_jvp(tr.V_in[:1].contiguous().to(DEV))


# ---------------------------------------------------------------------------------------------------------- 2. operators
def _adjoint(V, JV, U, JtU):
    """max over rows of |<JV_i, U_i> - <V_i, (J^T U)_i>| / (|JV_i| |U_i|) on the device results, U drawn independently of JV:
    the form and the 1e-4 bar of test_gpu_parity.test_adjointness_and_linearity_full_size."""
    JV, U, V, JtU = JV.double(), U.double(), V.double(), JtU.double()
    lhs, rhs = (JV * U).sum(dim=1), (V * JtU).sum(dim=1)
    return float(((lhs - rhs).abs() / (JV.norm(dim=1) * U.norm(dim=1))).max())


def _adjoint_of(eng, V, JV):
    """The same with U = JV (<JV, U> = |JV|^2, no cancellation): an extra on top of the independent pair."""
    return _adjoint(V, JV, JV, eng.pmp_vjp(JV.contiguous()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_batch,k", [(2, 3), (2, 5), (4, 3), (4, 5)])
@pytest.mark.parametrize("tag", sorted(CFGS))
def test_encoder_operator(tag, max_batch, k, prec, engines):
    tr, eng = truth(tag), engines(tag, max_batch, prec)
    JV_t, JtU_t = tr.enc()
    x = tr.x.to(DEV)
    eng.pmp_primal(x, T, tr.at, None, tap="enc")
    V, U = tr.V_in[:k].contiguous().to(DEV), tr.U_h[:k].contiguous().to(DEV)
    JV, JtU = eng.pmp_jvp(V), eng.pmp_vjp(U)
    assert tuple(JV.shape) == (k, tr.n_h) and tuple(JtU.shape) == (k, tr.n)
    assert eng.mask_count() == tr.n_h and torch.equal(eng.mask_gather(JV), JV)      # rows of J V as they are: n_h wide
    adj, adj_jv = _adjoint(V, JV, U, JtU), _adjoint_of(eng, V, JV)
    print(f"enc jvp {rel(JV, JV_t[:k]):.2e} vjp {rel(JtU, JtU_t[:k]):.2e} adjoint {adj:.2e} (U = JV: {adj_jv:.2e})")
    assert rel(JV, JV_t[:k]) < JAC[prec] and rel(JtU, JtU_t[:k]) < JAC[prec]
    assert adj < 1e-4 and adj_jv < 1e-4


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("use_et", [True, False])
@pytest.mark.parametrize("max_batch,k", [(2, 3), (2, 5), (4, 3), (4, 5)])
@pytest.mark.parametrize("tag", sorted(CFGS))
def test_decoder_operator(tag, max_batch, k, use_et, masked, prec, engines):
    tr, eng = truth(tag), engines(tag, max_batch, prec)
    JV_t, JtU_t = tr.dec(masked, use_et)
    eng.pmp_primal(tr.x.to(DEV), T, tr.at, tr.mask.to(DEV) if masked else None, use_et=use_et, tap="dec")
    V, U = tr.V_h[:k].contiguous().to(DEV), tr.U_out[:k].contiguous().to(DEV)
    JV, JtU = eng.pmp_jvp(V), eng.pmp_vjp(U)
    assert tuple(JV.shape) == (k, tr.n) and tuple(JtU.shape) == (k, tr.n_h)
    adj, adj_jv = _adjoint(V, JV, U, JtU), _adjoint_of(eng, V, JV)
    print(f"dec jvp {rel(JV, JV_t[:k]):.2e} vjp {rel(JtU, JtU_t[:k]):.2e} adjoint {adj:.2e} (U = JV: {adj_jv:.2e})")
    assert rel(JV, JV_t[:k]) < JAC[prec] and rel(JtU, JtU_t[:k]) < JAC[prec]
    if masked:
        assert float(JV[:, ~tr.mask.reshape(-1).to(DEV)].abs().max()) == 0.0
    assert adj < 1e-4 and adj_jv < 1e-4


@pytest.mark.parametrize("prec", PRECS)
def test_two_stream_lanes_and_forked_context(prec, engines):
    """The probe batch cut in two lanes on two streams (B >= 4), and a forked context: the same products."""
    tr, eng = truth("tiny_ddpm"), engines("tiny_ddpm", 4, prec)
    x = tr.x.to(DEV)
    V, U = tr.V_in[:5].contiguous().to(DEV), tr.U_h[:5].contiguous().to(DEV)
    Vh, Uo = tr.V_h[:5].contiguous().to(DEV), tr.U_out[:5].contiguous().to(DEV)

    def products(e):
        e.pmp_primal(x, T, tr.at, None, tap="enc")
        a = (e.pmp_jvp(V), e.pmp_vjp(U))
        e.pmp_primal(x, T, tr.at, tr.mask.to(DEV), use_et=False, tap="dec")
        return a + (e.pmp_jvp(Vh), e.pmp_vjp(Uo))
    one = products(eng)
    eng.set_streams(2)
    try:
        two = products(eng)
    finally:
        eng.set_streams(1)
    want = tr.enc() + tr.dec(True, False)
    for a, b, w in zip(one, two, want):
        assert rel(b, w) < JAC[prec] and rel(b, a) < JAC[prec]
    child = eng.fork()
    child.set_precision(prec)
    assert child.h_shape == eng.h_shape
    for a, b in zip(one, products(child)):
        assert torch.equal(a, b)
    assert torch.equal(child.get_h(x, T), eng.get_h(x, T))


@pytest.mark.parametrize("prec", PRECS)
def test_conditioned_context_with_residual_scale(prec):
    """A conditioned context (set_context + set_cond) of the DeepFloyd-IF family: the same ops, so the tap comes with them; its
    ResBlocks scale their output by 1 / sqrt(2), which forward_dh has to undo for the shift it feeds through the residual."""
    from loco_edit_amd.config import TINY_IF
    from loco_edit_amd.hip import LocoEngine
    from loco_edit_amd.tloco import IFTextConditioner
    cfg = TINY_IF
    params = synth_params(cfg, 2)
    p = {k: v.double() for k, v in orc.to_torch(params).items()}
    g = torch.Generator().manual_seed(11)
    states = torch.randn(1, cfg.context_len, cfg.encoder_dim, generator=g)
    eng = LocoEngine(cfg, max_batch=2, device=torch.device(DEV))
    eng.load_state_dict(params)
    context, aug = IFTextConditioner(params, cfg, DEV)(states)
    eng.set_context(context)
    eng.set_cond(aug)
    eng.set_precision(prec)
    ctx, add = orc.if_text_conditioning(p, cfg, states.double())
    cond = dict(context=ctx, emb_add=add)
    x = torch.randn(2, 3, cfg.resolution, cfg.resolution, generator=g)
    t, tt = 417.0, torch.tensor(417.0)
    dh = 2.0 * torch.randn(2, eng.n_h, generator=g)
    with torch.no_grad():
        h = hso.get_h(p, cfg, x.double(), tt, **cond)
        e = hso.forward_dh(p, cfg, x.double(), tt, dh.double(), **cond)
        e0 = hso.forward_dh(p, cfg, x.double(), tt, None, **cond)
    xd = x.to(DEV)
    print(f"IF get_h {rel(eng.get_h(xd, t), h):.2e} forward_dh {rel(eng.unet_forward(xd, t, dh=dh.to(DEV)), e):.2e} "
          f"(shift moved eps by {rel(e, e0):.2e})")
    assert rel(eng.get_h(xd, t), h) < FWD[prec]
    assert rel(eng.unet_forward(xd, t, dh=dh.to(DEV)), e) < FWD[prec] and rel(e, e0) > 10 * FWD[prec]
    assert torch.equal(eng.unet_forward(xd, t, dh=torch.zeros_like(dh).to(DEV)), eng.unet_forward(xd, t))
    # the decoder operator at x[0], k = 3 through max_batch = 2
    x1, h1 = x[:1].double(), h[:1]
    V = torch.randn(3, eng.n_h, generator=g)
    f = lambda h_: hso.h_to_e(p, cfg, x1, tt, h_, **cond).reshape(-1)
    JV_t = torch.stack([torch.func.jvp(f, (h1,), (v.double().reshape(h1.shape),))[1] for v in V])
    eng.pmp_primal(xd[:1].contiguous(), t, 0.5, None, use_et=True, tap="dec")
    JV = eng.pmp_jvp(V.to(DEV))
    Uo = torch.randn(3, eng.n_out, generator=g).to(DEV)
    adj = max(_adjoint(V.to(DEV), JV, Uo, eng.pmp_vjp(Uo)), _adjoint_of(eng, V.to(DEV), JV))
    print(f"IF dec jvp {rel(JV, JV_t):.2e} adjoint {adj:.2e}")
    assert rel(JV, JV_t) < JAC[prec] and adj < 1e-4
    Vx = torch.randn(3, eng.n, generator=g)
    fe = lambda x_: hso.get_h(p, cfg, x_, tt, **cond).reshape(-1)
    JVe_t = torch.stack([torch.func.jvp(fe, (x1,), (v.double().reshape(x1.shape),))[1] for v in Vx])
    eng.pmp_primal(xd[:1].contiguous(), t, 0.5, None, tap="enc")
    JVe = eng.pmp_jvp(Vx.to(DEV))
    Uh = torch.randn(3, eng.n_h, generator=g).to(DEV)
    adj = max(_adjoint(Vx.to(DEV), JVe, Uh, eng.pmp_vjp(Uh)), _adjoint_of(eng, Vx.to(DEV), JVe))
    print(f"IF enc jvp {rel(JVe, JVe_t):.2e} adjoint {adj:.2e}")
    assert rel(JVe, JVe_t) < JAC[prec] and adj < 1e-4


# ---------------------------------------------------------------------------------------------------------- 3. state hygiene
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", sorted(CFGS))
def test_tap_products_do_not_see_an_earlier_full_pass_and_leave_none_behind(tag, prec):
    """The passes over half of the program read skip tangents, skip cotangent slots and kept concatenation partials that only
    a full pass writes: after full x0 products at another x' the tap products must be what a fresh context computes, and full
    x0 products after tap products likewise."""
    tr = truth(tag)
    x, x2 = tr.x.to(DEV), tr.xb[1:2].contiguous().to(DEV)
    k = 4
    V, Uh = tr.V_in[:k].contiguous().to(DEV), tr.U_h[:k].contiguous().to(DEV)
    Vh, Uo = tr.V_h[:k].contiguous().to(DEV), tr.U_out[:k].contiguous().to(DEV)
    mask = tr.mask.to(DEV)

    def full(e, at_x):
        e.pmp_primal(at_x, T, tr.at, mask)
        return e.pmp_jvp(V), e.pmp_vjp(Uo)

    def taps(e):
        e.pmp_primal(x, T, tr.at, None, tap="enc")
        a = (e.pmp_jvp(V), e.pmp_vjp(Uh))
        e.pmp_primal(x, T, tr.at, mask, use_et=True, tap="dec")
        return a + (e.pmp_jvp(Vh), e.pmp_vjp(Uo))

    def engine():
        e = new_engine(CFGS[tag], 4)
        e.set_precision(prec)
        return e
    fresh_taps = taps(engine())
    fresh_full = full(engine(), x)
    e = engine()
    full(e, x2)                                 # leaves tangents / cotangents / partials of x' everywhere
    for a, b in zip(taps(e), fresh_taps):
        assert torch.equal(a, b)
    e = engine()
    taps(e)
    e.pmp_primal(x2, T, tr.at, None, tap="dec")
    e.pmp_jvp(Vh)
    for a, b in zip(full(e, x), fresh_full):
        assert torch.equal(a, b)
    # tap = None after a tap primal is the x0 operator again, with its widths
    assert tuple(full(e, x)[0].shape) == (k, tr.n)


# ---------------------------------------------------------------------------------------------------------- 4. solvers
class _Sched:
    def __init__(self, at):
        self.at = at

    def alpha_at(self, t):
        return self.at


def _edit(eng, at):
    """An EditUncondDiffusion around an existing engine (its constructor builds the model from CLI arguments)."""
    from loco_edit_amd.dist import ProbeSharder
    from loco_edit_amd.edit import EditUncondDiffusion
    ed = object.__new__(EditUncondDiffusion)
    ed.engine, ed.device, ed.scheduler, ed.sharder = eng, torch.device(DEV), _Sched(at), ProbeSharder(None)
    return ed


def _abs_cos_rows(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).abs()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_batch", [2, 4])
@pytest.mark.parametrize("which", ["enc", "dec", "x0dec"])
def test_pullback_solvers_vs_reference_golden(which, max_batch, prec, engines, golden):
    g = golden("hspace_tiny_ddpm")
    r = g[which]
    eng = engines("tiny_ddpm", max_batch, prec)
    ed = _edit(eng, g["at"])
    kw = dict(x=g["x"].to(DEV), t=float(g["t"]), op='mid', block_idx=0, pca_rank=g["k"], chunk_size=g["k"], min_iter=10,
              max_iter=g["n_iter"], convergence_threshold=0, v0=r["v0"].to(DEV), verbose=False)
    if which == "enc":
        u, s, vT = ed.local_encoder_pullback_xt(**kw)
    elif which == "dec":
        u, s, vT = ed.local_decoder_pullback_xt(**kw)
    else:
        u, s, vT = ed.local_x0_decoder_pullback_xt(at=torch.tensor(g["at"]), **kw)
    assert ed.last_n_iter == g["n_iter"]
    assert tuple(u.shape) == tuple(r["u"].shape) and tuple(vT.shape) == tuple(r["vT"].shape)
    print(f"{which}: s {s.tolist()} ref {r['s'].tolist()} cos vT {_abs_cos_rows(vT, r['vT']).tolist()} "
          f"cos u {_abs_cos_rows(u.T, r['u'].T).tolist()}")
    assert torch.allclose(s.cpu(), r["s"], rtol=1e-3)
    assert (_abs_cos_rows(vT, r["vT"]) >= 0.999).all()
    assert (_abs_cos_rows(u.T, r["u"].T) >= 0.999).all()


def test_solver_targets_and_krylov_refusal(engines):
    from loco_edit_amd import solver
    tr, eng = truth("tiny_ddpm"), engines("tiny_ddpm", 4, "f32")
    x = tr.x.to(DEV)
    with pytest.raises(ValueError, match="Krylov"):
        solver.local_basis(eng, x, T, tr.at, 2, target="h_enc", solver="krylov", verbose=False)
    with pytest.raises(ValueError, match="target"):
        solver.local_basis(eng, x, T, tr.at, 2, target="h", verbose=False)
    with pytest.raises(ValueError, match="no mask"):
        solver.local_basis(eng, x, T, tr.at, 2, target="h_enc", mask=tr.mask, verbose=False)
    # subspace_iteration runs unchanged on the tap operators: rows of the operators' widths
    u, s, vT, n_iter = solver.local_basis(eng, x, T, tr.at, 2, target="h_dec", mask=tr.mask, noise=True, max_iter=2, verbose=False)
    assert tuple(u.shape) == (int(tr.mask.sum()), 2) and tuple(vT.shape) == (2, tr.n_h) and n_iter == 2
    u, s, vT, n_iter = solver.local_basis(eng, x, T, tr.at, 2, target="h_enc", max_iter=2, verbose=False)
    assert tuple(u.shape) == (tr.n_h, 2) and tuple(vT.shape) == (2, tr.n)


# ---------------------------------------------------------------------------------------------------------- 5. driver
@pytest.mark.parametrize("null_proj", ["True", "False"])
def test_cli_jacobian_target_h(null_proj, tmp_path, monkeypatch):
    from loco_edit_amd.main import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("LOCO_SOLVER", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    rdir = tmp_path / "runs" / "CelebA_HQ_HF-Random" / "results" / "sample_seed11"
    os.makedirs(rdir / "mask")
    masks = torch.zeros(2, 32, 32, dtype=torch.bool)
    masks[0, 8:20, 6:18] = True
    masks[1, 20:28, 20:30] = True
    torch.save(masks, rdir / "mask" / "mask.pt")
    base = ["--sh_file_name", "main_celeba_hf_null_space_projection.sh", "--sample_idx", "3", "--device", DEV,
            "--dtype", "fp32", "--seed", "11", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random",
            "--unet_preset", "tiny_ddpm", "--synthetic_weights", "0", "--for_steps", "100", "--inv_steps", "100",
            "--use_yh_custom_scheduler", "True", "--x_space_guidance_edit_step", "1", "--x_space_guidance_scale", "0.5",
            "--x_space_guidance_num_step", "16", "--edit_t", "0.6", "--performance_boosting_t", "0.2", "--mask_index", "0",
            "--null_space_projection", null_proj, "--use_mask", "True", "--pca_rank_null", "2", "--pca_rank", "2", "--vis_num", "2",
            "--run_edit_null_space_projection", "True"]
    xt = main(base + ["--jacobian_target", "h"])
    assert xt.shape == (5, 3, 32, 32)
    bdir = rdir / "basis" / "local_basis-0.6T-select-mask-0"
    assert (bdir / "vT-modify-pca-rank-2-hspace.pt").exists() and not (bdir / "vT-modify-pca-rank-2.pt").exists()
    assert (bdir / "vT-null-2.pt").exists() == (null_proj == "True")
    vT_modify = torch.load(bdir / "vT-modify-pca-rank-2-hspace.pt")
    assert tuple(vT_modify.shape) == (2, 3 * 32 * 32)
    pcs = sorted(f for f in os.listdir(bdir) if f.endswith("-vT.pt"))
    assert len(pcs) == 2 and all("-hspace-pc_" in f for f in pcs)
    grids = sorted(f for f in os.listdir(rdir) if f.startswith("3-Edit-randomFalse_xt-noise-") and f.endswith(".png"))
    assert len(grids) == 2 and all("-hspace-pc_" in f for f in grids)
    # the saved direction through --vT_path walks the same frames
    xt2 = main(base + ["--jacobian_target", "h", "--vT_path", str(bdir / pcs[1])])
    assert torch.equal(xt2, xt)
    # a default-target run in the same folder: today's names, and the tagged basis is not taken for it
    before = set(os.listdir(bdir))
    main(base)
    new = set(os.listdir(bdir)) - before
    assert "vT-modify-pca-rank-2.pt" in new and not any("hspace" in f for f in new)
    assert len([f for f in new if f.endswith("-vT.pt")]) == 2
    assert not torch.equal(torch.load(bdir / "vT-modify-pca-rank-2.pt"), vT_modify)


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(engines):
    tr, eng = truth("tiny_ddpm"), engines("tiny_ddpm", 4, "f32")
    x = tr.x.to(DEV)
    with pytest.raises(RuntimeError, match="takes no mask"):
        eng.pmp_primal(x, T, tr.at, tr.mask.to(DEV), tap="enc")
    with pytest.raises(ValueError, match="tap must be"):
        eng.pmp_primal(x, T, tr.at, None, tap="mid")
    eng.pmp_primal(x, T, tr.at, None, tap="enc")
    with pytest.raises(ValueError, match=f"{tr.n}"):
        eng.pmp_jvp(tr.V_h[:2].contiguous().to(DEV))             # h-space rows into the x_t -> h operator
    with pytest.raises(ValueError, match=f"{tr.n_h}"):
        eng.pmp_vjp(tr.U_out[:2].contiguous().to(DEV))
    eng.pmp_primal(x, T, tr.at, None, use_et=True, tap="dec")
    with pytest.raises(ValueError, match=f"{tr.n_h}"):
        eng.pmp_jvp(tr.V_in[:2].contiguous().to(DEV))
    with pytest.raises(ValueError, match="dh must hold"):
        eng.unet_forward(x, T, dh=torch.zeros(1, tr.n, device=DEV))
    dec = new_engine(TINY_DECODER, 2)
    z = torch.randn(1, 4, 16, 16, device=DEV)
    for call in (lambda: dec.h_shape, lambda: dec.get_h(z, 0.0), lambda: dec.unet_forward(z, 0.0, dh=torch.zeros(1, 4, device=DEV)),
                 lambda: dec.pmp_primal(z, 0.0, 1.0, None, use_et=True, tap="dec")):
        with pytest.raises(RuntimeError, match="no h-space tap"):
            call()
