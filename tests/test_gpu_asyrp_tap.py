"""MI355X: the decoder-tap primal at a shifted bottleneck (loco_pmp_primal_tap_dh, LocoEngine.pmp_primal(tap="dec", dh=...))
against the float64 restatement tests/hspace_oracle.py differentiated AT h + dh, on TINY_DDPM and TINY_ADM with seeded weights.

dh is a seeded normal tensor of h's own spread (std(h) = 1.9 / 1.6 on the two networks).  With the float64 oracle on the CPU
that shift moves J V and J^T U by 38 % / 85 % (a quarter of it: 11 % / 25 %), three orders above the bars, so a linearisation
taken at the unshifted point cannot pass; the test asserts that margin on its own oracle values (> 10 x the bar).

Bars, those of test_gpu_hspace.py for the unshifted products: Jacobian products rel-L2 <= 1e-4 (f32) / 1e-3 (bf16x3);
|<JV, U> - <V, J^T U>| <= 1e-4 |JV| |U| per row with U independent of JV.  pmp_primal_eps at the shifted point equals
unet_forward(x, t, dh=dh) to the last bit (the same launch list), and dh = NULL is bit-identical to loco_pmp_primal_tap(tap = 2).
"""
import ctypes as C

import pytest
import torch

import loco_oracle as orc
from loco_edit_amd.config import TINY_ADM, TINY_DDPM, TINY_DECODER, synth_params

import hspace_oracle as hso

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECS = ["f32", "bf16x3"]
JAC = {"f32": 1e-4, "bf16x3": 1e-3}
CFGS = {"tiny_ddpm": TINY_DDPM, "tiny_adm": TINY_ADM}
T = 601.0
K = 5


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(tag, max_batch, prec):
        from loco_edit_amd.hip import LocoEngine
        if (tag, max_batch) not in cache:
            e = LocoEngine(CFGS[tag], max_batch=max_batch, device=torch.device(DEV))
            e.load_state_dict(synth_params(CFGS[tag], 0))
            cache[(tag, max_batch)] = e
        cache[(tag, max_batch)].set_precision(prec)
        return cache[(tag, max_batch)]
    return get


class Truth:
    """Float64 restatement of one configuration at a fixed (x, t, dh): computed once, shared, never written to."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.p = {k: v.double() for k, v in orc.to_torch(synth_params(cfg, 0)).items()}
        g = torch.Generator().manual_seed(3)
        R, Cin = cfg.resolution, cfg.in_channels
        self.x = torch.randn(1, Cin, R, R, generator=g)
        self.t = torch.tensor(T)
        self.at = float(orc.Scheduler().alpha_at(torch.tensor(int(T))))
        with torch.no_grad():
            self.h = hso.get_h(self.p, cfg, self.x.double(), self.t)
        self.n, self.n_h = self.x.numel(), self.h.numel()
        self.dh = (float(self.h.std()) * torch.randn(self.h.shape, generator=g)).float()
        self.V_h = torch.randn(K, self.n_h, generator=g)
        self.U_out = torch.randn(K, self.n, generator=g)
        self.mask = torch.zeros(Cin, R, R, dtype=torch.bool)
        self.mask[:, 9:22, 5:19] = True
        self._cache = {}

    def dec(self, shifted, masked, use_et):
        """(J V_h [K, n], J^T U_out [K, n_h]) of J = mask . c . d eps / d h at h + dh (shifted) or at h."""
        key = (shifted, masked, use_et)
        if key not in self._cache:
            c = 1.0 if use_et else -((1 - self.at) ** 0.5) / self.at ** 0.5
            m = self.mask.reshape(-1).double() if masked else torch.ones(self.n, dtype=torch.float64)
            x = self.x.double()
            f = lambda h_: (c * m * hso.h_to_e(self.p, self.cfg, x, self.t, h_).reshape(-1))
            h0 = self.h + self.dh.double() if shifted else self.h
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


def _adjoint(V, JV, U, JtU):
    JV, U, V, JtU = JV.double(), U.double(), V.double(), JtU.double()
    lhs, rhs = (JV * U).sum(dim=1), (V * JtU).sum(dim=1)
    return float(((lhs - rhs).abs() / (JV.norm(dim=1) * U.norm(dim=1))).max())


def _primal_tap_dh_raw(eng, x, at, m8, use_et, dh):
    """loco_pmp_primal_tap_dh itself (the Python method takes the existing entry point when dh is None)."""
    from loco_edit_amd.hip import _ptr, _stream
    eng._check(eng.lib.loco_pmp_primal_tap_dh(eng._ctx, _ptr(x), C.c_float(T), C.c_float(at), _ptr(m8), int(use_et), _ptr(dh), _stream()),
               "loco_pmp_primal_tap_dh")
    eng._tap = "dec"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("tag", sorted(CFGS))
def test_null_shift_is_the_existing_primal(tag, masked, prec, engines):
    tr, eng = truth(tag), engines(tag, 4, prec)
    x, V, U = tr.x.to(DEV), tr.V_h.to(DEV), tr.U_out.to(DEV)
    mask = tr.mask.to(DEV) if masked else None
    eng.pmp_primal(x, T, tr.at, mask, use_et=False, tap="dec")
    want = (eng.pmp_jvp(V), eng.pmp_vjp(U), eng.pmp_primal_eps())
    m8 = mask.to(torch.uint8).contiguous().view(-1) if masked else None
    _primal_tap_dh_raw(eng, x, tr.at, m8, False, None)
    got = (eng.pmp_jvp(V), eng.pmp_vjp(U), eng.pmp_primal_eps())
    eng.pmp_primal(x, T, tr.at, mask, use_et=False, tap="dec", dh=None)
    again = (eng.pmp_jvp(V), eng.pmp_vjp(U), eng.pmp_primal_eps())
    for a, b, c in zip(want, got, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    # an all-zero shift goes through the injection and still lands on the same values
    eng.pmp_primal(x, T, tr.at, mask, use_et=False, tap="dec", dh=torch.zeros(tr.n_h, device=DEV))
    assert torch.equal(eng.pmp_primal_eps(), want[2])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("masked,use_et", [(False, True), (True, False)])
@pytest.mark.parametrize("max_batch,k", [(2, 3), (4, 5)])
@pytest.mark.parametrize("tag", sorted(CFGS))
def test_shifted_operator(tag, max_batch, k, masked, use_et, prec, engines):
    tr, eng = truth(tag), engines(tag, max_batch, prec)
    JV_t, JtU_t = tr.dec(True, masked, use_et)
    JV_0, JtU_0 = tr.dec(False, masked, use_et)
    moved = min(rel(JV_0[:k], JV_t[:k]), rel(JtU_0[:k], JtU_t[:k]))
    assert moved > 10 * JAC[prec]                 # the unshifted linearisation misses the oracle: the case can tell the two apart
    x, dh = tr.x.to(DEV), tr.dh.to(DEV)
    eng.pmp_primal(x, T, tr.at, tr.mask.to(DEV) if masked else None, use_et=use_et, tap="dec", dh=dh)
    V, U = tr.V_h[:k].contiguous().to(DEV), tr.U_out[:k].contiguous().to(DEV)
    JV, JtU = eng.pmp_jvp(V), eng.pmp_vjp(U)
    eps = eng.pmp_primal_eps()
    assert tuple(JV.shape) == (k, tr.n) and tuple(JtU.shape) == (k, tr.n_h)
    adj = max(_adjoint(V, JV, U, JtU), _adjoint(V, JV, JV, eng.pmp_vjp(JV.contiguous())))
    print(f"{tag} {prec} shifted dec jvp {rel(JV, JV_t[:k]):.2e} vjp {rel(JtU, JtU_t[:k]):.2e} adjoint {adj:.2e}; the shift moved the products by "
          f"{moved:.2e}; against the unshifted oracle jvp {rel(JV, JV_0[:k]):.2e}")
    assert rel(JV, JV_t[:k]) < JAC[prec] and rel(JtU, JtU_t[:k]) < JAC[prec]
    assert adj < 1e-4
    if masked:
        assert float(JV[:, ~tr.mask.reshape(-1).to(DEV)].abs().max()) == 0.0
    # the network output at the linearisation point is the shifted forward, to the last bit; asked for after the products: they keep it
    assert torch.equal(eps, eng.pmp_primal_eps())
    fwd = eng.unet_forward(x, T, dh=dh.reshape(1, -1))
    assert torch.equal(eps.reshape(-1), fwd.reshape(-1))
    assert not torch.equal(fwd, eng.unet_forward(x, T))
    with pytest.raises(RuntimeError, match="has not been called"):       # the forwards dropped the primal
        eng.pmp_jvp(V)


def test_refusals(engines):
    from loco_edit_amd.hip import LocoEngine
    tr, eng = truth("tiny_ddpm"), engines("tiny_ddpm", 4, "f32")
    x = tr.x.to(DEV)
    with pytest.raises(ValueError, match="needs tap='dec'"):
        eng.pmp_primal(x, T, tr.at, None, tap="enc", dh=tr.dh.to(DEV))
    with pytest.raises(ValueError, match="needs tap='dec'"):
        eng.pmp_primal(x, T, tr.at, None, dh=tr.dh.to(DEV))
    with pytest.raises(ValueError, match="dh must have"):
        eng.pmp_primal(x, T, tr.at, None, tap="dec", dh=torch.zeros(tr.n, device=DEV))
    dec = LocoEngine(TINY_DECODER, max_batch=2, device=torch.device(DEV))
    dec.load_state_dict(synth_params(TINY_DECODER, 0))
    z = torch.randn(1, 4, 16, 16, device=DEV)
    with pytest.raises(RuntimeError, match="loco_pmp_primal_tap_dh: this network has no h-space tap"):
        _primal_tap_dh_raw(dec, z, 1.0, None, True, None)
