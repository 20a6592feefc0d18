"""MI355X: the Asyrp block f_t alone (csrc/asyrp.hip through hip.LocoAsyrpBlock) against the float64 run of its restatement
tests/asyrp_oracle.py.

Shapes (B, C, H, W, E): (1, 64, 8, 8, 128) TINY_DDPM's bottleneck; (3, 96, 4, 4, 64) an odd batch, C no power of two, groups of
3 channels, a 16-pixel map (half a tile of the product kernel, a quarter of a wave in the per-channel sums); (2, 512, 8, 8, 512)
the headline network's bottleneck.  h has an offset of 10 and a spread of 1 (a one-pass fp32 variance would show), every
parameter is away from its initial value so that no gradient is trivially zero, and s is 1 / 0.7 / 1.3.

Bar: for each quantity -- dh, the cotangent of h, each of the ten parameter gradients for a seeded cotangent, each parameter
after 5 Adam steps (lr 1e-2) on L = 0.5 |dh - target|^2 -- the error max |x - x64| / max |x64| of the restatement's fp32 CPU run
against its float64 run is measured on every case of the file; the largest is the yardstick, and the HIP result stays within
4 x it (the margin this project gives its exact-fp32 units for another summation order, as in test_gpu_pca.py).  Both are
printed.  Measured on MI355X (yardstick / worst HIP error over the three shapes):
  dh 5.1e-07 / 1.0e-07; d L / d h 1.1e-06 / 2.1e-07; gradients g1 1.6e-06 / 1.6e-07, b1 9.1e-07 / 1.2e-07, W1 1.2e-06 / 1.4e-07,
  c1 1.0e-06 / 1.6e-07, Wt 9.9e-07 / 2.0e-07, ct 1.0e-06 / 1.6e-07, g2 5.2e-07 / 1.1e-07, b2 4.1e-07 / 8.5e-08, W2 5.2e-07 / 9.0e-08,
  c2 1.6e-07 / 6.4e-08; after 5 Adam steps g1 1.6e-07 / 1.2e-07, b1 2.6e-07 / 1.2e-07, W1 4.9e-05 / 2.1e-06, c1 8.5e-07 / 1.1e-07,
  Wt 1.9e-06 / 1.3e-07, ct 9.3e-07 / 8.8e-08, g2 1.4e-07 / 1.4e-07, b2 1.6e-07 / 9.3e-08, W2 5.9e-06 / 3.6e-07, c2 2.9e-07 / 1.1e-07
  (Adam divides by sqrt(v): an entry whose gradient is near zero amplifies that gradient's rounding, hence W1's yardstick).
Further: accumulation over two backward calls equals the sum of the two gradients up to the roundings of the three stored
values (|acc - (a + b)| <= 2^-23 (|a| + |b|): the store takes `old + this call's sum` formed in double and rounded once); two
identical call sequences are bit-identical; the initial W2 = c2 = 0 gives exactly zero; s = 2 and s = -0.5 scale dh and every
gradient exactly; refusals by their messages.  The kernels read single floats, so there is no alignment contract to refuse.
"""
import pytest
import torch

import asyrp_oracle as ao

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
LR = 1e-2
STEPS = 5
CASES = {"tiny": ((1, 64, 8, 8, 128), 1.0), "odd": ((3, 96, 4, 4, 64), 0.7), "headline": ((2, 512, 8, 8, 512), 1.3)}


def Block(*a, **k):
    from loco_edit_amd.hip import LocoAsyrpBlock as cls
    return cls(*a, device=torch.device(DEV), **k)


class Case:
    """Inputs and both oracle runs of one shape: computed once, shared, never written to."""

    def __init__(self, shape, s):
        B, C, H, W, E = shape
        self.shape, self.s = shape, s
        gen = torch.Generator().manual_seed(C + B)
        self.p = ao.random_params(C, E, seed=C)
        self.h = 10 + torch.randn(B, C, H, W, generator=gen)
        self.e = torch.randn(E, generator=gen)
        self.g = torch.randn(B, C, H, W, generator=gen)
        self.target = torch.randn(B, C, H, W, generator=gen)
        self.ref, self.err32 = {}, {}
        runs = {}
        for dt in (torch.float64, torch.float32):
            p = {k: v.to(dt) for k, v in self.p.items()}
            h, e, g, tgt = self.h.to(dt), self.e.to(dt), self.g.to(dt), self.target.to(dt)
            dh, gh, grads = ao.block_grads(p, h, e, g, s, EPS)
            trained = ao.train_quadratic(p, h, e, tgt, STEPS, LR, s, EPS)
            runs[dt] = {"dh": dh, "g_h": gh, **{f"grad:{k}": grads[k] for k in ao.PARAMS}, **{f"adam:{k}": trained[k] for k in ao.PARAMS}}
        self.ref = runs[torch.float64]
        self.err32 = {k: ao.rel_err(runs[torch.float32][k], self.ref[k]) for k in self.ref}


_CASES = {}


def cases():
    if not _CASES:
        for tag, (shape, s) in CASES.items():
            _CASES[tag] = Case(shape, s)
    return _CASES


def yardstick():
    """{quantity: the largest fp32-oracle error over the file's cases}"""
    cs = list(cases().values())
    return {k: max(c.err32[k] for c in cs) for k in cs[0].err32}


def block_of(c, max_batch=None):
    B, C, H, W, E = c.shape
    blk = Block(C, H, W, E, max_batch=max_batch or B, gn_eps=EPS, seed=None)
    blk.load_state_dict(c.p)
    return blk


def check(tag, got, c):
    yard = yardstick()
    bad = []
    for k, v in got.items():
        err = ao.rel_err(v.cpu(), c.ref[k])
        print(f"{tag} {k}: yardstick {yard[k]:.2e}, this case's fp32 oracle {c.err32[k]:.2e}, HIP {err:.2e}")
        if not err <= 4 * yard[k]:
            bad.append((k, err, yard[k]))
    assert not bad, bad


@pytest.mark.parametrize("tag", sorted(CASES))
def test_forward_and_gradients(tag):
    c = cases()[tag]
    blk = block_of(c)
    dh = blk.forward(c.h.to(DEV), c.e.to(DEV), s=c.s)
    blk.zero_grad()
    gh = blk.backward(c.g.to(DEV), need_g_h=True)
    grads = blk.grads()
    check(tag, {"dh": dh, "g_h": gh, **{f"grad:{k}": grads[k] for k in ao.PARAMS}}, c)
    # the parameters are untouched by forward / backward
    sd = blk.state_dict()
    assert all(torch.equal(sd[k], c.p[k]) for k in ao.PARAMS)


def train(blk, c, steps):
    h, e, tgt = c.h.to(DEV), c.e.to(DEV), c.target.to(DEV)
    for t in range(1, steps + 1):
        dh = blk.forward(h, e, s=c.s)
        blk.zero_grad()
        blk.backward(dh - tgt)
        blk.adam_step(t, LR)
    return blk.state_dict()


@pytest.mark.parametrize("tag", sorted(CASES))
def test_adam_steps(tag):
    c = cases()[tag]
    sd = train(block_of(c), c, STEPS)
    check(tag, {f"adam:{k}": sd[k] for k in ao.PARAMS}, c)
    assert not any(torch.equal(sd[k], c.p[k]) for k in ao.PARAMS)


@pytest.mark.parametrize("tag", ["tiny", "odd"])
def test_gradients_accumulate(tag):
    c = cases()[tag]
    blk = block_of(c)
    h, e = c.h.to(DEV), c.e.to(DEV)
    g2 = torch.randn(c.g.shape, generator=torch.Generator().manual_seed(77))
    blk.forward(h, e, s=c.s)
    single = []
    for g in (c.g, g2):
        blk.zero_grad()
        blk.backward(g.to(DEV))
        single.append(blk.grads())
    blk.zero_grad()
    assert not any(v.any() for v in blk.grads().values())
    blk.backward(c.g.to(DEV))
    blk.backward(g2.to(DEV))
    acc = blk.grads()
    for k in ao.PARAMS:
        a, b = single[0][k].double(), single[1][k].double()
        assert bool(((acc[k].double() - (a + b)).abs() <= 2.0 ** -23 * 1.01 * (a.abs() + b.abs()) + 1e-37).all()), k


def test_bit_identical_runs():
    c = cases()["odd"]
    outs = []
    for _ in range(2):
        blk = block_of(c)
        sd = train(blk, c, 3)
        dh = blk.forward(c.h.to(DEV), c.e.to(DEV), s=c.s)
        gh = blk.backward(c.g.to(DEV), need_g_h=True)
        outs.append((sd, dh.cpu(), gh.cpu(), blk.grads()))
    (sa, da, ga, gra), (sb, db, gb, grb) = outs
    assert torch.equal(da, db) and torch.equal(ga, gb)
    assert all(torch.equal(sa[k], sb[k]) and torch.equal(gra[k], grb[k]) for k in ao.PARAMS)


def test_untrained_block_is_the_identity_edit():
    B, C, H, W, E = CASES["tiny"][0]
    c = cases()["tiny"]
    blk = Block(C, H, W, E, max_batch=2, gn_eps=EPS, seed=0)
    sd = blk.state_dict()
    assert not sd["W2"].any() and not sd["c2"].any() and sd["W1"].any()
    dh = blk.forward(c.h.to(DEV), c.e.to(DEV), s=1.7)
    assert dh.shape == c.h.shape and not dh.any()


@pytest.mark.parametrize("s", [2.0, -0.5])
def test_scale_is_exact_for_powers_of_two(s):
    c = cases()["odd"]
    blk = block_of(c)
    h, e, g = c.h.to(DEV), c.e.to(DEV), c.g.to(DEV)
    out = []
    for scale in (1.0, s):
        dh = blk.forward(h, e, s=scale)
        blk.zero_grad()
        gh = blk.backward(g, need_g_h=True)
        out.append((dh.cpu(), gh.cpu(), blk.grads()))
    (d1, g1, gr1), (ds, gs, grs) = out
    assert torch.equal(ds, s * d1) and torch.equal(gs, s * g1)
    assert all(torch.equal(grs[k], s * gr1[k]) for k in ao.PARAMS)


def test_refusals():
    B, C, H, W, E = CASES["tiny"][0]
    with pytest.raises(RuntimeError, match="not a positive multiple of the 32 GroupNorm groups"):
        Block(48, H, W, E)
    blk = Block(C, H, W, E, max_batch=1, gn_eps=EPS, seed=0)
    h = torch.randn(1, C, H, W, device=DEV)
    e = torch.randn(E, device=DEV)
    with pytest.raises(RuntimeError, match="no records"):
        blk.backward(h)
    blk.forward(h, e, keep_records=False)
    with pytest.raises(RuntimeError, match="no records"):
        blk.backward(h)
    blk.forward(h, e)
    blk.backward(h)
    with pytest.raises(RuntimeError, match=r"outside \[1, max_batch = 1\]"):
        blk.forward(torch.randn(2, C, H, W, device=DEV), e)
    with pytest.raises(ValueError, match="expected shape"):
        blk.forward(h, torch.randn(E + 1, device=DEV))
    with pytest.raises(ValueError, match="expected torch.float32"):
        blk.forward(h.double(), e)
    empty = Block(C, H, W, E, seed=None)
    with pytest.raises(RuntimeError, match="missing parameter g1"):
        empty.forward(h, e)
