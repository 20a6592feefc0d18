"""CPU: the float64 reference of tests/token_oracle.py against torch's own operators and torch.func, and its tolerances against fp32
restatements of every launcher with and without planted errors.

  - the reference means what the engine means: ln_fwd is F.layer_norm over the channel axis of the [C][T] layout, ln_tan / ln_cot are
    torch.func.jvp / vjp through it (to the 1e-6 of the fp32-rounded {mean, rstd} they take as given); GEGLU kind 0 is
    value * F.gelu(gate), kinds 1 and 2 its jvp and vjp; temb is the sinusoid, dense, act, dense, act of the float oracle the parity
    tests use; pool and upsample are F.avg_pool2d * 4 * scale and F.interpolate(mode="nearest") * scale; ddim_step and latent_sample
    the formulas of their kernel comments; the adjoint identities hold for the reference itself;
  - an fp32 torch restatement of every launcher in the kernel's own operation order (token_oracle.restate32) stays inside tau on
    EVERY case of the table, at every offset level, and no bound's scale A is zero where an output is not an exact zero by contract;
  - the check rejects planted errors on that restatement: each lands above 1 x tau on some element of some case (PLANTS below).

The temb angle: the kernel takes sin / cos of the fp32 product float32(t) * freq[i], and so does the reference.  A reference that
took them of the exact product would sit up to |angle| u (3e-5 at t = 999) from the kernel's embedding, far outside the 2 u the
embedding is allowed: the plant "angle_not_rounded" is that other convention, and the check tells the two apart AT THE EMBEDDING --
the fp32-rounded angle is the one asserted.  At the launch's output it cannot: the (ch + 8) u accumulation bound of dense0 (1e-5 of
|w0| |emb|) is of the size of what one angle's rounding moves the output by.

Worst share of tau of the fp32 restatements (this machine's torch, max over the cases of a launcher):
  ln_fwd 0.114   ln_tan 0.012   ln_cot 0.018   geglu kind 0 / 1 / 2 0.080 / 0.055 / 0.074   temb < 0.001   temb_proj 0.001
  pool2x2_sum 0.095   upsample2x 0.190  copy 0.250   masked_axpby 0.162   cot_seed 0.250   ddim_step 0.132   latent_sample 0.070
  lincomb 0.055   add 0.250
(0.250 = 1 / MARGIN: a single correctly rounded operation sits at most half an ulp = u from the float64 value, against MARGIN u.
temb's bound is a chain of two dense layers' worst-case accumulations through two activations' slope bounds: far above what a
faithful evaluation uses, and still 1000 times below the planted errors.)
"""
import math

import pytest
import torch
import torch.nn.functional as F

import token_oracle as to

D = torch.float64
IDS = [c["id"] for c in to.CASES]


def _close(a, b, tol=1e-11):
    scale = max(float(b.abs().max()), 1.0)
    assert float((a - b).abs().max()) <= tol * scale, (float((a - b).abs().max()), scale)


def _find(op, **kw):
    return next(c for c in to.CASES if c["op"] == op and all(c.get(k) == v for k, v in kw.items()))


# ---- the reference means what the engine means --------------------------------------------------------------------------------

def test_ln_fwd_is_layer_norm_over_the_channel_axis():
    c = _find("ln_fwd", C=96, T=48, level=0.0)
    inp = to.inputs(c)
    refs, _ = to.reference(c, inp)
    want = F.layer_norm(inp["x"].transpose(1, 2), (c["C"],), inp["gamma"], inp["beta"], eps=c["eps"]).transpose(1, 2)
    _close(refs["y"][0], want)
    st = refs["stats"][0]
    assert torch.equal(refs["y"][0][0, :, 3], inp["beta"])                      # the token of equal channels: y = beta
    _close(st[0, 1, 3:4], torch.tensor([1 / math.sqrt(c["eps"])], dtype=D))      # rstd = rsqrt(eps)
    assert torch.equal(refs["y"][0][1, :, 5], inp["beta"]) and float(st[1, 0, 5]) == 0.0


@pytest.mark.parametrize("base", [False, True])
def test_ln_tan_is_the_jvp_and_ln_cot_the_vjp(base):
    ct, cc = _find("ln_tan", C=96, T=16, level=0.0), _find("ln_cot", C=96, T=16, level=0.0, base=base)
    inp = to.inputs(ct)
    ln = lambda x: F.layer_norm(x.transpose(0, 1), (ct["C"],), inp["gamma"], inp["beta"], eps=ct["eps"]).transpose(0, 1)
    tan = to.reference(ct, inp)[0]["out"][0]
    cot = to.reference(cc, inp)[0]["out"][0]
    for b in range(ct["B"]):
        _close(tan[b], torch.func.jvp(ln, (inp["prim"],), (inp["d"][b],))[1], 1e-6)
        want = torch.func.vjp(ln, inp["prim"])[1](inp["g"][b])[0] + (inp["base"][b] if base else 0)
        _close(cot[b], want, 1e-6)


def test_geglu_is_value_gelu_gate_with_its_jvp_and_vjp():
    cs = [_find("geglu", kind=k, B=2) for k in (0, 1, 2)]
    inp = to.inputs(cs[0])
    n4 = cs[0]["n4"]
    fn = lambda f: f[:n4] * F.gelu(f[n4:])
    r = [to.reference(c, inp)[0]["out"][0] for c in cs]
    for b in range(2):
        _close(r[0][b], fn(inp["f"][b]))
        _close(r[1][b], torch.func.jvp(fn, (inp["f"][0],), (inp["df"][b],))[1])
        _close(r[2][b], torch.func.vjp(fn, inp["f"][0])[1](inp["g"][b])[0])


@pytest.mark.parametrize("cid", [c["id"] for c in to.CASES if c["op"] == "temb" and c["ch"] < 100])
def test_temb_is_sinusoid_dense_act_dense_act(cid):
    c = to.BY_ID[cid]
    inp = to.inputs(c)
    half = c["ch"] // 2
    a = to.temb_angle(c["t"], inp["freq"])
    parts = [torch.cos(a), torch.sin(a)] if c["cos_first"] else [torch.sin(a), torch.cos(a)]
    emb = torch.cat(parts + [torch.zeros(c["ch"] - 2 * half, dtype=D)])
    if c["add_in"]:
        emb = emb + inp["add_in"]
    act = F.gelu if c["act"] else F.silu
    h = act(F.linear(emb, inp["w0"], inp["b0"]))
    pre = F.linear(h, inp["w1"], inp["b1"]) + (inp["add"] if c["add"] else 0)
    _close(to.reference(c, inp)[0]["out"][0], act(pre))
    p = to.BY_ID[next(x["id"] for x in to.CASES if x.get("after") == cid)]
    tact = to._f32(act(pre))
    _close(to.reference(p, inp, tact)[0]["out"][0], F.linear(tact, inp["pw"], inp["pb"] if p["bias"] else None))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 0.25, 0.37])
def test_pool_and_upsample_are_avg_pool_and_nearest(scale, acc):
    s = float(torch.tensor(scale, dtype=torch.float32))
    cp, cu = _find("pool2x2_sum", H=6, W=10, scale=scale, acc=acc), _find("upsample2x", H=6, W=10, scale=scale, acc=acc)
    inp = to.inputs(cp)
    _close(to.reference(cp, inp)[0]["out"][0], F.avg_pool2d(inp["x"], 2) * 4 * s + (inp["small0"] if acc else 0))
    _close(to.reference(cu, inp)[0]["out"][0], F.interpolate(inp["y"], scale_factor=2, mode="nearest") * s + (inp["large0"] if acc else 0))


def test_ddim_step_and_latent_sample_are_their_formulas():
    c = _find("ddim_step", noise=1, x0=1)
    inp = to.inputs(c)
    cx, cxe, cn0, cne, cnz = inp["f"]
    refs, _ = to.reference(c, inp)
    p = (inp["x"] - inp["e"] * cxe) / cx
    _close(refs["out2"][0], p)
    _close(refs["out"][0], cn0 * p + cne * inp["e"] + cnz * inp["noise"])
    c = _find("latent_sample", noise=1)
    inp = to.inputs(c)
    n = c["n"]
    std = torch.exp(0.5 * torch.clamp(inp["mom"][:, n:], -30.0, 20.0))
    _close(to.reference(c, inp)[0]["out"][0], inp["scale"] * (inp["mom"][:, :n] + std * inp["noise"]))
    assert float(inp["mom"][:, n:].min()) < -30 and float(inp["mom"][:, n:].max()) > 20


@pytest.mark.parametrize("aid", [a["id"] for a in to.ADJOINTS if "cap" not in a["id"] and "525288" not in a["id"]])
def test_the_reference_satisfies_the_adjoint_identities(aid):
    a = next(x for x in to.ADJOINTS if x["id"] == aid)
    ca, cb = to.BY_ID[a["a"]], to.BY_ID[a["b"]]
    ia, ib = to.inputs(ca), to.inputs(cb)
    oa, ob = to.reference(ca, ia)[0]["out"][0], to.reference(cb, ib)[0]["out"][0]
    zero = torch.zeros_like
    diff, _ = to.adjoint(to.adjoint_io(ca, ia), oa, zero(oa), to.adjoint_io(cb, ib), ob, zero(ob))
    assert diff <= 1e-10 * max(1.0, float((oa * to.adjoint_io(cb, ib)).abs().sum())), diff


# ---- the fp32 restatements stay inside tau; no scale vanishes ------------------------------------------------------------------

def _tact(c, plant=None):
    """temb_proj's input: the restated temb before it"""
    if c["op"] != "temb_proj":
        return None
    a = to.BY_ID[c["after"]]
    return to.restate32(a, to.inputs(a))["out"].to(D)


SHARES = {}


@pytest.mark.parametrize("cid", IDS)
def test_fp32_restatement_stays_inside_tau(cid):
    c = to.BY_ID[cid]
    inp = to.inputs(c)
    tact = _tact(c)
    refs, info = to.reference(c, inp, tact)
    r = to.check(to.restate32(c, inp, tact=tact), refs, info)
    key = to.launcher_key(c)
    SHARES[key] = max(SHARES.get(key, 0.0), r["share"])
    print(f"{cid}: worst share of tau {r['share']:.3f} ({', '.join(f'{k} {v:.3f}' for k, v in r['shares'].items())})")
    assert r["share"] <= 1.0, r["msg"]
    assert r["unwritten"] == 0 and r["bits_bad"] == 0 and r["zero_bad"] == 0, r
    live = ~info["zero"] if "zero" in info else torch.ones_like(info["A"], dtype=torch.bool)
    assert float(info["A"][live].min()) > 0.0, "a bound's scale vanishes"
    for name, (ref, tau) in refs.items():
        assert bool(torch.isfinite(tau).all()) and float(tau.min()) > 0.0, name


def test_fp32_restatement_shares_are_reported():
    """prints the worst share per launcher of the cases that ran before it (the figures of this file's docstring)"""
    print("  ".join(f"{k} {v:.3f}" for k, v in SHARES.items()))
    assert all(v <= 1.0 for v in SHARES.values())


# ---- planted errors --------------------------------------------------------------------------------------------------------------

def _ln(op, **kw):
    return [c["id"] for c in to.CASES if c["op"] == op and c["level"] == 0.0 and all(c.get(k) == v for k, v in kw.items())]


def _ids(op, **kw):
    return [c["id"] for c in to.CASES if c["op"] == op and all(c.get(k) == v for k, v in kw.items())]


PLANTS = [      # (plant, the cases it is tried on: it must land above tau on at least one)
    ("mean_over_c_minus_1", _ln("ln_fwd")),
    ("eps_outside_sqrt", _ln("ln_fwd")),
    ("rstd_as_variance", _ln("ln_fwd")),
    ("sample_slot", _ln("ln_fwd") + _ln("ln_tan") + _ln("ln_cot")),
    ("tangent_no_gamma", _ln("ln_tan")),
    ("no_xhat_m2", _ln("ln_tan") + _ln("ln_cot")),
    ("gamma_after_means", _ln("ln_cot")),
    ("base_ignored", _ln("ln_cot", base=True)),
    ("neighbour_stats", _ln("ln_tan") + _ln("ln_cot")),
    ("gelu_tanh", _ids("geglu", B=2)),
    ("quick_gelu", _ids("geglu", B=2)),
    ("no_dgate_term", _ids("geglu", B=2, kind=1) + _ids("geglu", B=2, kind=2)),
    ("halves_swapped", _ids("geglu", B=2)),
    ("sin_cos_swapped", _ids("temb", ch=32) + _ids("temb", ch=33)),
    ("add_after_act", _ids("temb", ch=32, add=1)),
    ("angle_not_rounded", _ids("temb", ch=32, t=999.0) + _ids("temb", ch=33, t=437.25)),
    ("pool_no_scale", _ids("pool2x2_sum", scale=0.25, B=2) + _ids("pool2x2_sum", scale=0.37)),
    ("accumulate_ignored", _ids("pool2x2_sum", acc=1) + _ids("upsample2x", acc=1)),
    ("hw_swapped", _ids("pool2x2_sum", B=2) + _ids("upsample2x", B=2)),
    ("mask_as_product", _ids("masked_axpby", n=1000, poison=True) + _ids("cot_seed", n=1000, poison=True)),
    ("mask2_from_split_plus_1", _ids("masked_axpby", split=1) + _ids("cot_seed", split=1)),
    ("tail_dropped", _ids("lincomb", n=4099)),
]


@pytest.mark.parametrize("plant, cids", PLANTS, ids=[p[0] for p in PLANTS])
def test_planted_errors_are_rejected(plant, cids):
    assert cids, "the plant has no case"
    hit = []
    for cid in cids:
        c = to.BY_ID[cid]
        inp = to.inputs(c)
        refs, info = to.reference(c, inp)
        outs = to.restate32(c, inp, plant=plant)
        r = to.check(outs, refs, info)
        if plant == "angle_not_rounded":
            # told apart at the embedding: behind dense0 its (ch + 8) u |w0| |emb| accumulation bound, 1e-5, covers the 3e-5 |w0[o][i]| that one
            # angle's rounding moves the output by.  The unplanted restatement's embedding is inside its 2 u bound, the other convention's is not.
            emb, t_emb = info["emb"]
            assert to.worst(to.restate32(c, inp)["_emb"], emb, t_emb + to.EPS_ABS, "emb")[0] <= 1.0
            r = dict(r, share=to.worst(outs["_emb"], emb, t_emb + to.EPS_ABS, "emb")[0])
        if r["share"] > 1.0 or r["zero_bad"]:
            hit.append((cid, r["share"]))
    print(f"{plant}: above tau on {len(hit)} of {len(cids)} cases, e.g. {hit[:2]}")
    assert hit, f"{plant} stayed inside tau on every case"
    if plant in ("tangent_no_gamma", "gelu_tanh", "quick_gelu", "sin_cos_swapped", "hw_swapped",
                 "mask_as_product", "tail_dropped", "pool_no_scale", "accumulate_ignored", "base_ignored", "no_xhat_m2", "gamma_after_means"):
        assert len(hit) == len(cids), f"{plant} passed on {sorted(set(cids) - {h[0] for h in hit})}"
