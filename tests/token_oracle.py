"""Float64 reference of the token-wise and pointwise launchers (xfmr.hip: LayerNorm forward / tangent / cotangent, GEGLU; misc.hip: the
time embedding and its projections, 2x2 sum-pool and nearest x2, copy, the masked seeds, the DDIM / latent / linear-combination
steps), the tolerances of their checks and the case table of tests/test_gpu_token_oracle.py and tests/test_token_oracle_host.py.

    inputs(case)            seeded operands, float64 tensors holding float32 values (dense; strides are the GPU test's business)
    reference(case, inp)    {output name: (ref, tau)}: the launch in float64 and the bound |out - ref| <= tau on every element
    restate32(case, inp)    the launch restated in torch float32 in the kernel's own order of operations (CPU test); plant = an error
    check(outs, refs)       worst share of tau per output, with the worst element's index
    ADJOINTS / adjoint()    <A(d), g> = <d, A^T(g)> from two cases' outputs, bound sum |weight| tau

Where a launcher reads what an earlier launch computed (sprim = {mean, rstd} of ln_tan / ln_cot, fprim of GEGLU kinds 1 and 2, tact
of temb_proj) the reference takes the caller's fp32 values as given: each launch is one unit under test.

Tolerances have the project's form tau = MARGIN (k u + e) A + 1e-30 (tol()): u = 2^-24, k the roundings on the kernel's path (an
accumulation of n terms counts n + 8), A the magnitude of the quantity BEFORE cancellation from the reference alone (abs forms
below: a difference x - mean counts |x| + |mean|, an activation |f(y)| + |f'(y)| |y| as conv_oracle.prologue does), e the error
of the same expression in float32 torch relative to A (conv_oracle.prologue_term's reading of an fp32 activation or derivative;
e_term()).  Bounds of a composed launch (LayerNorm, temb) propagate the bounds of its parts; their docstrings count the roundings.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List

import torch

import conv_oracle as co
import gemm_oracle as go

MARGIN = co.MARGIN
U = 2.0 ** -24
EPS_ABS = 1e-30
D = torch.float64
F = torch.float32
ACT_SILU, ACT_GELU = 0, 1
LEVELS = (0.0, 50.0, 1000.0)      # |mean| / std of the affected tokens: the regimes of tests/norm_offsets.py
SQH = 0.7071067811865476
PHI0 = 0.3989422804014327


def _f32(t):
    return t.to(F).to(D)


def tol(k, A, e=0.0):
    return MARGIN * (k * U + e) * A + EPS_ABS


def e_term(fn, args, A) -> float:
    """error of the float32-torch evaluation of fn relative to its absolute form A (conv_oracle.prologue_term)"""
    r64 = fn(*args)
    r32 = fn(*[a.to(F) if torch.is_tensor(a) else a for a in args]).to(D)
    return float(((r32 - r64).abs() / A.clamp_min(1e-300)).max())


def act_f(y, act):
    return co._gelu(y) if act == ACT_GELU else co._silu(y)


def act_d(y, act):
    return co._dgelu(y) if act == ACT_GELU else co._dsilu(y)


def act_abs(y, act):
    """|f(y)| + |f'(y)| |y|; GELU's 1 + erf counted as 1 + |erf| (it cancels in the left tail)"""
    fa = 0.5 * y.abs() * (1 + torch.erf(y * SQH).abs()) if act == ACT_GELU else act_f(y, act).abs()
    return fa + act_d(y, act).abs() * y.abs()


def gelu_abs(g):
    return 0.5 * g.abs() * (1 + torch.erf(g * SQH).abs())


def dgelu_abs(g):
    return 0.5 * (1 + torch.erf(g * SQH).abs()) + g.abs() * PHI0 * torch.exp(-0.5 * g * g)


def _lip_silu() -> float:
    x = torch.arange(-120000, 120001, dtype=D) * 1e-4
    y = co._silu(x)
    return float(((y[1:] - y[:-1]).abs() / 1e-4).max())


LIP = {ACT_SILU: _lip_silu(), ACT_GELU: go.LIP["gelu"]}      # largest slope of the activation, as gemm_oracle takes GELU's


# ---------------------------------------------------------------------------------------------------------------------------
# cases

CASES: List[dict] = []
ADJOINTS: List[dict] = []      # dict(id, a, b): <out_a, in_b> = <in_a, out_b>


def _case(op, cid, **kw):
    c = dict(op=op, id=f"{op}-{cid}", **kw)
    CASES.append(c)
    return c["id"]


LN_EPS = 1e-5


def _build():
    # LayerNorm: B = 2 (padded batch and statistics strides in the GPU test), T = 16 (one workgroup) and 48 (three), three offset levels
    fwd_w = (320, 640, 1280, 64, 96, 32, 8, 768, 1024)      # NPER 5 / 10 / 20; one channel per slice; ragged; idle slices; CLIP widths
    lin_w = (320, 640, 1280, 96, 256)
    for T in (16, 48):
        for lv in LEVELS:
            tag = f"T{T}_L{int(lv)}"
            for C in fwd_w:
                _case("ln_fwd", f"C{C}_{tag}", C=C, T=T, B=2, level=lv, eps=LN_EPS, special=(C == 96 and T == 48))
            _case("ln_fwd", f"C256_inplace_{tag}", C=256, T=T, B=2, level=lv, eps=1e-6, inplace=True)      # the SAM decoder's call
            for C in lin_w:
                a = _case("ln_tan", f"C{C}_{tag}", C=C, T=T, B=2, level=lv, eps=LN_EPS)
                b = _case("ln_cot", f"C{C}_{tag}", C=C, T=T, B=2, level=lv, eps=LN_EPS, base=False)
                _case("ln_cot", f"C{C}_base_{tag}", C=C, T=T, B=2, level=lv, eps=LN_EPS, base=True)
                ADJOINTS.append(dict(id=f"ln-C{C}_{tag}", a=a, b=b))
    # GEGLU: 4 * 320 * 16 (B = 2, padded strides) and 2048 * 256 + 1000 (the grid-stride loop and a ragged last block)
    for n4, B in ((4 * 320 * 16, 2), (2048 * 256 + 1000, 1)):
        ids = [_case("geglu", f"k{kind}_n{n4}_B{B}", kind=kind, n4=n4, B=B) for kind in (0, 1, 2)]
        ADJOINTS.append(dict(id=f"geglu-n{n4}_B{B}", a=ids[1], b=ids[2]))
    # temb, each followed by temb_proj on its output: every switch takes both values at every shape
    ts = (0.0, 1.0, 999.0, 437.25)
    for si, (ch, tch) in enumerate(((32, 128), (320, 1280), (33, 132))):
        for i in range(8):
            t = ts[i % 4]
            sw = dict(cos_first=i & 1, act=(i >> 1) & 1, add=((i >> 2) + i + si) & 1, add_in=((i >> 2) + (i >> 1)) & 1, ptr=((i >> 2) + i) & 1)
            tid = _case("temb", f"ch{ch}_{tch}_t{t:g}_c{sw['cos_first']}a{sw['act']}d{sw['add']}i{sw['add_in']}p{sw['ptr']}", ch=ch, tch=tch, t=t, **sw)
            _case("temb_proj", f"ch{ch}_{tch}_{i}_b{(i >> 2) & 1}", tch=tch, cout=10, bias=(i >> 2) & 1, after=tid)
    # 2x2 sum-pool and nearest x2: non-square maps, B = 2 with strides of their own, three scales, accumulate, one case over the cap
    for op in ("pool2x2_sum", "upsample2x"):
        for (H, W) in ((6, 10), (10, 6)):      # the small side; the large side is 12 x 20 / 20 x 12
            for scale in (1.0, 0.25, 0.37):
                for acc in (0, 1):
                    _case(op, f"C3_{H}x{W}_s{scale:g}_acc{acc}", C=3, H=H, W=W, B=2, scale=scale, acc=acc)
    _case("pool2x2_sum", "C3_300x584_cap", C=3, H=300, W=584, B=1, scale=0.25, acc=0)      # 525 600 outputs > 2048 * 256
    _case("upsample2x", "C3_150x292_cap", C=3, H=150, W=292, B=1, scale=0.25, acc=0)       # 525 600 outputs
    for scale in (1.0, 0.25):      # the two pairings of engine.hip: avg-pool / its transpose (0.25) and nearest / its transpose (1)
        for (H, W) in ((6, 10), (10, 6)):
            ADJOINTS.append(dict(id=f"pool-{H}x{W}_s{scale:g}", a=f"pool2x2_sum-C3_{H}x{W}_s{scale:g}_acc0", b=f"upsample2x-C3_{H}x{W}_s{scale:g}_acc0"))
    for per in (4, 2048 * 256 * 4 + 8):
        for acc in (0, 1):
            _case("copy", f"n{per}_acc{acc}", n=per, B=2, acc=acc)
    # the masked seeds: k = 3 rows of 1000; no mask, a mask, a second mask from row 1, from row 0 and from row k; null V / gX0; the cap
    for op in ("masked_axpby", "cot_seed"):
        for (m, split) in (("none", 0), ("mask", 0), ("mask2", 1), ("mask2", 0), ("mask2", 3)):
            _case(op, f"k3_n1000_{m}_s{split}", k=3, n=1000, masks=m, split=split, null=False, poison=(m != "none"))
        _case(op, "k3_n1000_mask2_s1_null", k=3, n=1000, masks="mask2", split=1, null=True, poison=True)
        _case(op, "k3_n350000_cap", k=3, n=350000, masks="mask", split=0, null=False, poison=True)      # 1 050 000 > 4096 * 256
    for noise in (0, 1):
        for x0 in (0, 1):
            _case("ddim_step", f"noise{noise}_x0{x0}", n=5000, noise=noise, x0=x0)
    for noise in (0, 1):
        _case("latent_sample", f"noise{noise}", B=2, n=4 * 33, noise=noise)
    for n in (1, 2, 3, 4):
        _case("lincomb", f"n{n}_4099", nsrc=n, n=4099, alias=False)
    _case("lincomb", "n3_4099_alias", nsrc=3, n=4099, alias=True)
    _case("lincomb", "n2_cap", nsrc=2, n=2048 * 256 * 4 + 4 * 300 + 3, alias=False)
    _case("add", "n1000", n=1000)
    _case("add", "cap", n=4096 * 256 + 1000)


_build()
BY_ID = {c["id"]: c for c in CASES}
LAUNCHERS = ("ln_fwd", "ln_tan", "ln_cot", "geglu", "temb", "temb_proj", "pool2x2_sum", "upsample2x", "copy", "masked_axpby", "cot_seed",
             "ddim_step", "latent_sample", "lincomb", "add")


def launcher_key(c) -> str:
    return f"geglu kind {c['kind']}" if c["op"] == "geglu" else c["op"]


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def _gen(*key):
    return torch.Generator().manual_seed(11 + sum(ord(ch) * (i + 1) for i, ch in enumerate(repr(key))) % 1000003)


@functools.lru_cache(maxsize=4)
def _ln_inputs(C, T, B, level, eps, special):
    """shared by the forward, tangent and cotangent cases of one shape: x [B][C][T] (unit-variance tokens, per-channel scales and
    offsets; level: an offset of level x std on every second token), the primal = x[0] with its fp32 {mean, rstd}, d, g, base"""
    g = _gen("ln", C, T, B, level, eps)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    x = rn(B, C, T) * (0.5 + torch.rand(C, generator=g, dtype=D)).view(1, -1, 1) + 0.3 * rn(C).view(1, -1, 1)
    if level:
        x = x + level * (torch.arange(T) % 2 == 0).to(D).view(1, 1, -1)
    if special:
        x[0, :, 3] = 2.5      # all channels equal: variance 0
        x[1, :, 5] = 0.0      # an all-zero padding token
    x = _f32(x)
    o = dict(x=x, gamma=_f32(1.0 + 0.3 * rn(C)), beta=_f32(0.3 * rn(C)))
    prim = x[0]
    mean = prim.mean(0)
    rstd = 1.0 / torch.sqrt(prim.var(0, unbiased=False) + eps)
    o.update(prim=prim, sprim=_f32(torch.stack([mean, rstd])), d=_f32(rn(B, C, T) + 0.5), g=_f32(rn(B, C, T) - 0.25), base=_f32(rn(B, C, T)))
    return o


@functools.lru_cache(maxsize=2)
def _geglu_inputs(n4, B):
    """f = [value | gate], gates uniform over [-8, 8] (both tails and the region around +-1); df, g"""
    g = _gen("geglu", n4, B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    f = torch.cat([rn(B, n4), 16.0 * torch.rand(B, n4, generator=g, dtype=D) - 8.0], 1)
    return dict(f=_f32(f), df=_f32(rn(B, 2 * n4)), g=_f32(rn(B, n4)))


@functools.lru_cache(maxsize=2)
def _temb_weights(ch, tch):
    g = _gen("temb", ch, tch)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    half = ch // 2
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F) / max(half - 1, 1)).to(D)      # an fp32 table, as the engine builds it
    return dict(freq=freq, w0=_f32(rn(tch, ch) / math.sqrt(ch)), b0=_f32(0.1 * rn(tch)), w1=_f32(rn(tch, tch) / math.sqrt(tch)), b1=_f32(0.1 * rn(tch)),
                add=_f32(0.5 * rn(tch)), add_in=_f32(0.5 * rn(ch)), pw=_f32(rn(10, tch) / math.sqrt(tch)), pb=_f32(0.1 * rn(10)))


@functools.lru_cache(maxsize=4)
def _resample_inputs(C, H, W, B):
    """x [B][C][2 H][2 W] (what the pool reads), y [B][C][H][W] (what the upsample reads), seeded accumulate operands of both"""
    g = _gen("resample", C, H, W, B)
    rn = lambda *s: _f32(torch.randn(*s, generator=g, dtype=D))
    return dict(x=rn(B, C, 2 * H, 2 * W), y=rn(B, C, H, W), small0=rn(B, C, H, W), large0=rn(B, C, 2 * H, 2 * W))


def inputs(c) -> Dict[str, torch.Tensor]:
    op = c["op"]
    if op in ("ln_fwd", "ln_tan", "ln_cot"):
        return _ln_inputs(c["C"], c["T"], c["B"], c["level"], c["eps"], bool(c.get("special")))
    if op == "geglu":
        return _geglu_inputs(c["n4"], c["B"])
    if op == "temb":
        return _temb_weights(c["ch"], c["tch"])
    if op == "temb_proj":
        a = BY_ID[c["after"]]
        return _temb_weights(a["ch"], a["tch"])
    if op in ("pool2x2_sum", "upsample2x"):
        return _resample_inputs(c["C"], c["H"], c["W"], c["B"])
    g = _gen(c["id"])
    rn = lambda *s: _f32(torch.randn(*s, generator=g, dtype=D))
    if op == "copy":
        return dict(x=rn(c["B"], c["n"]), out0=rn(c["B"], c["n"]))
    if op in ("masked_axpby", "cot_seed"):
        k, n = c["k"], c["n"]
        o = dict(V=rn(k, n), dE=rn(k, n), U=rn(k, n), cv=0.8125, ce=1.3125)
        mask = torch.rand(n, generator=g) < 0.6
        mask2 = torch.rand(n, generator=g) < 0.4
        o["mask"] = None if c["masks"] == "none" else mask
        o["mask2"] = mask2 if c["masks"] == "mask2" else None
        o["pass"] = pass_of(c, o)
        if c["poison"]:      # NaN and Inf OUTSIDE the mask: they must not reach the output
            off = (~o["pass"]).nonzero()
            for i, (r, j) in enumerate(off[:: max(1, len(off) // 40)].tolist()):
                v = (float("nan"), float("inf"), float("-inf"))[i % 3]
                o["V"][r, j], o["dE"][r, j], o["U"][r, j] = v, (v if i % 2 else 1.0), v
        return o
    if op == "ddim_step":
        n = c["n"]
        at, an = 0.35, 0.55      # alpha-bar of the step and of the next; eta > 0 with noise
        sig = 0.2 if c["noise"] else 0.0
        f = [math.sqrt(at), math.sqrt(1 - at), math.sqrt(an), math.sqrt(1 - an - sig * sig), sig]
        return dict(x=rn(n), e=rn(n), noise=rn(n), f=[float(torch.tensor(v, dtype=F)) for v in f])
    if op == "latent_sample":
        B, n = c["B"], c["n"]
        lv = 6.0 * torch.randn(B, n, generator=g, dtype=D)
        lv[:, :4] = torch.tensor([-40.0, -30.5, 20.5, 30.0], dtype=D)      # beyond both clamps
        return dict(mom=_f32(torch.cat([torch.randn(B, n, generator=g, dtype=D), lv], 1)), noise=rn(B, n), scale=float(torch.tensor(0.18215, dtype=F)))
    if op == "lincomb":
        return dict(src=[rn(c["n"]) for _ in range(c["nsrc"])], coef=[float(torch.tensor(v, dtype=F)) for v in (7.5, -6.5, 0.3, 1.7)[:c["nsrc"]]])
    assert op == "add", op
    return dict(a=rn(c["n"]), b=rn(c["n"]))


def pass_of(c, o):
    """[k][n] bool: the element passes the mask of its row (rows >= split use mask2 when it is given)"""
    k, n = c["k"], c["n"]
    ones = torch.ones(n, dtype=torch.bool)
    m1 = ones if o["mask"] is None else o["mask"]
    m2 = m1 if o["mask2"] is None else o["mask2"]
    return torch.stack([m2 if r >= c["split"] else m1 for r in range(k)])


# ---------------------------------------------------------------------------------------------------------------------------
# references and bounds: {name: (ref, tau)}; "bits": outputs that must equal float32(ref) bit for bit; "zero": a mask of exact zeros

def _ln_fwd_ref(c, inp):
    """mean    a sum of C fp32 terms and one division: MARGIN (u |mean| + (C + 8) u mean|x|) = t_mean.
    rstd    the kernel sums (x - m)^2 about its fp32 mean m: a mean off by delta adds delta^2 to the variance (the first-order term
            vanishes), each square carries 3 roundings, the sum C + 8; rsqrtf and the division 2 more:
            d rstd / rstd <= MARGIN (2 u + (C + 11) u / 2 var / (var + eps)) + t_mean^2 / (2 (var + eps)).
    y       (x - mean) rstd gamma + beta: the bound of the mean at the scale rstd |gamma| -- the offset term |mean| rstd |gamma| u of
            stats_oracle.tol_fwd's sh --, the bound of rstd at |xhat gamma|, and 4 roundings of A = (|x| + |mean|) rstd |gamma| + |beta|."""
    x, gamma, beta, eps, C = inp["x"], inp["gamma"].view(1, -1, 1), inp["beta"].view(1, -1, 1), c["eps"], c["C"]
    mean = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * gamma + beta
    t_mean = MARGIN * (U * mean.abs() + (C + 8) * U * x.abs().mean(1, keepdim=True))
    r_rstd = MARGIN * (2 * U + 0.5 * (C + 11) * U * var / (var + eps)) + 0.5 * t_mean ** 2 / (var + eps)
    A = (x.abs() + mean.abs()) * rstd * gamma.abs() + beta.abs()
    t_y = t_mean * rstd * gamma.abs() + ((x - mean) * rstd * gamma).abs() * r_rstd + tol(4, A)
    return dict(y=(y, t_y), stats=(torch.cat([mean, rstd], 1), torch.cat([t_mean, r_rstd * rstd], 1) + EPS_ABS)), dict(A=A)


def _ln_lin_ref(c, inp):
    """z = gamma g (cotangent, 1 rounding) or d; xhat = (x - mean) rstd from the caller's fp32 {mean, rstd}: 2 roundings, absolute form
    (|x| + |mean|) rstd.  m1 = mean_c z: C + 8 (+ 1); m2 = mean_c xhat z: C + 8 + 3 (+ 1), A = mean_c |xhat|_abs |z|.
    out = rstd [gamma] (z - m1 - xhat m2) [+ base]: the bounds of m1 and m2 at the scales rstd |gamma| and rstd |gamma xhat|, and 8
    roundings of A = rstd |gamma| (|z| + |m1| + |xhat|_abs |m2|) + |base|."""
    cot = c["op"] == "ln_cot"
    C = c["C"]
    x, gamma = inp["prim"].unsqueeze(0), inp["gamma"].view(1, -1, 1)
    mean, rstd = inp["sprim"][0].view(1, 1, -1), inp["sprim"][1].view(1, 1, -1)
    d = inp["g"] if cot else inp["d"]
    z = gamma * d if cot else d
    za = z.abs()
    xh = (x - mean) * rstd
    xha = (x.abs() + mean.abs()) * rstd
    m1 = z.mean(1, keepdim=True)
    m2 = (xh * z).mean(1, keepdim=True)
    k = C + 8 + int(cot)
    t1 = tol(k, za.mean(1, keepdim=True)) + MARGIN * U * m1.abs()
    t2 = tol(k + 3, (xha * za).mean(1, keepdim=True)) + MARGIN * U * m2.abs()
    f = rstd * (torch.ones_like(gamma) if cot else gamma).abs()
    sgn = torch.ones_like(gamma) if cot else gamma
    r = rstd * sgn * (z - m1 - xh * m2)
    A = f * (za + m1.abs() + xha * m2.abs())
    if cot and c["base"]:
        r = r + inp["base"]
        A = A + inp["base"].abs()
    tau = f * (t1 + xh.abs() * t2) + tol(8, A)
    return dict(out=(r, tau)), dict(A=A)


def _geglu_parts(kind, a, fp, n4):
    """the expression of geglu_kernel<kind> on in = a, fprim = fp (any dtype)"""
    if kind == 0:
        return [a[:, :n4] * co._gelu(a[:, n4:])]
    v, g = fp[:n4].unsqueeze(0), fp[n4:].unsqueeze(0)
    if kind == 1:
        return [a[:, :n4] * co._gelu(g) + v * co._dgelu(g) * a[:, n4:]]
    return [torch.cat([a * co._gelu(g), a * v * co._dgelu(g)], 1)]


def _geglu_ref(c, inp):
    """kind 0: value gelu(gate), 6 roundings (the argument of erf, erf twice, 1 + erf, 0.5 gate, the products); kind 1: two such products
    and their sum, 12; kind 2: 6 and 8.  A: every factor by its absolute value, 1 + erf as 1 + |erf|, gelu' as 0.5 (1 + |erf|) + |g| phi(g)
    -- it does not vanish in the left tail, where 1 + erff cancels to 0 in fp32.  e: the float32-torch error of the expression."""
    kind, n4 = c["kind"], c["n4"]
    f = inp["f"]
    fp = f[0]
    a = {0: f, 1: inp["df"], 2: inp["g"]}[kind]
    ref = _geglu_parts(kind, a, fp, n4)[0]
    v, g = fp[:n4].unsqueeze(0), fp[n4:].unsqueeze(0)
    if kind == 0:
        A = f[:, :n4].abs() * gelu_abs(f[:, n4:])
    elif kind == 1:
        A = a[:, :n4].abs() * gelu_abs(g) + v.abs() * dgelu_abs(g) * a[:, n4:].abs()
    else:
        A = torch.cat([a.abs() * gelu_abs(g), a.abs() * v.abs() * dgelu_abs(g)], 1)
    e = e_term(lambda a_, fp_: _geglu_parts(kind, a_, fp_, n4)[0], (a, fp), A)
    return dict(out=(ref, tol({0: 6, 1: 12, 2: 8}[kind], A, e))), dict(A=A, e=e)


def temb_angle(t, freq):
    """the kernel's angle: the fp32 product float32(t) * freq[i], rounded ONCE (both factors are fp32, so their float64 product is
    exact and its rounding to fp32 is the fp32 product)"""
    return _f32(float(torch.tensor(t, dtype=F)) * freq)


def _temb_emb(c, angle):
    ch, half = c["ch"], c["ch"] // 2
    s, co_ = torch.sin(angle), torch.cos(angle)
    emb = torch.zeros(ch, dtype=angle.dtype)
    emb[:2 * half] = torch.cat([co_, s]) if c["cos_first"] else torch.cat([s, co_])
    return emb


def _act_bound(pre, t_pre, act):
    """act(pre) where pre carries t_pre: the slope bound times t_pre, plus 4 roundings and the fp32 activation's error e at
    |f| + |f'| |pre|"""
    A = act_abs(pre, act)
    e = e_term(lambda y: act_f(y, act), (pre,), A)
    return LIP[act] * t_pre + tol(4, A, e), A


def _temb_ref(c, inp):
    """emb = sin / cos of the fp32 angle: 2 u absolute (sinf, cosf), + 1 rounding of emb + add_in.  dense0: ch + 8 roundings of
    A = |b0| + |w0| |emb|, and |w0| t_emb.  act: _act_bound.  dense1 (+ add): temb_ch + 9 of A = |b1| + |w1| |h| + |add|, and |w1| t_h."""
    act, ch, tch = c["act"], c["ch"], c["tch"]
    emb = _temb_emb(c, temb_angle(c["t"], inp["freq"]))
    t_emb = tol(2, torch.ones(ch, dtype=D))
    if ch & 1:
        t_emb[ch - 1] = 0.0
    if c["add_in"]:
        t_emb = t_emb + tol(1, emb.abs() + inp["add_in"].abs())
        emb = emb + inp["add_in"]
    w0, w1 = inp["w0"], inp["w1"]
    pre0 = inp["b0"] + w0 @ emb
    t0 = tol(ch + 8, inp["b0"].abs() + w0.abs() @ emb.abs()) + w0.abs() @ t_emb
    h = act_f(pre0, act)
    t_h, _ = _act_bound(pre0, t0, act)
    pre1 = inp["b1"] + w1 @ h
    A1 = inp["b1"].abs() + w1.abs() @ h.abs()
    if c["add"]:
        pre1 = pre1 + inp["add"]
        A1 = A1 + inp["add"].abs()
    t1 = tol(tch + 9, A1) + w1.abs() @ t_h
    t_out, A = _act_bound(pre1, t1, act)
    return dict(out=(act_f(pre1, act), t_out)), dict(A=A, emb=(emb, t_emb))


def _temb_proj_ref(c, inp, tact):
    w = inp["pw"]
    ref = w @ tact
    A = w.abs() @ tact.abs()
    if c["bias"]:
        ref, A = ref + inp["pb"], A + inp["pb"].abs()
    return dict(out=(ref, tol(c["tch"] + 8, A))), dict(A=A)


def pool_f(x, scale):
    return ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + (x[..., 1::2, 0::2] + x[..., 1::2, 1::2])) * scale


def up_f(y, scale):
    return scale * y.repeat_interleave(2, -2).repeat_interleave(2, -1)


def _resample_ref(c, inp):
    """pool: three sums, the scale, the accumulate: 5 roundings of A = |scale| sum |x| + |out0|.  upsample: 2 of |scale x| + |out0|."""
    s = float(torch.tensor(c["scale"], dtype=F))
    pool = c["op"] == "pool2x2_sum"
    if pool:
        ref, A = pool_f(inp["x"], s), pool_f(inp["x"].abs(), abs(s))
        o0 = inp["small0"]
    else:
        ref, A = up_f(inp["y"], s), up_f(inp["y"].abs(), abs(s))
        o0 = inp["large0"]
    if c["acc"]:
        ref, A = ref + o0, A + o0.abs()
    bits = (not pool) and (c["scale"] == 1.0 or (c["scale"] == 0.25 and not c["acc"]))
    return dict(out=(ref, tol(5 if pool else 2, A))), dict(A=A, bits=["out"] if bits else [])


def _mask_ref(c, inp):
    cv, ce, ps = inp["cv"], inp["ce"], inp["pass"]
    zero = torch.zeros_like(inp["dE"])
    if c["op"] == "masked_axpby":
        v = zero if c["null"] else cv * inp["V"]
        ref = torch.where(ps, v + ce * inp["dE"], zero)
        A = torch.where(ps, v.abs() + (ce * inp["dE"]).abs(), zero)
        return dict(out=(ref, tol(3, A))), dict(A=A, zero=~ps)
    u = torch.where(ps, inp["U"], zero)
    o = dict(out=(ce * u, tol(1, (ce * u).abs())))
    if not c["null"]:
        o["out2"] = (cv * u, tol(1, (cv * u).abs()))
    return o, dict(A=u.abs(), zero=~ps)


def _step_ref(c, inp):
    op = c["op"]
    if op == "ddim_step":
        # P = (x - e c_x0_e) / c_x0_x: 4 roundings of (|x| + |e c_x0_e|) / |c_x0_x|; next = c_next_x0 P + c_next_e e (+ c_noise noise):
        # the bound of P at |c_next_x0| and 5 roundings of the absolute form
        cx, cxe, cn0, cne, cnz = inp["f"]
        x, e = inp["x"], inp["e"]
        p = (x - e * cxe) / cx
        Ap = (x.abs() + (e * cxe).abs()) / abs(cx)
        v, Av = cn0 * p + cne * e, abs(cn0) * Ap + (cne * e).abs()
        if c["noise"]:
            v, Av = v + cnz * inp["noise"], Av + (cnz * inp["noise"]).abs()
        o = dict(out=(v, abs(cn0) * tol(4, Ap) + tol(5, Av)))
        if c["x0"]:
            o["out2"] = (p, tol(4, Ap))
        return o, dict(A=Av)
    if op == "latent_sample":
        # z = scale (mean + exp(0.5 clamp(logvar, -30, 20)) noise): 6 roundings (expf twice) and the float32-torch error of the expression
        n, s = c["n"], inp["scale"]
        fn = lambda mom, nz: s * (mom[:, :n] + torch.exp(0.5 * mom[:, n:].clamp(-30.0, 20.0)) * nz)
        nz = inp["noise"] if c["noise"] else torch.zeros_like(inp["noise"])
        mom = inp["mom"]
        A = abs(s) * (mom[:, :n].abs() + torch.exp(0.5 * mom[:, n:].clamp(-30.0, 20.0)) * nz.abs())
        return dict(out=(fn(mom, nz), tol(6, A, e_term(fn, (mom, nz), A)))), dict(A=A)
    if op == "lincomb":
        src = list(inp["src"])
        ref = sum(cf * s for cf, s in zip(inp["coef"], src))
        A = sum((cf * s).abs() for cf, s in zip(inp["coef"], src))
        return dict(out=(ref, tol(c["nsrc"] + 8, A))), dict(A=A)
    if op == "copy":
        ref, A = inp["x"], inp["x"].abs()
        if c["acc"]:
            ref, A = ref + inp["out0"], A + inp["out0"].abs()
        return dict(out=(ref, tol(1, A))), dict(A=A, bits=[] if c["acc"] else ["out"])
    assert op == "add"
    return dict(out=(inp["a"] + inp["b"], tol(1, inp["a"].abs() + inp["b"].abs()))), dict(A=inp["a"].abs() + inp["b"].abs())


def reference(c, inp, tact=None):
    """({output: (ref, tau)}, info): info["A"] the scale of the main output, info["bits"] outputs that must be float32(ref) bit for
    bit, info["zero"] the elements that must be exact zeros.  tact: temb_proj's input, the fp32 output of the temb launch before it"""
    op = c["op"]
    if op == "ln_fwd":
        return _ln_fwd_ref(c, inp)
    if op in ("ln_tan", "ln_cot"):
        return _ln_lin_ref(c, inp)
    if op == "geglu":
        return _geglu_ref(c, inp)
    if op == "temb":
        return _temb_ref(c, inp)
    if op == "temb_proj":
        return _temb_proj_ref(c, inp, tact)
    if op in ("pool2x2_sum", "upsample2x"):
        return _resample_ref(c, inp)
    if op in ("masked_axpby", "cot_seed"):
        return _mask_ref(c, inp)
    return _step_ref(c, inp)


def adjoint_io(c, inp):
    """the input tensor of a case that takes part in an adjoint identity"""
    op = c["op"]
    if op == "geglu":
        return inp["df"] if c["kind"] == 1 else inp["g"]
    return inp[{"ln_tan": "d", "ln_cot": "g", "pool2x2_sum": "x", "upsample2x": "y"}[op]]


def adjoint(in_a, out_a, tau_a, in_b, out_b, tau_b):
    """<out_a, in_b> = <in_a, out_b> in float64: (|lhs - rhs|, bound = sum |in_b| tau_a + sum |in_a| tau_b)"""
    lhs = float((out_a.to(D) * in_b).sum())
    rhs = float((in_a * out_b.to(D)).sum())
    return abs(lhs - rhs), float((in_b.abs() * tau_a).sum() + (in_a.abs() * tau_b).sum())


def worst(got, ref, tau, name):
    """(share, message): max |got - ref| / tau over EVERY element, NaN and Inf counting as a failure; the message names the worst element"""
    got = got.to(D).reshape(ref.shape)
    err = (got - ref).abs()
    ratio = err / tau
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    share = float(ratio.max())
    return share, (f"worst element {name}{list(idx)}: got {float(got[idx])!r} ref {float(ref[idx])!r} |err| = {float(err[idx]):.3e} against tau = "
                   f"{float(tau[idx]):.3e} ({share:.3f} of tau); {int((ratio > 1).sum())} of {ratio.numel()} fail")


def check(outs, refs, info):
    """outs {name: fp32 tensor} against reference()'s result -> dict(share, msg, unwritten, bits_bad, zero_bad, shares {name: share})"""
    shares, msgs, unwritten, bits_bad, zero_bad = {}, [], 0, 0, 0
    for name, (ref, tau) in refs.items():
        got = outs[name].reshape(ref.shape)
        unwritten += int(torch.isnan(got).sum())
        shares[name], m = worst(got, ref, tau, name)
        msgs.append(m)
        if name in info.get("bits", ()):
            bits_bad += int((got.to(F).contiguous().view(torch.int32) != ref.to(F).contiguous().view(torch.int32)).sum())
        if "zero" in info:
            zero_bad += int((got[info["zero"]] != 0).sum())
    top = max(shares, key=shares.get)
    return dict(share=shares[top], msg=msgs[list(refs).index(top)], unwritten=unwritten, bits_bad=bits_bad, zero_bad=zero_bad, shares=shares)


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 restatements in the kernels' own order of operations (torch float32 on the CPU).  plant: an error of
# tests/test_token_oracle_host.py; a plant that does not apply to the case raises KeyError there, not here.

def _gelu_tanh(y):
    return 0.5 * y * (1 + torch.tanh(0.7978845608028654 * (y + 0.044715 * y ** 3)))


def _quick_gelu(y):
    return y * torch.sigmoid(1.702 * y)


def restate32(c, inp, plant=None, tact=None) -> Dict[str, torch.Tensor]:
    op = c["op"]
    f = lambda t: t.to(F)
    if op == "ln_fwd":
        x, gamma, beta, C = f(inp["x"]), f(inp["gamma"]).view(1, -1, 1), f(inp["beta"]).view(1, -1, 1), c["C"]
        mean = x.sum(1, keepdim=True, dtype=F) / (C - 1 if plant == "mean_over_c_minus_1" else C)
        d = x - mean
        var = (d * d).sum(1, keepdim=True, dtype=F) / C
        rstd = 1.0 / (torch.sqrt(var) + c["eps"]) if plant == "eps_outside_sqrt" else torch.rsqrt(var + c["eps"])
        y = d * rstd * gamma + beta
        if plant == "sample_slot":
            y[0] = y[1]
        return dict(y=y, stats=torch.cat([mean, var if plant == "rstd_as_variance" else rstd], 1))
    if op in ("ln_tan", "ln_cot"):
        cot = op == "ln_cot"
        x, gamma, sp = f(inp["prim"]).unsqueeze(0), f(inp["gamma"]).view(1, -1, 1), f(inp["sprim"])
        if plant == "neighbour_stats":
            sp = torch.roll(sp, 1, dims=1)
        mean, rstd = sp[0].view(1, 1, -1), sp[1].view(1, 1, -1)
        d = f(inp["g"] if cot else inp["d"])
        late = cot and plant == "gamma_after_means"
        z = gamma * d if cot and not late else d
        xh = (x - mean) * rstd
        m1 = z.sum(1, keepdim=True, dtype=F) / c["C"]
        m2 = (xh * z).sum(1, keepdim=True, dtype=F) / c["C"]
        if plant == "no_xhat_m2":
            m2 = torch.zeros_like(m2)
        fac = gamma if (late or (not cot and plant != "tangent_no_gamma")) else torch.ones_like(gamma)
        r = rstd * fac * (z - m1 - xh * m2)
        if cot and c["base"] and plant != "base_ignored":
            r = r + f(inp["base"])
        if plant == "sample_slot":
            r[0] = r[1]
        return dict(out=r)
    if op == "geglu":
        kind, n4 = c["kind"], c["n4"]
        fp = f(inp["f"][0])
        a = f({0: inp["f"], 1: inp["df"], 2: inp["g"]}[kind])
        if plant == "halves_swapped":
            fp = torch.cat([fp[n4:], fp[:n4]])
            a = torch.cat([a[:, n4:], a[:, :n4]], 1) if kind == 0 else a
        gl = {"gelu_tanh": _gelu_tanh, "quick_gelu": _quick_gelu}.get(plant, co._gelu)
        if kind == 0:
            return dict(out=a[:, :n4] * gl(a[:, n4:]))
        v, g = fp[:n4].unsqueeze(0), fp[n4:].unsqueeze(0)
        if kind == 1:
            second = torch.zeros_like(a[:, :n4]) if plant == "no_dgate_term" else v * co._dgelu(g) * a[:, n4:]
            return dict(out=a[:, :n4] * gl(g) + second)
        return dict(out=torch.cat([a * gl(g), torch.zeros_like(a) if plant == "no_dgate_term" else a * v * co._dgelu(g)], 1))
    if op == "temb":
        act = c["act"]
        t32 = torch.tensor(c["t"], dtype=F)
        angle = t32 * f(inp["freq"])
        cc = dict(c, cos_first=1 - c["cos_first"]) if plant == "sin_cos_swapped" else c
        if plant == "angle_not_rounded":      # sin / cos of the exact product: a reference convention, not the kernel's
            emb = f(_temb_emb(cc, float(t32) * inp["freq"]))
        else:
            emb = _temb_emb(cc, angle)
        if c["add_in"]:
            emb = emb + f(inp["add_in"])
        h = act_f(f(inp["b0"]) + f(inp["w0"]) @ emb, act)
        pre = f(inp["b1"]) + f(inp["w1"]) @ h
        if c["add"] and plant != "add_after_act":
            pre = pre + f(inp["add"])
        out = act_f(pre, act)
        if c["add"] and plant == "add_after_act":
            out = out + f(inp["add"])
        return dict(out=out, _emb=emb)      # _emb: the embedding behind dense0, not an output of the launch (the angle convention's check)
    if op == "temb_proj":
        out = f(inp["pw"]) @ f(tact)
        return dict(out=out + f(inp["pb"]) if c["bias"] else out)
    if op in ("pool2x2_sum", "upsample2x"):
        s = torch.tensor(c["scale"], dtype=F)
        pool = op == "pool2x2_sum"
        x = f(inp["x"] if pool else inp["y"])
        if plant == "hw_swapped":
            B, C, H, W = x.shape
            x = x.reshape(B, C, W, H)
        r = pool_f(x, torch.tensor(1.0, dtype=F) if plant == "pool_no_scale" else s) if pool else up_f(x, s)
        if plant == "hw_swapped":
            r = r.reshape(r.shape[0], r.shape[1], r.shape[3], r.shape[2])
        if c["acc"] and plant != "accumulate_ignored":
            r = r + f(inp["small0"] if pool else inp["large0"])
        return dict(out=r)
    if op in ("masked_axpby", "cot_seed"):
        cv, ce = torch.tensor(inp["cv"], dtype=F), torch.tensor(inp["ce"], dtype=F)
        ps = inp["pass"]
        if plant == "mask2_from_split_plus_1":
            ps = pass_of(dict(c, split=c["split"] + 1), inp)
        zero = torch.zeros(ps.shape, dtype=F)
        if op == "masked_axpby":
            expr = (zero if c["null"] else cv * f(inp["V"])) + ce * f(inp["dE"])
            return dict(out=ps.to(F) * expr if plant == "mask_as_product" else torch.where(ps, expr, zero))
        u = ps.to(F) * f(inp["U"]) if plant == "mask_as_product" else torch.where(ps, f(inp["U"]), zero)
        o = dict(out=ce * u)
        if not c["null"]:
            o["out2"] = cv * u
        return o
    if op == "ddim_step":
        cx, cxe, cn0, cne, cnz = (torch.tensor(v, dtype=F) for v in inp["f"])
        x, e = f(inp["x"]), f(inp["e"])
        p = (x - e * cxe) / cx
        v = cn0 * p + cne * e
        if c["noise"]:
            v = v + cnz * f(inp["noise"])
        o = dict(out=v)
        if c["x0"]:
            o["out2"] = p
        return o
    if op == "latent_sample":
        n, mom = c["n"], f(inp["mom"])
        nz = f(inp["noise"]) if c["noise"] else torch.zeros(mom.shape[0], n, dtype=F)
        return dict(out=torch.tensor(inp["scale"], dtype=F) * (mom[:, :n] + torch.exp(0.5 * mom[:, n:].clamp(-30.0, 20.0)) * nz))
    if op == "lincomb":
        acc = torch.zeros(c["n"], dtype=F)
        for cf, s in zip(inp["coef"], inp["src"]):
            acc = torch.tensor(cf, dtype=F) * f(s) + acc
        if plant == "tail_dropped":
            acc[c["n"] - c["n"] % 4:] = float("nan")
        return dict(out=acc)
    if op == "copy":
        return dict(out=f(inp["x"]) + f(inp["out0"]) if c["acc"] else f(inp["x"]))
    assert op == "add"
    return dict(out=f(inp["a"]) + f(inp["b"]))
