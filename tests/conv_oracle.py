"""Float64 reference of ONE conv launch (loco_debug_conv, include/loco_hip_diag.h), its componentwise error scale, the error
a number format alone causes, the operands and the case table of tests/test_gpu_conv_oracle.py.

A case `d` is a plain dict of the descriptor fields (taps, Cin, Cout, H, W, B, mode, stride, upsample, zins, transposed, pad,
cpg, accumulate, res_scale, in_arena, Cin2) plus flags saying which optional operands exist (bias, bias2, res, cot); `ops` is
a dict of float64 CPU tensors whose values are exactly representable in float32 (what the kernel receives).

    reference(d, ops)      the launch as kernels.h specifies it (ConvMode, the cot_d comment of ConvArgs), in float64
    magnitude(d, ops)      the same expression with every operand and every term replaced by its absolute value: A
    emulated(d, ops, p)    the same expression with the two matrix operands rounded as precision p defines them
    tolerance(d, ops, p)   tau of the check |out - ref| <= tau A + 1e-30, from the reference alone (see below)

tau = MARGIN * (format + accumulation + prologue):
  format        max |emulated - reference| / A over the case's outputs (0 for f32)
  accumulation  (K + 8) 2^-24, K = Cin taps + Cin2: an fp32 sum of K terms (+ the epilogue's handful)
  prologue      max |a32 - a64| / a_abs of the mode's prologue evaluated in float32 torch on the CPU, where a_abs is the prologue
                with every term replaced by its absolute value (prologue(absolute=True)) -- the prologue A is built from.
                (Relative to |a64| itself the figure is unbounded: sc x + sh, d - m1 - xhat m2 and silu'(y) cross zero, and
                over 10^5 elements some a64 is 10^-6 of its terms: a tau of 0.2 came out of that reading, under which every
                planted error passes.  a_abs >= |a64|, so this reading only tightens tau.)
  MARGIN = 4    the emulation rounds to nearest where hardware may truncate or split differently (x2), and the order of the
                accumulation varies (x2)
"""
from __future__ import annotations

import math
from typing import Dict, List

import torch
import torch.nn.functional as F

MARGIN = 4.0
EPS_ABS = 1e-30
GN_EPS = 1e-6
PRECISIONS = {"f32": 0, "bf16x3": 1, "f16": 2}
CM_NONE, CM_GN_SILU, CM_GN, CM_TAN_SILU, CM_COT_SILU, CM_GN_GELU = range(6)


# ---------------------------------------------------------------------------------------------------------------------------
# geometry

def case(taps, Cin, Cout, H, W=None, B=1, mode=0, **kw) -> dict:
    d = dict(taps=taps, Cin=Cin, Cout=Cout, H=H, W=W if W is not None else H, B=B, mode=mode, stride=1, upsample=0, zins=0,
             transposed=0, pad=-1, accumulate=0, res_scale=1.0, in_arena=1, Cin2=0, bias=True, bias2=False, res=False,
             cot=False, cpg=0)
    d.update(kw)
    if d["mode"] in (CM_TAN_SILU, CM_COT_SILU) and not d["cpg"]:
        d["cpg"] = max(1, d["Cin"] // 8)
    if d["cot"]:
        d.setdefault("cot_cpg", max(1, d["Cout"] // 8))
    return d


def out_hw(d):
    if d["stride"] == 2:
        return d["H"] // 2, d["W"] // 2
    if d["upsample"] or d["zins"]:
        return 2 * d["H"], 2 * d["W"]
    return d["H"], d["W"]


def pad_of(d):
    if d["pad"] >= 0:
        return d["pad"]
    return 0 if d["taps"] == 1 else 2 if d["zins"] else 0 if d["stride"] == 2 else 1


def case_id(d) -> str:
    ho, wo = out_hw(d)
    s = f"{'3x3' if d['taps'] == 9 else '1x1'}_{d['Cin']}to{d['Cout']}_{d['H']}x{d['W']}_B{d['B']}_m{d['mode']}"
    for k, t in (("stride", "s2"), ("upsample", "up"), ("zins", "zins"), ("transposed", "T"), ("accumulate", "acc")):
        if d[k] not in (0, 1) or (d[k] == 1 and k != "stride"):
            s += "_" + t
    if d["Cin2"]:
        s += f"_kcat{d['Cin2']}"
    for k in ("bias2", "res", "cot"):
        if d[k]:
            s += "_" + k
    if not d["bias"]:
        s += "_nobias"
    if d["res_scale"] != 1.0:
        s += "_rs"
    if not d["in_arena"]:
        s += "_user"
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# the expression

def _silu(y):
    return y * torch.sigmoid(y)


def _dsilu(y):
    sg = torch.sigmoid(y)
    return sg * (1 + y * (1 - sg))


def _gelu(y):
    return 0.5 * y * (1 + torch.erf(y * 0.7071067811865476))


def _per_channel(v, cpg):
    """[..., G] -> [..., C] (a group value repeated over its channels)"""
    return torch.repeat_interleave(v, cpg, dim=-1)


def _d2silu(y):
    sg = torch.sigmoid(y)
    return sg * (1 - sg) * (2 + y * (1 - 2 * sg))


def _dgelu(y):
    return 0.5 * (1 + torch.erf(y * 0.7071067811865476)) + y * 0.3989422804014327 * torch.exp(-0.5 * y * y)


def prologue(d, ops, dtype=torch.float64, absolute=False):
    """a(mode) of kernels.h ConvMode on [B][Cin][H][W].

    absolute: the same expression with every term replaced by its absolute value, down to the affine y = sc x + sh inside the
    activation and the difference x - mean inside xhat: f(y) counts as |f(y)| + |f'(y)| (|sc x| + |sh|), the first-order size of
    f over the terms of y -- without it the scale vanishes where silu'(y) or y crosses zero while the fp32 value of y does not
    get any more exact there."""
    x = ops["in"].to(dtype)
    mode = d["mode"]
    if mode == CM_NONE:
        return x.abs() if absolute else x
    sc = ops["sc"].to(dtype).view(1, -1, 1, 1)
    sh = ops["sh"].to(dtype).view(1, -1, 1, 1)
    if mode in (CM_GN_SILU, CM_GN, CM_GN_GELU):
        y = sc * x + sh
        f, df = {CM_GN: (lambda t: t, torch.ones_like), CM_GN_SILU: (_silu, _dsilu), CM_GN_GELU: (_gelu, _dgelu)}[mode]
        if absolute:
            ya = (sc * x).abs() + sh.abs()
            fa = f(y).abs() if mode != CM_GN_GELU else 0.5 * y.abs() * (1 + torch.erf(y * 0.7071067811865476).abs())      # (1 + erf cancels)
            return ya if mode == CM_GN else fa + df(y).abs() * ya
        return f(y)
    cpg = d["cpg"]
    p = ops["prim"].to(dtype).unsqueeze(0)
    mr = ops["mr"].to(dtype)
    mean = _per_channel(mr[:, 0], cpg).view(1, -1, 1, 1)
    rstd = _per_channel(mr[:, 1], cpg).view(1, -1, 1, 1)
    tst = ops["tst"].to(dtype)
    m1 = _per_channel(tst[:, :, 0], cpg).view(x.shape[0], -1, 1, 1)
    m2 = _per_channel(tst[:, :, 1], cpg).view(x.shape[0], -1, 1, 1)
    y = sc * p + sh
    ds = _dsilu(y)
    xh = (p - mean) * rstd
    if absolute:
        ds = ds.abs() + _d2silu(y).abs() * ((sc * p).abs() + sh.abs())
        xh = (p.abs() + mean.abs()) * rstd.abs()
    if mode == CM_TAN_SILU:
        if absolute:
            return ds * sc.abs() * (x.abs() + m1.abs() + xh * m2.abs())
        return ds * sc * (x - m1 - xh * m2)
    gamma = ops["gamma"].to(dtype).view(1, -1, 1, 1)
    if absolute:
        return rstd.abs() * (gamma.abs() * ds * x.abs() + m1.abs() + xh * m2.abs())
    return rstd * (gamma * ds * x - m1 - xh * m2)


def _resample(d, a):
    if d["upsample"]:
        return F.interpolate(a, scale_factor=2, mode="nearest")
    if d["zins"]:
        z = a.new_zeros(a.shape[0], a.shape[1], 2 * a.shape[2], 2 * a.shape[3])
        z[:, :, ::2, ::2] = a
        return z
    return a


def _product(d, a, w):
    """the launch's matrix product: `a` already resampled, `w` the module's weight (see loco_conv_desc)"""
    k = 3 if d["taps"] == 9 else 1
    p = pad_of(d)
    q = k - 1 - p                       # zeros behind the map (bottom / right)
    ho, wo = out_hw(d)
    a = F.pad(a, (p, q, p, q)) if q >= 0 else F.pad(a, (p, 0, p, 0))
    if d["transposed"]:                 # flipped taps, channels swapped: the correlation form of conv_transpose2d
        w = w.flip(2, 3).transpose(0, 1)
    o = F.conv2d(a, w, stride=d["stride"])
    return o[:, :, :ho, :wo]


def _expr(d, ops, a, w, in2, w2, absolute):
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    out = _product(d, _resample(d, a), w)
    B = out.shape[0]
    if "bias" in ops:
        out = out + ab(ops["bias"]).view(1, -1, 1, 1)
    if "bias2" in ops:
        out = out + ab(ops["bias2"]).view(B, -1, 1, 1)
    if "res" in ops:
        out = out + ab(d["res_scale"] * ops["res"])
    if d["Cin2"]:
        out = out + F.conv2d(in2, w2)
        if "bias2nd" in ops:
            out = out + ab(ops["bias2nd"]).view(1, -1, 1, 1)
    if "cot_d" in ops:
        cpg = d["cot_cpg"]
        x = ops["cot_prim"].unsqueeze(0)
        sc = ops["cot_sc"].view(1, -1, 1, 1)
        sh = ops["cot_sh"].view(1, -1, 1, 1)
        mean = _per_channel(ops["cot_mr"][:, 0], cpg).view(1, -1, 1, 1)
        rstd = _per_channel(ops["cot_mr"][:, 1], cpg).view(1, -1, 1, 1)
        S = sc * _dsilu(sc * x + sh)
        xh = (x - mean) * rstd
        m1 = ops["cot_tc"][:, :, 0].view(B, -1, 1, 1)
        m2 = ops["cot_tc"][:, :, 1].view(B, -1, 1, 1)
        if absolute:
            out = out + S.abs() * ops["cot_d"].abs() + (rstd * m1).abs() + (xh * rstd * m2).abs()
        else:
            out = out + S * ops["cot_d"] - (rstd * m1 + xh * rstd * m2)
    if d["accumulate"]:
        out = out + ab(ops["out0"])
    return out


def reference(d, ops):
    return _expr(d, ops, prologue(d, ops), ops["weight"], ops.get("in2"), ops.get("w2"), False)


def magnitude(d, ops):
    in2 = ops["in2"].abs() if d["Cin2"] else None
    w2 = ops["w2"].abs() if d["Cin2"] else None
    return _expr(d, ops, prologue(d, ops, absolute=True), ops["weight"].abs(), in2, w2, True)


def _bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _split(t):
    """(hi, lo) bf16 pieces of the float32 value of t, as float64"""
    t32 = t.to(torch.float32).to(torch.float64)
    hi = _bf16(t32)
    return hi, _bf16(t32 - hi)


def emulated(d, ops, prec):
    """reference() with the matrix operands (prologue output and weights, of both operators) in the number format of `prec`"""
    a = prologue(d, ops)
    if prec == "f32":
        return _expr(d, ops, a, ops["weight"], ops.get("in2"), ops.get("w2"), False)
    if prec == "f16":
        r = lambda t: t.to(torch.float32).to(torch.float16).to(torch.float64)
        return _expr(d, ops, r(a), r(ops["weight"]), r(ops["in2"]) if d["Cin2"] else None, r(ops["w2"]) if d["Cin2"] else None, False)
    assert prec == "bf16x3"
    # hi hi + hi lo + lo hi = (hi + lo)(hi + lo) - lo lo: the full expression on the summed pieces minus the dropped products
    ah, al = _split(a)
    wh, wl = _split(ops["weight"])
    full = _expr(d, ops, ah + al, wh + wl, *(((lambda p, q: (p[0] + p[1], q[0] + q[1]))(_split(ops["in2"]), _split(ops["w2"])))
                                            if d["Cin2"] else (None, None)), False)
    drop = _product(d, _resample(d, al), wl)
    if d["Cin2"]:
        drop = drop + F.conv2d(_split(ops["in2"])[1], _split(ops["w2"])[1])
    return full - drop


def prologue_term(d, ops) -> float:
    if d["mode"] == CM_NONE:
        return 0.0
    a64 = prologue(d, ops)
    a32 = prologue(d, ops, dtype=torch.float32).to(torch.float64)
    return float(((a32 - a64).abs() / prologue(d, ops, absolute=True).clamp_min(1e-300)).max())


def tolerance(d, ops, prec, ref=None, A=None) -> Dict[str, float]:
    ref = reference(d, ops) if ref is None else ref
    A = magnitude(d, ops) if A is None else A
    fmt = 0.0 if prec == "f32" else float(((emulated(d, ops, prec) - ref).abs() / A).max())
    acc = (d["Cin"] * d["taps"] + d["Cin2"] + 8) * 2.0 ** -24
    pro = prologue_term(d, ops)
    return dict(format=fmt, accumulation=acc, prologue=pro, tau=MARGIN * (fmt + acc + pro))


def worst(out, ref, A, tau):
    """(ok, message): the check |out - ref| <= tau A + EPS_ABS on every element, NaN counting as a failure; the message names the
    worst element's (b, cout, y, x)"""
    err = (out.to(torch.float64) - ref).abs()
    ratio = err / (tau * A + EPS_ABS)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    b, c, y, x = reversed(idx)
    bad = int((ratio > 1).sum())
    msg = (f"worst element (b, cout, y, x) = ({b}, {c}, {y}, {x}): out {float(out[b, c, y, x])!r} ref {float(ref[b, c, y, x])!r} "
           f"|err| / A = {float(err[b, c, y, x] / A[b, c, y, x]):.3e} against tau = {tau:.3e}; {bad} of {ratio.numel()} elements fail")
    return bad == 0, msg


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def _f32(t):
    return t.to(torch.float32).to(torch.float64)


def _norm_arrays(x, cpg, g):
    """float64 GroupNorm statistics of x [C][H][W] and a drawn affine -> sc, sh, mr [G][2], gamma (rounded to float32)"""
    C = x.shape[0]
    G = C // cpg
    xg = x.reshape(G, -1)
    mean = xg.mean(1)
    rstd = 1.0 / torch.sqrt(xg.var(1, unbiased=False) + GN_EPS)
    gamma = _f32(1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64))
    beta = _f32(0.3 * torch.randn(C, generator=g, dtype=torch.float64))
    mr = _f32(torch.stack([mean, rstd], 1))
    rs = _per_channel(mr[:, 1], cpg)
    sc = _f32(gamma * rs)
    sh = _f32(beta - _per_channel(mr[:, 0], cpg) * rs * gamma)
    return sc, sh, mr, gamma


def make_operands(d, seed=0) -> Dict[str, torch.Tensor]:
    """Seeded operands at the scale of real activations: unit-variance maps with a per-channel offset of a few units, weights of
    1 / sqrt(K), statistics arrays from the actual float64 statistics of the primal they describe."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * d["Cin"] + 31 * d["Cout"] + d["H"] + 3 * d["mode"] + d["B"])
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, Cin, Cout, H, W = d["B"], d["Cin"], d["Cout"], d["H"], d["W"]
    ho, wo = out_hw(d)
    k = 3 if d["taps"] == 9 else 1
    ops = {}
    off = lambda C: 3.0 * rn(C).view(-1, 1, 1)
    ops["in"] = _f32(rn(B, Cin, H, W) * (0.5 + torch.rand(Cin, generator=g, dtype=torch.float64)).view(1, -1, 1, 1) + off(Cin))
    wshape = (Cin, Cout, k, k) if d["transposed"] else (Cout, Cin, k, k)
    ops["weight"] = _f32(rn(*wshape) / math.sqrt(Cin * k * k))
    if d["bias"]:
        ops["bias"] = _f32(0.5 * rn(Cout) + 0.25)
    if d["bias2"]:
        ops["bias2"] = _f32(0.5 * rn(B, Cout))
    if d["res"]:
        ops["res"] = _f32(rn(B, Cout, ho, wo) + off(Cout))
    if d["accumulate"]:
        ops["out0"] = _f32(rn(B, Cout, ho, wo) + off(Cout))
    mode = d["mode"]
    if mode in (CM_GN_SILU, CM_GN, CM_GN_GELU):
        cpg = d["cpg"] or max(1, Cin // 8)
        ops["sc"], ops["sh"], _, _ = _norm_arrays(ops["in"][0], cpg, g)
    elif mode in (CM_TAN_SILU, CM_COT_SILU):
        cpg = d["cpg"]
        G = Cin // cpg
        prim = _f32(rn(Cin, H, W) * (0.5 + torch.rand(Cin, generator=g, dtype=torch.float64)).view(-1, 1, 1) + off(Cin))
        sc, sh, mr, gamma = _norm_arrays(prim, cpg, g)
        ops.update(prim=prim, sc=sc, sh=sh, mr=mr, gamma=gamma)
        xh = (prim - _per_channel(mr[:, 0], cpg).view(-1, 1, 1)) * _per_channel(mr[:, 1], cpg).view(-1, 1, 1)
        z = ops["in"]
        if mode == CM_COT_SILU:
            z = (gamma.view(-1, 1, 1) * _dsilu(sc.view(-1, 1, 1) * prim + sh.view(-1, 1, 1))).unsqueeze(0) * z
        m1 = z.reshape(B, G, -1).mean(2)
        m2 = (z * xh.unsqueeze(0)).reshape(B, G, -1).mean(2)
        ops["tst"] = _f32(torch.stack([m1, m2], 2))
        ops["tc"] = torch.repeat_interleave(ops["tst"], cpg, dim=1).contiguous()
    if d["Cin2"]:
        C2 = d["Cin2"]
        ops["in2"] = _f32(rn(B, C2, ho, wo) + off(C2))
        ops["w2"] = _f32(rn(Cout, C2, 1, 1) / math.sqrt(C2))
        ops["bias2nd"] = _f32(0.5 * rn(Cout) - 0.25)
    if d["cot"]:
        cpg = d["cot_cpg"]
        G = Cout // cpg
        prim = _f32(rn(Cout, ho, wo) + off(Cout))
        sc, sh, mr, gamma = _norm_arrays(prim, cpg, g)
        dd = _f32(rn(B, Cout, ho, wo) + 0.5)
        xh = (prim - _per_channel(mr[:, 0], cpg).view(-1, 1, 1)) * _per_channel(mr[:, 1], cpg).view(-1, 1, 1)
        z = (gamma.view(-1, 1, 1) * _dsilu(sc.view(-1, 1, 1) * prim + sh.view(-1, 1, 1))).unsqueeze(0) * dd
        m1 = z.reshape(B, G, -1).mean(2)
        m2 = (z * xh.unsqueeze(0)).reshape(B, G, -1).mean(2)
        tc = torch.repeat_interleave(_f32(torch.stack([m1, m2], 2)), cpg, dim=1).contiguous()
        ops.update(cot_d=dd, cot_prim=prim, cot_sc=sc, cot_sh=sh, cot_mr=mr, cot_tc=tc)
    return ops


# ---------------------------------------------------------------------------------------------------------------------------
# the case table: (case, precisions, what the plan must say for each precision)
#
# `expect` keys, all about the MAIN operator's launches (a shortcut that ran first is listed apart):
#   kernel   substring of conv_variant_name of launch 0      tile     tile variant of launch 0
#   split    launch 0 has nsplit > 1                          gemm_tm  0: not the GEMM kernel, 2 / 4: its cout tile
#   pair     launch 0 runs the tap-pair kernel                kcat     launch 0 carries the shortcut (Cin2 > 0)
#   sc_first the shortcut ran as a launch of its own          cot      the norm-cotangent term rode in the epilogue
#   tail     number of probes of the split tail launch (0: one launch)

ROWS: List[dict] = []


def _row(family, d, precs, probes=None, refused=False, **expect):
    """one table row.  expect: `all` for every precision, `f32` / `bf16` / `f16` on top of it for one; probes: the samples whose
    reference is computed (None: all); refused: the planner routes the row as `expect` says, but no kernel can walk its map
    (see DESIGN.md): loco_debug_conv must refuse it"""
    per = {p: dict(expect.get("all", {}), **expect.get(p.replace("bf16x3", "bf16"), {})) for p in precs}
    ROWS.append(dict(family=family, case=d, precs=precs, expect=per, id=case_id(d), probes=probes, refused=refused))


def _build_table():
    LP = ("bf16x3",)
    LPH = ("bf16x3", "f16")
    ALL = ("f32", "bf16x3", "f16")
    f32k = dict(kernel="conv_mfma_f32", gemm_tm=0, pair=0, kcat=0)
    # exact-fp32 tiles 3 / 1 / 2 / 0
    for (ci, co, hw, tile) in ((32, 64, 8, 3), (32, 96, 8, 1), (32, 32, 16, 2), (32, 64, 16, 0)):
        for B in (1, 3):
            for mode in (0, 1, 3, 4):
                _row("f32 tiles", case(9, ci, co, hw, B=B, mode=mode), ("f32",), all=dict(f32k, tile=tile, split=False, tail=0))
    _row("f32 split-K", case(9, 256, 64, 8, B=1), ("f32",), all=dict(f32k, tile=3, split=True, tail=0))
    # low precision, 64 x 64 tile of the B = 1 chains
    for taps in (9, 1):
        for hw in (8, 32):
            _row("lowp tile 3", case(taps, 64, 64, hw, B=1), LP, all=dict(kernel="conv_mfma_bf16x3", tile=3, gemm_tm=0, pair=0, tail=0))
    _row("lowp tile 3", case(9, 64, 64, 32, B=1, mode=1), LP, all=dict(kernel="conv_mfma_bf16x3", tile=3, tail=0))
    # lock-step 128 x 256 tile; at B = 1 a 64-multiple of couts goes to tile 3 (conv_bf16_pick_tile), so B = 1 takes 96 couts
    t5 = dict(tile=5, split=False, pair=0, kcat=0, tail=0)
    t5b, t5h = dict(kernel="conv_mfma_bf16x3<9,2,4,2,2"), dict(kernel="conv_mfma_f16<9,2,4,2,2")
    for B in (2, 3):
        for mode in (0, 1, 3, 4):
            _row("lowp tile 5", case(9, 48, 64, 16, B=B, mode=mode), LPH, all=t5, bf16=t5b, f16=t5h)
    for mode in (0, 1, 3, 4):
        _row("lowp tile 5", case(9, 48, 96, 16, B=1, mode=mode), LPH, all=t5, bf16=t5b, f16=t5h)
    _row("lowp tile 5", case(9, 48, 64, 16, B=1, mode=3), LP, all=dict(tile=3, split=False, tail=0))
    _row("lowp tile 5", case(9, 48, 64, 16, B=2, mode=5), ALL, bf16=t5, f16=t5, f32=dict(f32k, tile=0))
    # ragged channels
    _row("ragged", case(9, 3, 64, 32, B=2, in_arena=0), ALL, bf16=dict(tile=5, split=False), f16=dict(tile=5), f32=dict(f32k, tile=0))
    _row("ragged", case(9, 3, 64, 32, B=1, in_arena=0, mode=0), ALL, bf16=dict(tile=3), f16=dict(tile=3), f32=dict(f32k, tile=0))
    _row("ragged", case(9, 4, 64, 16, B=2), ALL, bf16=dict(tile=5), f16=dict(tile=5), f32=dict(f32k, tile=0))
    for co in (3, 4, 6, 8):
        _row("ragged", case(9, 64, co, 32, B=2), ALL, bf16=dict(tile=2), f16=dict(tile=2), f32=dict(f32k, tile=2))
    _row("ragged", case(1, 40, 40, 16, B=2), ALL, bf16=dict(tile=0), f16=dict(tile=0), f32=dict(f32k, tile=0))
    # split-K + reduce (the reduce kernel applies the epilogue)
    sk = dict(split=True, tail=0, gemm_tm=0)
    for hw in (8, 16):
        for B in (1, 2):
            _row("lowp split-K", case(9, 512, 128, hw, B=B), ALL, all=sk)
    _row("lowp split-K", case(9, 512, 128, 8, B=2, bias=False), ALL, all=sk)
    _row("lowp split-K", case(9, 512, 128, 8, B=2, bias2=True), ALL, all=sk)
    _row("lowp split-K", case(9, 512, 128, 16, B=2, res=True), ALL, all=sk)
    _row("lowp split-K", case(9, 512, 128, 16, B=1, res=True, res_scale=0.7071067811865476), ALL, all=sk)
    _row("lowp split-K", case(9, 512, 128, 8, B=2, accumulate=1), ALL, all=sk)
    _row("lowp split-K", case(9, 512, 128, 16, B=2, mode=1), ALL, all=sk)
    # stride 2: the 128 x 128 tile where stride 1 would take 128 x 256 (B = 1 with a 64-multiple of couts: tile 3)
    _row("stride 2", case(9, 64, 64, 32, B=2, stride=2), ALL, bf16=dict(tile=0, split=False), f16=dict(tile=0), f32=dict(f32k, tile=0))
    _row("stride 2", case(9, 64, 96, 32, B=1, stride=2), ALL, bf16=dict(tile=0), f16=dict(tile=0), f32=dict(f32k, tile=0))
    _row("stride 2", case(9, 64, 64, 32, B=1, stride=2), ALL, bf16=dict(tile=3), f16=dict(tile=3), f32=dict(f32k, tile=0))
    _row("upsample", case(9, 64, 64, 16, B=2, upsample=1), ALL, bf16=dict(tile=5), f16=dict(tile=5), f32=dict(f32k, tile=0))
    _row("upsample", case(9, 64, 64, 16, B=2, upsample=1, mode=1), ALL, bf16=dict(tile=5), f16=dict(tile=5), f32=dict(f32k, tile=0))
    _row("zero-insert dgrad", case(9, 64, 64, 16, B=2, zins=1, transposed=1), ALL, bf16=dict(tile=5), f16=dict(tile=5), f32=dict(f32k, tile=0))
    _row("zero-insert dgrad", case(9, 64, 64, 16, B=2, zins=1, transposed=1, accumulate=1), ALL, bf16=dict(tile=5), f16=dict(tile=5),
         f32=dict(f32k, tile=0))
    for B in (2, 3):
        _row("dgrad stride 1", case(9, 64, 48, 16, B=B, mode=4, transposed=1), ALL, bf16=dict(tile=5), f16=dict(tile=5),
             f32=dict(f32k, tile=0))
    _row("dgrad stride 1", case(9, 64, 48, 16, B=2, mode=0, transposed=1, accumulate=1), ALL, bf16=dict(tile=5), f16=dict(tile=5),
         f32=dict(f32k, tile=0))
    # 1x1: tile 0 for B >= 2, tile 5 for B = 1 (a 64-multiple of couts up to 32 x 32 goes to tile 3 at B = 1: re-derived)
    for mode in (0, 2):
        _row("1x1 tiles", case(1, 128, 128, 32, B=3, mode=mode), ALL, bf16=dict(tile=0, kernel="conv_mfma_bf16x3<1,2,2,2,2"),
             f16=dict(tile=0), f32=dict(f32k, tile=0))
        _row("1x1 tiles", case(1, 112, 96, 32, B=1, mode=mode), ALL, bf16=dict(tile=5, split=False, kernel="conv_mfma_bf16x3<1,2,4,2,2"),
             f16=dict(tile=5), f32=dict(f32k, tile=0))
        _row("1x1 tiles", case(1, 128, 128, 32, B=1, mode=mode), ALL, bf16=dict(tile=3), f16=dict(tile=3), f32=dict(f32k, tile=0))
    _row("1x1 tiles", case(1, 128, 128, 32, B=3, accumulate=1), LP, bf16=dict(tile=0))
    # the DMA-fed 1x1 GEMM
    for mode in (0, 2):
        _row("GEMM tm=4 split", case(1, 320, 1280, 16, B=1, mode=mode), LP, all=dict(kernel="conv_gemm_bf16x3<4>", gemm_tm=4, split=True))
    _row("GEMM tm=4 split", case(1, 320, 1280, 16, B=1, accumulate=1, res=True), LP, all=dict(gemm_tm=4, split=True))
    _row("GEMM tm=4", case(1, 320, 2560, 32, B=5), LP, all=dict(kernel="conv_gemm_bf16x3<4>", gemm_tm=4, split=False))
    _row("GEMM tm=2", case(1, 2560, 640, 16, B=2), LP, all=dict(kernel="conv_gemm_bf16x3<2>", gemm_tm=2))
    _row("GEMM declined", case(1, 320, 1280, 48, B=1), LP, refused=True, all=dict(kernel="conv_mfma_bf16x3<1,", gemm_tm=0, tile=5))
    # the tap-pair kernel and the shapes it declines
    for mode in (0, 1, 3, 4):
        _row("tap-pair", case(9, 32, 128, 128, B=2, mode=mode), LP, all=dict(kernel="conv_pair_bf16x3", pair=1, tile=5, split=False, tail=0))
    _row("tap-pair", case(9, 32, 128, 128, B=2, accumulate=1, res=True), LP, all=dict(pair=1))
    _row("pair declined", case(9, 48, 128, 128, B=2), LP, all=dict(kernel="conv_mfma_bf16x3<9,2,4,2,2", pair=0, tile=5))
    _row("pair declined", case(9, 32, 128, 128, 144, B=2), LP, refused=True, all=dict(kernel="conv_mfma_bf16x3<9,2,4,2,2", pair=0, tile=5))
    # K-concatenated shortcut; with bias2 the shortcut runs first
    for mode in (1, 3):
        _row("kcat", case(9, 64, 128, 64, B=4, mode=mode, Cin2=32), ALL, bf16=dict(kernel="conv_kcat_bf16x3", kcat=32, sc_first=0, tile=5),
             f16=dict(kernel="conv_kcat_f16", kcat=32, sc_first=0), f32=dict(f32k, sc_first=1))
        _row("kcat", case(9, 64, 128, 64, B=4, mode=mode, Cin2=32, bias2=True), LPH, all=dict(kcat=0, sc_first=1, tile=5))
    # tail-probe split
    _row("tail split", case(1, 128, 128, 64, B=9), LP, all=dict(tile=0, split=False, tail=1, tail_split=True))
    _row("tail split", case(9, 128, 128, 128, B=5), LP, all=dict(kernel="conv_pair_bf16x3", pair=1, split=False, tail=1, tail_split=True),
         probes=(0, 3, 4))
    # norm-cotangent term in the 1x1 epilogue; declined behind split-K (and by the exact-fp32 kernel)
    _row("cot epilogue", case(1, 64, 128, 64, B=4, cot=True), ALL, bf16=dict(cot=1, tile=0, split=False), f16=dict(cot=1), f32=dict(f32k, cot=0))
    _row("cot epilogue", case(1, 64, 128, 8, B=1, cot=True), LP, all=dict(cot=1, tile=3))
    _row("cot epilogue", case(1, 128, 128, 8, B=1, cot=True), LP, all=dict(cot=0, split=True))


_build_table()


def sub_case(d, ops, probes):
    """the case and operands restricted to the samples `probes` (the reference of a big case on a main and a tail probe only)"""
    idx = torch.tensor(probes)
    d2 = dict(d, B=len(probes))
    o2 = {k: (v.index_select(0, idx) if k in ("in", "bias2", "res", "out0", "tst", "tc", "in2", "cot_d", "cot_tc") else v)
          for k, v in ops.items()}
    return d2, o2


def check_plan(plan, exp, d) -> List[str]:
    """the plan text of a case against its row's expectation: a list of complaints (empty: as expected)"""
    main = plan
    if d["taps"] == 9:      # a shortcut that ran first is a 1x1 launch ahead of the 3x3 one
        main = [p for p in plan if not (p["kernel"].startswith("conv_mfma") and "<1," in p["kernel"])]
    short = [p for p in plan if p not in main]
    bad = []
    if not main:
        return ["no launch of the main operator in the plan"]
    l0 = main[0]
    tail = [p for p in main if p["launch"] == 1]

    def want(key, got, val):
        if got != val:
            bad.append(f"{key}: planned {got!r}, the table says {val!r}")
    for k, v in exp.items():
        if k == "kernel":
            if v not in l0["kernel"]:
                bad.append(f"kernel: planned {l0['kernel']}, the table says {v}")
        elif k == "tile":
            want(k, l0["tile"], v)
        elif k == "split":
            want(k, l0["nsplit"] > 1, v)
        elif k == "gemm_tm":
            want(k, l0["gemm_tm"] if l0["gemm"] else 0, v)
        elif k == "pair":
            want(k, l0["pair"], v)
        elif k == "kcat":
            want(k, l0["Cin2"], v)
        elif k == "sc_first":
            want(k, l0["sc_first"], v)
            want("shortcut launches", len(short) > 0, bool(v))
        elif k == "cot":
            want(k, l0["cot"], v)
        elif k == "tail":
            want(k, sum(p["B"] for p in tail), v)
            if v:
                want("main probes", sum(p["B"] for p in main if p["launch"] == 0), d["B"] - v)
        elif k == "tail_split":
            want(k, bool(tail) and tail[0]["nsplit"] > 1, v)
        else:
            raise KeyError(k)
    return bad


def parse_plan(text: str) -> List[dict]:
    """the launch lines of conv_plan_text.h (what loco_debug_conv returns) as dicts; everything but `kernel` and `stats` is an
    integer.  A plan's closing line (stats_all, keep_ntile; tests/stats_oracle.parse_plan reads it) is no launch and is left out;
    texts from before the statistics words parse as they did."""
    plan = []
    for line in text.splitlines():
        rec = dict(f.split("=", 1) for f in line.split(" ") if f)
        if "launch" in rec:
            plan.append({k: (v if k in ("kernel", "stats") else int(v)) for k, v in rec.items()})
    return plan


def plan_line(d, prec: str) -> str:
    """the case as one input line of tests/c/conv_plan_cases.cpp"""
    in_padded = 1 if d["in_arena"] else 0
    return " ".join(str(int(v)) for v in (PRECISIONS[prec], d["taps"], d["Cin"], d["Cout"], d["H"], d["W"], d["B"], d["mode"], d["stride"],
                                          pad_of(d), d["upsample"], d["zins"], in_padded, d["Cin2"], d["bias2"], d["cot"], d["accumulate"]))
