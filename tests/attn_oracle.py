"""Float64 reference of ONE pass of ONE attention stage (loco_debug_attn, include/loco_hip_diag.h), its componentwise error
scale, the error the split-bf16 number format alone causes on the route the engine is expected to take, the operands and the
case table of tests/test_gpu_attn_oracle.py.

What is restated (the comments in the product that specify the passes, not their launch sequences):
  self-attention core (engine.hip "multi-head self-attention core", attn_flash.hip header; the reference project's call sites are
  guided_diffusion/unet.py:330-356 QKVAttentionLegacy and diffusers' AttnAddedKVProcessor for the [text ; image] keys):
      forward    P = softmax_j(s q^T [K_text | k]) with the padding columns L .. Lt masked out,  o = [V_text | v] P^T,  s = CH^-1/2
      tangent    do = V W^T + dv P_img^T - r o,   W = s P o dS,  dS = dq^T [K_text | k] + q^T [0 | dk],  r_i = sum_j W_ij
      cotangent  G = s P o (gP - delta),  gP = g_o^T [V_text | v],  delta_i = <g_o_i, o_i>;
                 g_q = [K_text | k] G^T,  g_k = q G_img,  g_v = g_o P_img
  text cross-attention (xattn.hip:5-7; diffusers' attn2 of a SpatialTransformer block):
      forward    P = softmax_l(s q^T K),  o = V P^T;   tangent R = s P o (dS - <P, dS>), dS = dq^T K, do = V R^T;
      cotangent  the tangent with K and V exchanged (g_o -> g_q)
The linear passes take the primal P and o from the caller (the float64 reference rounded to float32), so each pass is one unit.

A case `d` is a plain dict (kind, T, NH, CH, B, Lt, L, pair); `ops` holds float64 CPU tensors whose values are exactly
representable in float32, in the engine's [channel][token] layout ([C][T], per-probe tensors [B][C][T], P [NH][T][Tk]).

    reference(d, ops, pas)          {output name: tensor}, float64
    magnitude(d, ops, pas)          the same expression with every operand of the LAST products and every term in absolute value: P
                                    stays; the score-shaped intermediates enter by the absolute value they have (dS - <P, dS>
                                    becomes |dS| + <P, |dS|>, gP - delta becomes |gP| + |delta|, W becomes s P |dS|);
                                    acc - r o becomes |acc|' + |r| |o| with |acc|' the products of absolute operands: A.  (With the
                                    first products also taken over absolute operands A grows by about sqrt(CH) and a dropped
                                    lo hi product of the score GEMM passes: tests/test_attn_oracle_host.py.)  For the forward's
                                    P the scale is P (1 + |S - rowmax S|): the relative error of an fp32 exponential grows
                                    with its argument.
    emulated(d, ops, pas, flags)    the reference with both operands of every product that runs on the bf16 pipe split into
                                    hi + lo and the lo lo product dropped -- the in-kernel intermediates W, G and the P tile of the
                                    flash kernels included; products on the exact-fp32 kernels unchanged
    tolerance(d, ops, pas, flags)   tau of |out - ref| <= tau A + 1e-30 per output tensor, from the reference alone

tau = MARGIN (format + accumulation + row operation), MARGIN = 4 as for the convolutions (tests/conv_oracle.py):
  format         max |emulated - reference| / A  (0 on the exact-fp32 routes)
  accumulation   (n + 8) 2^-24, n = the fp32 additions that meet in one output element:
                   self  forward P: CH + Tk (score, row sum)      o: Tk
                         tangent do: 2 CH + 2 Tk  (dq^T k and q^T dk; W v and P dv -- the r sum rides with the +8: it enters one
                                     product r_i o_i)
                         cotangent g_q: 2 CH + Tk (gP, delta; the sum over keys)   g_k: 2 CH + T   g_v: T
                   cross forward P: CH + Lp   o: Lp      tangent / cotangent: CH + 2 Lp (scores, <P, dS>, values)
  row operation  softmax (forward) or softmax-Jacobian (linear passes of the generic and cross routes) evaluated in float32 torch on
                 the float32-rounded scores against float64, relative to its absolute-value version (as conv_oracle.prologue_term)
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

MARGIN = 4.0
EPS_ABS = 1e-30
PRECISIONS = {"f32": 0, "bf16x3": 1, "f16": 2}
PASSES = ("fwd", "tan", "cot")
FLASH_OWN, FLASH_BLK, FLASH_CH_MIN, FLASH_CH_MAX, FLASH_TXT_CH_MAX = 128, 64, 8, 96, 64      # attn_flash_supported (attn_flash.hip)
XA_LG = (4, 8, 12, 20, 32)                                                                    # xattn.hip: instantiated columns per lane
XA_LDS = 150 * 1024


def case(kind, T, NH, CH, B, Lt=0, L=0, pair=False) -> dict:
    return dict(kind=kind, T=T, NH=NH, CH=CH, B=B, Lt=Lt, L=L, pair=bool(pair))


def lp_of(d) -> int:
    """padded context rows of the cross-attention (program.hip: ctx_Lp)"""
    return 64 * ((d["L"] + 63) // 64)


def tk_of(d) -> int:
    return lp_of(d) if d["kind"] == "cross" else d["Lt"] + d["T"]


# ---------------------------------------------------------------------------------------------------------------------------
# products

def _f32(t):
    return t.to(torch.float32).to(torch.float64)


def _bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _split(t):
    t32 = _f32(t)
    hi = _bf16(t32)
    return hi, _bf16(t32 - hi)


def _mm(eq, a, b, split=False, drop_lohi=False):
    """einsum(eq, a, b); split: both operands as bf16 hi + lo without the lo lo product (drop_lohi: a planted fault, lo hi gone too)"""
    if not split:
        return torch.einsum(eq, a, b)
    ah, al = _split(a)
    bh, bl = _split(b)
    out = torch.einsum(eq, ah + al, bh + bl) - torch.einsum(eq, al, bl)
    if drop_lohi:
        out = out - torch.einsum(eq, al, bh)
    return out


def _h(t, NH):
    """[..., C, X] -> [..., NH, CH, X]"""
    return t.reshape(*t.shape[:-2], NH, t.shape[-2] // NH, t.shape[-1])


def _c(t):
    """[..., NH, CH, X] -> [..., C, X]"""
    return t.reshape(*t.shape[:-3], t.shape[-3] * t.shape[-2], t.shape[-1])


class _Cfg:
    """how one evaluation of a pass differs from the plain reference"""

    def __init__(self, absolute=False, flags=None, fault=None):
        self.absolute, self.flags, self.fault = absolute, flags or {}, fault

    def x(self, t):
        return t.abs() if self.absolute else t

    def sub(self, a, b):
        return a + b if self.absolute else a - b

    def sp(self, name):
        return bool(self.flags.get(name, False))


def _chan_fault(cfg, *ts):
    """planted fault: channels 64 - 79 of an 80-channel head missing from a contraction"""
    if cfg.fault != "ch64_79":
        return ts
    out = []
    for t in ts:
        t = t.clone()
        t[..., 64:80, :] = 0
        out.append(t)
    return out


def _self_scores(d, ops, cfg, q):
    """(S [B][NH][T][Tk] before the mask and the scale's fault, text columns first)"""
    NH, Lt, s = d["NH"], d["Lt"], 1.0 / math.sqrt(d["CH"])
    parts = []
    if Lt:
        st = s * _mm("bhci,hcj->bhij", q, cfg.x(_h(ops["kt"], NH)), cfg.sp("S_txt"))
        if cfg.fault == "scale2_txt":
            st = st * s
        parts.append(st)
    parts.append(s * _mm("bhci,bhcj->bhij", q, cfg.x(_h(ops["fk"], NH)), cfg.sp("S_img")))
    return torch.cat(parts, -1)


def _self_forward(d, ops, cfg) -> Dict[str, torch.Tensor]:
    NH, Lt, L = d["NH"], d["Lt"], d["L"]
    S = _self_scores(d, ops, _Cfg(flags=cfg.flags, fault=cfg.fault), _h(ops["fq"], NH))
    if Lt and cfg.fault != "pad_in_softmax":
        S[..., L:Lt] = -math.inf
    P = torch.softmax(S, -1)
    if cfg.absolute:
        Sm = torch.where(torch.isinf(S), torch.zeros_like(S), (S - S.max(-1, keepdim=True).values).abs())
        Pm = P * (1.0 + Sm)
    o = _mm("bhcj,bhij->bhci", cfg.x(_h(ops["fv"], NH)), P[..., Lt:], cfg.sp("O_img"))
    if Lt:
        o = o + _mm("hcj,bhij->bhci", cfg.x(_h(ops["vt"], NH)), P[..., :Lt], cfg.sp("O_txt"))
    return dict(P=Pm if cfg.absolute else P, o=_c(o))


def _self_tangent(d, ops, cfg) -> Dict[str, torch.Tensor]:
    NH, Lt, s = d["NH"], d["Lt"], 1.0 / math.sqrt(d["CH"])
    x = cfg.x
    q, k, dq, dk = (_h(ops[n], NH) for n in ("q", "k", "dq", "dk"))
    v, dv = x(_h(ops["v"], NH)), x(_h(ops["dv"], NH))
    P, o = ops["P"], x(_h(ops["o"], NH))
    lohi = cfg.fault == "drop_lohi"
    dq_, k_, q_, dk_ = _chan_fault(cfg, dq, k, q, dk)
    dS = _mm("bhci,hcj->bhij", dq_, k_, cfg.sp("dS_img"), lohi) + _mm("hci,bhcj->bhij", q_, dk_, cfg.sp("dS_img"), lohi)
    if Lt:
        dq_t, kt_ = _chan_fault(cfg, dq, _h(ops["kt"], NH))
        dS = torch.cat([_mm("bhci,hcj->bhij", dq_t, kt_, cfg.sp("dS_txt"), lohi), dS], -1)
    W = s * P * dS
    if cfg.fault == "scale2_txt":
        W[..., :Lt] *= s
    r = x(W.sum(-1))
    W = x(W)
    W2, P2 = W, P
    if cfg.fault == "swap":      # two streamed tokens of one 16-token k-step exchanged, in the second product only
        j = Lt + 18
        W2 = W.clone()
        W2[..., [j, j + 1]] = W[..., [j + 1, j]]
    if cfg.fault == "skip_last":
        W2, P2 = W.clone(), P.clone()
        W2[..., -64:] = 0
        P2[..., -64:] = 0
        r = W2.sum(-1)
    acc = _mm("hcj,bhij->bhci", v, W2[..., Lt:], cfg.sp("do_W_img")) + _mm("bhcj,hij->bhci", dv, P2[..., Lt:], cfg.sp("do_P_img"))
    if Lt:
        acc = acc + _mm("hcj,bhij->bhci", x(_h(ops["vt"], NH)), W2[..., :Lt], cfg.sp("do_W_txt"))
    ro = r.unsqueeze(-2) * o
    if cfg.fault == "no_ro":
        ro = 0 * ro
    return dict(out=_c(cfg.sub(acc, ro)))


def _self_cotangent(d, ops, cfg) -> Dict[str, torch.Tensor]:
    NH, Lt, s = d["NH"], d["Lt"], 1.0 / math.sqrt(d["CH"])
    x = cfg.x
    q, k = x(_h(ops["q"], NH)), x(_h(ops["k"], NH))
    go, P = _h(ops["go"], NH), ops["P"]
    lohi = cfg.fault == "drop_lohi"
    go_, v_ = _chan_fault(cfg, go, _h(ops["v"], NH))
    gP = _mm("bhci,hcj->bhij", go_, v_, cfg.sp("gP_img"), lohi)
    if Lt:
        gP = torch.cat([_mm("bhci,hcj->bhij", go, _h(ops["vt"], NH), cfg.sp("gP_txt"), lohi), gP], -1)
    delta = (go * _h(ops["o"], NH)).sum(-2)
    if cfg.fault == "no_ro":
        delta = 0 * delta
    G = s * P * cfg.sub(x(gP), x(delta).unsqueeze(-1))
    go = x(go)
    if cfg.fault == "scale2_txt":
        G[..., :Lt] *= s
    G2, P2 = G, P
    if cfg.fault == "swap":
        j = Lt + 18
        G2 = G.clone()
        G2[..., [j, j + 1]] = G[..., [j + 1, j]]
    if cfg.fault == "skip_last":
        G2, P2 = G.clone(), P.clone()
        G2[..., -64:] = 0
        P2[..., -64:, :] = 0      # (for g_v the streamed axis is the query one)
    gq = _mm("hcj,bhij->bhci", k, G2[..., Lt:], cfg.sp("gq_img"))
    if Lt:
        gq = gq + _mm("hcj,bhij->bhci", x(_h(ops["kt"], NH)), G2[..., :Lt], cfg.sp("gq_txt"))
    gk = _mm("hci,bhij->bhcj", q, G[..., Lt:], cfg.sp("gk"))
    gv = _mm("bhci,hij->bhcj", go, P2[..., Lt:], cfg.sp("gv"))
    return dict(gq=_c(gq), gk=_c(gk), gv=_c(gv))


def _cross(d, ops, cfg, pas) -> Dict[str, torch.Tensor]:
    NH, L, Lp, s = d["NH"], d["L"], lp_of(d), 1.0 / math.sqrt(d["CH"])
    x = cfg.x
    K, V = x(_h(ops["kt"], NH)), x(_h(ops["vt"], NH))
    if pas == "fwd":
        S = s * torch.einsum("bhci,hcl->bhil", _h(ops["fq"], NH), _h(ops["kt"], NH))
        if cfg.fault == "scale2_txt":
            S = S * s
        if cfg.fault != "pad_in_softmax":
            S[..., L:] = -math.inf
        P = torch.softmax(S, -1)
        Pm = P
        if cfg.absolute:
            Pm = P * (1.0 + torch.where(torch.isinf(S), torch.zeros_like(S), (S - S.max(-1, keepdim=True).values).abs()))
        return dict(P=Pm, o=_c(torch.einsum("hcl,bhil->bhci", V, P)))
    X = _h(ops["dq" if pas == "tan" else "go"], NH)
    K1, K2 = (_h(ops["kt"], NH), V) if pas == "tan" else (_h(ops["vt"], NH), K)
    P = ops["P"]
    dS = x(torch.einsum("bhci,hcl->bhil", X, K1))
    dot = (P * dS).sum(-1, keepdim=True)
    if cfg.fault == "no_ro":
        dot = 0 * dot
    R = s * P * cfg.sub(dS, dot)
    if cfg.fault == "scale2_txt":
        R = R * s
    if cfg.fault == "swap":
        R = R.clone()
        R[..., [1, 2]] = R[..., [2, 1]]
    return {("out" if pas == "tan" else "gq"): _c(torch.einsum("hcl,bhil->bhci", K2, R))}


def _eval(d, ops, pas, cfg) -> Dict[str, torch.Tensor]:
    assert pas in PASSES
    if d["kind"] == "cross":
        return _cross(d, ops, cfg, pas)
    return {"fwd": _self_forward, "tan": _self_tangent, "cot": _self_cotangent}[pas](d, ops, cfg)


def reference(d, ops, pas):
    return _eval(d, ops, pas, _Cfg())


def magnitude(d, ops, pas):
    return _eval(d, ops, pas, _Cfg(absolute=True))


def emulated(d, ops, pas, flags, fault=None):
    """flags: {product name: True} for the products the expected route runs on the bf16 pipe (route_of); fault: a planted error
    of tests/test_attn_oracle_host.py"""
    return _eval(d, ops, pas, _Cfg(flags=flags, fault=fault))


# ---------------------------------------------------------------------------------------------------------------------------
# tolerance

def additions(d, pas) -> Dict[str, int]:
    CH, T, Tk = d["CH"], d["T"], tk_of(d)
    if d["kind"] == "cross":
        return dict(P=CH + Tk, o=Tk) if pas == "fwd" else {("out" if pas == "tan" else "gq"): CH + 2 * Tk}
    if pas == "fwd":
        return dict(P=CH + Tk, o=Tk)
    if pas == "tan":
        return dict(out=2 * CH + 2 * Tk)
    return dict(gq=2 * CH + Tk, gk=2 * CH + T, gv=T)


def row_term(d, ops, pas, flash) -> float:
    """the row operation in float32 torch against float64, relative to its absolute-value version; 0 where the route has no row
    kernel (the flash kernels form W and G inside their products: the format term carries them)"""
    NH, L, s = d["NH"], d["L"], 1.0 / math.sqrt(d["CH"])
    cross = d["kind"] == "cross"
    if pas == "fwd":
        if cross:
            S = s * torch.einsum("bhci,hcl->bhil", _h(ops["fq"], NH), _h(ops["kt"], NH))
            S[..., L:] = -math.inf
        else:
            S = _self_scores(d, ops, _Cfg(), _h(ops["fq"], NH))
            if d["Lt"]:
                S[..., L:d["Lt"]] = -math.inf
        S = _f32(S)
        P64 = torch.softmax(S, -1)
        P32 = torch.softmax(S.to(torch.float32), -1).to(torch.float64)
        Sm = torch.where(torch.isinf(S), torch.zeros_like(S), (S - S.max(-1, keepdim=True).values).abs())
        return float(((P32 - P64).abs() / (P64 * (1.0 + Sm)).clamp_min(1e-300)).max())
    if flash:
        return 0.0
    P = ops["P"]
    if cross:
        X = _h(ops["dq" if pas == "tan" else "go"], NH)
        dS = torch.einsum("bhci,hcl->bhil", X, _h(ops["kt" if pas == "tan" else "vt"], NH))
    elif pas == "tan":
        q, k, dq, dk = (_h(ops[n], NH) for n in ("q", "k", "dq", "dk"))
        dS = torch.einsum("bhci,hcj->bhij", dq, k) + torch.einsum("hci,bhcj->bhij", q, dk)
        if d["Lt"]:
            dS = torch.cat([torch.einsum("bhci,hcj->bhij", dq, _h(ops["kt"], NH)), dS], -1)
    else:
        go = _h(ops["go"], NH)
        dS = torch.einsum("bhci,hcj->bhij", go, _h(ops["v"], NH))
        if d["Lt"]:
            dS = torch.cat([torch.einsum("bhci,hcj->bhij", go, _h(ops["vt"], NH)), dS], -1)
    dS = _f32(dS)
    j64 = s * P * (dS - (P * dS).sum(-1, keepdim=True))
    P32, dS32 = P.to(torch.float32), dS.to(torch.float32)
    j32 = (torch.tensor(s, dtype=torch.float32) * P32 * (dS32 - (P32 * dS32).sum(-1, keepdim=True))).to(torch.float64)
    jabs = s * P * (dS.abs() + (P * dS.abs()).sum(-1, keepdim=True))
    keep = jabs > 0
    return float(((j32 - j64).abs()[keep] / jabs[keep]).max())


def tolerance(d, ops, pas, flags, ref=None, A=None, flash=False) -> Dict[str, dict]:
    """per output tensor: dict(format, accumulation, row, tau)"""
    ref = reference(d, ops, pas) if ref is None else ref
    A = magnitude(d, ops, pas) if A is None else A
    emu = emulated(d, ops, pas, flags) if any(flags.values()) else None
    row = row_term(d, ops, pas, flash)
    out = {}
    for name, n in additions(d, pas).items():
        fmt = 0.0
        if emu is not None:
            keep = A[name] > 0
            fmt = float(((emu[name] - ref[name]).abs()[keep] / A[name][keep]).max())
        acc = (n + 8) * 2.0 ** -24
        out[name] = dict(format=fmt, accumulation=acc, row=row, tau=MARGIN * (fmt + acc + row))
    return out


def worst(name, out, ref, A, tau, d):
    """(ok, message, max |out - ref| / A): the check |out - ref| <= tau A + EPS_ABS on every element, NaN counting as a failure;
    the message names the worst element: tensor, probe, head, channel (or query row for P), token (or key column for P)"""
    err = (out.to(torch.float64) - ref).abs()
    ratio = err / (tau * A + EPS_ABS)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    if name == "P":
        where = "probe %d head %d query %d key column %d" % idx
    else:
        where = "probe %d head %d channel %d token %d" % (idx[0], idx[1] // d["CH"], idx[1] % d["CH"], idx[2])
    bad = int((ratio > 1).sum())
    a = float(A[idx])
    msg = (f"worst element of {name}: {where}: out {float(out[idx])!r} ref {float(ref[idx])!r} |err| / A = "
           f"{float(err[idx]) / a if a > 0 else float('inf'):.3e} against tau = {tau:.3e}; {bad} of {ratio.numel()} elements fail")
    keep = A > 0
    measured = float((err[keep] / A[keep]).nan_to_num(nan=float("inf")).max())
    if bool((err[~keep] > EPS_ABS).any()) or bool(torch.isnan(err).any()):
        measured = float("inf")
    return bad == 0, msg, measured


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def make_operands(d, seed=0) -> Dict[str, torch.Tensor]:
    """Seeded operands, exactly representable in float32.  q and k are scaled so the scores s q^T k have variance about 3 (rows
    where a few keys dominate); q, k, v carry per-channel offsets of 0.5, 2 and 3 units -- they cancel in exact arithmetic
    (a per-channel offset of k shifts a whole score row) and are the hazard in fp32; dq, dk, dv, g_o are standard normal; the text
    keys / values are zero beyond L.  fq, fk, fv [B][C][T] are the forward's per-sample inputs (sample 0 = the primal); P and o are
    the float64 forward of the primal rounded to float32 -- what the linear passes are handed."""
    g = torch.Generator().manual_seed(1000 + seed)
    NH, CH, T, B = d["NH"], d["CH"], d["T"], d["B"]
    C = NH * CH
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    amp = 3.0 ** 0.25      # var(s q^T k) = s^2 CH amp^4 = 3
    off = lambda c, u: u * torch.sign(rn(c, 1)) * (0.75 + 0.5 * torch.rand(c, 1, generator=g, dtype=torch.float64))
    ops = {}
    if d["kind"] == "cross":
        Lp, L = lp_of(d), d["L"]
        fq = _f32(amp * rn(B, C, T) + off(C, 0.5))
        kt = _f32(amp * rn(C, Lp) + off(C, 2.0))
        vt = _f32(rn(C, Lp) + off(C, 3.0))
        kt[:, L:] = 0
        vt[:, L:] = 0
        ops.update(fq=fq, q=fq[0].clone(), kt=kt, vt=vt, dq=_f32(rn(B, C, T)), go=_f32(rn(B, C, T)))
    else:
        Lt, L = d["Lt"], d["L"]
        fq = _f32(amp * rn(B, C, T) + off(C, 0.5))
        fk = _f32(amp * rn(B, C, T) + off(C, 2.0))
        fv = _f32(rn(B, C, T) + off(C, 3.0))
        ops.update(fq=fq, fk=fk, fv=fv, q=fq[0].clone(), k=fk[0].clone(), v=fv[0].clone())
        if Lt:
            kt = _f32(amp * rn(C, Lt) + off(C, 2.0))
            vt = _f32(rn(C, Lt) + off(C, 3.0))
            kt[:, L:] = 0
            vt[:, L:] = 0
            ops.update(kt=kt, vt=vt)
        ops.update(dq=_f32(rn(B, C, T)), dk=_f32(rn(B, C, T)), dv=_f32(rn(B, C, T)), go=_f32(rn(B, C, T)))
    d1 = dict(d, B=1)
    o1 = {k: (v[:1] if k in ("fq", "fk", "fv") else v) for k, v in ops.items()}
    f = reference(d1, o1, "fwd")
    ops["P"], ops["o"] = _f32(f["P"][0]), _f32(f["o"][0])
    return ops


def sub_case(d, ops, probes):
    """the case and operands restricted to the probes `probes`"""
    idx = torch.tensor(list(probes))
    per = ("fq", "fk", "fv", "dq", "dk", "dv", "go")
    return dict(d, B=len(probes)), {k: (v.index_select(0, idx) if k in per else v) for k, v in ops.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# the expected route: the public predicates of kernels.h on the case's shape (what the table claims the engine does)

def flash_supported(d) -> bool:
    T, CH, Lt = d["T"], d["CH"], d["Lt"]
    ok = CH >= FLASH_CH_MIN and T >= FLASH_OWN and T % FLASH_OWN == 0
    return ok and (CH <= FLASH_TXT_CH_MAX and Lt % FLASH_BLK == 0 if Lt else CH <= FLASH_CH_MAX)


def xattn_fused(d) -> bool:
    need = (d["L"] + 3) // 4
    lg = next((g for g in XA_LG if g >= need), 0)
    return lg > 0 and d["T"] % 64 == 0 and 2 * d["CH"] * 4 * lg * 4 <= XA_LDS


def _gemm(M, N, K, batch, heads, kcat, low, rec):
    """the kernel attn_gemm picks (gemm_rec_eligible, gemm_prefers_bf16x3), as one route line"""
    macs = float(M) * N * K * (2 if kcat else 1) * batch * heads
    kernel = "gemm_f32"
    if low and K >= 256 and macs >= 4e9:
        kernel = "gemm_rec" if rec and M >= 128 and N >= 256 else "gemm_bf16x3"
    return dict(kernel=kernel, M=M, N=N, K=K, batch=batch, heads=heads, kcat=int(kcat))


def route_of(d, pas, prec, workspace=True, rec=True):
    """(expected route lines, flags of emulated(), flash?) of one pass under one precision; workspace: the flash record workspace is
    handed over; rec: LOCO_GEMM_REC is not 0"""
    low = prec != "f32"
    T, NH, CH, B, Lt = d["T"], d["NH"], d["CH"], d["B"], d["Lt"]
    K = lambda name: dict(kernel=name)
    lines, flags = [], {}
    if d["kind"] == "cross":
        Lp = lp_of(d)
        if xattn_fused(d):
            return [K("xattn_fused_fwd" if pas == "fwd" else "xattn_fused_lin")], {}, False
        f32 = lambda M, N, Kk: _gemm(M, N, Kk, B, NH, False, False, False)
        return [f32(T, Lp, CH), K("softmax_rows" if pas == "fwd" else "softmax_jac"), f32(CH, T, Lp)], {}, False

    def g(name, M, N, Kk, kcat=False, text=False):
        line = _gemm(M, N, Kk, B, NH, kcat, low and not text, rec)
        lines.append(line)
        flags[name] = line["kernel"] != "gemm_f32"
        return line
    if pas == "fwd":
        if Lt:
            g("S_txt", T, Lt, CH, text=True)
        g("S_img", T, T, CH)
        lines.append(K("softmax_rows"))
        g("O_img", CH, T, T)
        if Lt:
            g("O_txt", CH, T, Lt, text=True)
        return lines, flags, False
    if low and flash_supported(d):
        names = ("dS_img", "dS_txt", "do_W_img", "do_P_img", "do_W_txt") if pas == "tan" else ("gP_img", "gP_txt", "gq_img", "gq_txt", "gk", "gv")
        flags = {n: True for n in names}
        pre = "flash_dma_" if workspace else "flash_"
        lines = ([K("attn_split")] if workspace else []) + [K(pre + n) for n in (("tan",) if pas == "tan" else ("cotq", "cotk"))]
        return lines, flags, True
    if pas == "tan":
        kcat = d["pair"] and (T <= 256 or _gemm(T, T, CH, B, NH, True, low, rec)["kernel"] == "gemm_rec")
        if Lt:
            g("dS_txt", T, Lt, CH, text=True)
        if kcat:
            g("dS_img", T, T, CH, kcat=True)
        else:
            a, b = g("dS_img", T, T, CH), g("dS_img", T, T, CH)
            assert a["kernel"] == b["kernel"]
        lines.append(K("softmax_jac"))
        if kcat:
            g("do_W_img", CH, T, T, kcat=True)
            flags["do_P_img"] = flags["do_W_img"]
        else:
            g("do_P_img", CH, T, T)
            g("do_W_img", CH, T, T)
        if Lt:
            g("do_W_txt", CH, T, Lt, text=True)
        return lines, flags, False
    g("gv", CH, T, T)
    if Lt:
        g("gP_txt", T, Lt, CH, text=True)
    g("gP_img", T, T, CH)
    lines.append(K("softmax_jac"))
    g("gq_img", CH, T, T)
    if Lt:
        g("gq_txt", CH, T, Lt, text=True)
    g("gk", CH, T, T)
    return lines, flags, False


def check_route(route: List[dict], expected: List[dict]) -> List[str]:
    """the route text of a case (parsed: one dict per launch) against the expectation: a list of complaints (empty: as expected)"""
    bad = []
    if [r["kernel"] for r in route] != [e["kernel"] for e in expected]:
        return [f"launches {[r['kernel'] for r in route]}, expected {[e['kernel'] for e in expected]}"]
    for i, (r, e) in enumerate(zip(route, expected)):
        for k, v in e.items():
            if r.get(k) != v:
                bad.append(f"launch {i} ({e['kernel']}): {k} = {r.get(k)}, expected {v}")
    return bad


def parse_route(text: str) -> List[dict]:
    out = []
    for line in text.splitlines():
        rec = dict(f.split("=", 1) for f in line.split(" "))
        out.append({k: (v if k == "kernel" else int(v)) for k, v in rec.items()})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the case table

def _row(family, rid, d, passes=("tan", "cot"), precs=("f32", "bf16x3"), both_ws=False, probes=None, refused=None, rec=True,
         f16=False, B_by_pass=None):
    return dict(family=family, id=rid, case=d, passes=tuple(passes), precs=tuple(precs), both_ws=both_ws, probes=probes,
                refused=refused, rec=rec, f16=f16, B_by_pass=B_by_pass or {})


def _build_table():
    R = []
    fl = lambda rid, fam, *a, **kw: R.append(_row(fam, rid, case("self", *a, **kw), both_ws=True))
    fl("flash42_t128", "flash 4/2", 128, 2, 64, 1)
    R[-1]["f16"] = True                                   # also under f16: must equal bf16x3 bit for bit
    fl("flash32_t384", "flash 3/2", 384, 3, 40, 3)
    fl("flash32_ch8", "flash 3/2", 256, 1, 8, 2)
    fl("flash32_ch48", "flash 3/2", 256, 2, 48, 1)
    fl("flash53_ch72", "flash 5/3", 256, 1, 72, 1)
    fl("flash53_ch80", "flash 5/3", 256, 1, 80, 2)
    fl("flash63_ch96", "flash 6/3", 128, 2, 96, 1)
    fl("flash_long", "flash long", 1024, 1, 64, 1)
    fl("flash_text_l5", "flash text", 128, 2, 64, 2, Lt=64, L=5)
    fl("flash_text_l77", "flash text", 256, 1, 32, 1, Lt=128, L=77)
    fl("flash_text_full", "flash text", 128, 1, 64, 1, Lt=64, L=64)
    all3 = ("fwd", "tan", "cot")
    R.append(_row("generic", "generic_pair", case("self", 64, 2, 32, 3, pair=True), passes=all3))
    R.append(_row("generic", "generic_xfmr", case("self", 64, 4, 16, 2), passes=all3))
    R.append(_row("generic", "generic_wide", case("self", 256, 1, 128, 2, pair=True)))
    R.append(_row("generic text", "generic_text", case("self", 64, 1, 64, 2, Lt=128, L=77), passes=all3))
    R.append(_row("generic", "generic_f32_text", case("self", 128, 2, 64, 2, Lt=64, L=5), precs=("f32",)))
    R.append(_row("long rows", "long_rows", case("self", 1024, 1, 16, 1, Lt=64, L=64), passes=all3, precs=("f32",)))
    big = dict(probes=(0, 7, 15), B_by_pass=dict(tan=8, cot=16), precs=("bf16x3",))
    R.append(_row("record GEMM", "gemm_rec", case("self", 1024, 1, 256, 16, pair=True), **big))
    R.append(_row("converting bf16x3 GEMM", "gemm_bf16x3", case("self", 1024, 1, 256, 16, pair=True), rec=False, **big))
    cr = lambda rid, fam, *a, **kw: R.append(_row(fam, rid, case("cross", *a, **kw), passes=all3))
    cr("cross_lg4", "cross", 64, 2, 40, 2, L=7)
    cr("cross_lg8", "cross", 64, 1, 64, 2, L=17)
    cr("cross_lg12", "cross", 128, 2, 10, 1, L=48)
    cr("cross_lg20_lds", "cross", 64, 1, 160, 1, L=77)
    cr("cross_lg32_part", "cross", 64, 1, 64, 1, L=81)
    cr("cross_lg32_full", "cross", 64, 1, 64, 1, L=128)
    cr("cross_generic_l129", "cross generic", 64, 1, 32, 2, L=129)
    cr("cross_generic_lds", "cross generic", 64, 1, 256, 1, L=77)
    R.append(_row("refused", "refused_t96", case("self", 96, 1, 32, 1), passes=("tan",), precs=("f32",), refused="T must be a multiple of 64"))
    R.append(_row("refused", "refused_lt80", case("self", 128, 1, 32, 1, Lt=80, L=77), passes=("tan",), precs=("f32",),
                  refused="Lt must be a multiple of 64"))
    return R


ROWS = _build_table()


def case_of(row, pas) -> dict:
    """the row's case for one pass (the record-GEMM rows run fewer probes in the tangent)"""
    d = row["case"]
    return dict(d, B=row["B_by_pass"].get(pas, d["B"]))


def probes_of(row, pas) -> Optional[tuple]:
    if not row["probes"]:
        return None
    B = case_of(row, pas)["B"]
    return tuple(sorted({min(p, B - 1) for p in row["probes"]}))


def keys() -> List[tuple]:
    """(row id, pass, precision, workspace) of every GPU case; precision 'f16' marks the bit-identity case"""
    out = []
    for r in ROWS:
        for pas in r["passes"]:
            for prec in r["precs"]:
                for ws in ((True, False) if r["both_ws"] and prec != "f32" else (True,)):
                    out.append((r["id"], pas, prec, ws))
            if r["f16"]:
                out.append((r["id"], pas, "f16", True))
    return out
