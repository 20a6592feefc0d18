"""Float64 reference of the GroupNorm statistics subsystem (misc.hip, the statistics epilogues of conv_bf16_kernel.h, the routing
of conv_plan.hip: stats_route and engine.hip: run_conv), the tolerances of its checks and the case tables of
tests/test_gpu_stats_oracle.py and tests/test_stats_oracle_host.py.

The same numbers reach a norm by five routes -- the conv epilogue's row-tile partials + a finalize launch (`epi`), the split-K
epilogue (`splitk`), the standalone kernels behind the conv (`alone`), partials kept for a norm over a concatenation (`keep` + a
cat finalize) and the tail-probe split, which mixes `epi` and `splitk` over the samples of one tensor -- in three kinds
(FWD {mean, rstd, sc, sh}; TAN and COT {m1, m2} per group and their per-channel expansion tc).

    fwd_stats / z_of / lin_stats / apply / records / ctx_groupnorm      the operations in float64
    partials_fwd / partials_tan / partials_cot, merge_*                  row-tile partials of a tensor at a tile size, and their merge
    tol_fwd / tol_lin / tol_apply                                        the bounds, from the reference alone (docstrings)
    route32_*                                                            fp32 restatements of each route's summation structure (CPU test)

What a conv-carried statistic is compared with: the float64 statistic of the fp32 tensor the SAME launch wrote, read back -- the
epilogues take them from the values they store, so one tolerance serves f32, bf16x3 and f16 and the conv's own precision (checked
apart, conv_oracle) does not enter.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List

import torch

import conv_oracle as co

MARGIN = co.MARGIN      # the conv oracle's, for its reasons: the order of an fp32 accumulation varies (x2) and hardware may contract or
                        # split an expression differently from the statement the bound is derived from (x2)
U = 2.0 ** -24
EPS_ABS = 1e-30
ST_FWD, ST_TAN, ST_COT = 1, 2, 3
KINDS = {"fwd": ST_FWD, "tan": ST_TAN, "cot": ST_COT}
ACT_SILU, ACT_GELU = 0, 1
D = torch.float64


def _f32(t):
    return t.to(torch.float32).to(D)


def _pc(v, cpg):
    return torch.repeat_interleave(v, cpg, dim=-1)


def act_f(y, act):
    return co._gelu(y) if act == ACT_GELU else co._silu(y)


def act_d(y, act):
    return co._dgelu(y) if act == ACT_GELU else co._dsilu(y)


def act_d2(y, act):
    if act == ACT_GELU:      # d/dy [Phi(y) + y phi(y)] = phi(y) (2 - y^2)
        return 0.3989422804014327 * torch.exp(-0.5 * y * y) * (2 - y * y)
    return co._d2silu(y)


# ---------------------------------------------------------------------------------------------------------------------------
# the operations (float64).  Tensors are [B][C][HW...]; a primal and its arrays may have a leading 1 (broadcast over the samples).

def fwd_stats(x, G, gamma, beta, eps, ss_scale=None, ss_shift=None):
    """launch_gn_stats: mr [B][G][2] = {mean, rstd}, sc [B][C] = gamma rstd, sh [B][C] = beta - mean rstd gamma; with a scale-shift
    norm sc (1 + scale), sh (1 + scale) + shift"""
    B, C = x.shape[:2]
    cpg = C // G
    xg = x.reshape(B, G, -1).to(D)
    mean = xg.mean(2)
    rstd = 1.0 / torch.sqrt(xg.var(2, unbiased=False) + eps)
    sc = gamma * _pc(rstd, cpg)
    sh = beta - _pc(mean, cpg) * _pc(rstd, cpg) * gamma
    if ss_scale is not None:
        sc = sc * (1 + ss_scale)
        sh = sh * (1 + ss_scale) + ss_shift
    return torch.stack([mean, rstd], 2), sc, sh


def _bc(v, x):
    """per-channel array [Bp][C] -> broadcastable against x [B][C][...]"""
    return v.reshape(v.shape[0], v.shape[1], *([1] * (x.dim() - 2)))


def xhat_of(prim, mr, cpg):
    return (prim - _bc(_pc(mr[..., 0], cpg), prim)) * _bc(_pc(mr[..., 1], cpg), prim)


def z_of(kind, d, prim, sc, sh, mr, cpg, act=ACT_SILU, absolute=False):
    """the summand of launch_gn_tstats: kind 0 z = d, 1 z = gamma act'(sc x + sh) d, 2 z = gamma d, gamma = sc / rstd.
    absolute: every term by its absolute value, act'(y) counted as |act'(y)| + |act''(y)| (|sc x| + |sh|) (conv_oracle.prologue)"""
    if kind == 0:
        return d.abs() if absolute else d
    gm = _bc(sc / _pc(mr[..., 1], cpg), prim)
    if kind == 2:
        return gm.abs() * d.abs() if absolute else gm * d
    scb, shb = _bc(sc, prim), _bc(sh, prim)
    y = scb * prim + shb
    if absolute:
        return gm.abs() * (act_d(y, act).abs() + act_d2(y, act).abs() * ((scb * prim).abs() + shb.abs())) * d.abs()
    return gm * act_d(y, act) * d


def lin_stats(z, prim, mr, cpg):
    """tst [B][G][2] = {mean_g z, mean_g xhat z}"""
    B, C = z.shape[:2]
    G = C // cpg
    xh = xhat_of(prim, mr, cpg)
    return torch.stack([z.reshape(B, G, -1).mean(2), (xh * z).reshape(B, G, -1).mean(2)], 2)


def tc_of(tst, mr, cpg, by_rstd):
    """the per-channel expansion the kernels write, bit for bit: float32(f) * float32 tst, f = 1 (tangent) or the primal rstd"""
    t = _pc(tst.to(torch.float32).transpose(1, 2), cpg).transpose(1, 2)                     # [B][C][2]
    if not by_rstd:
        return t.contiguous()
    f = _pc(mr[..., 1].to(torch.float32), cpg)                                              # [Bp][C]
    return (f.unsqueeze(-1) * t).contiguous()


def apply(kind, x, sc, sh, cpg, d=None, mr=None, tst=None, base=None, base_scale=1.0, out0=None, act=ACT_SILU, absolute=False):
    """launch_gn_apply, kinds 0 - 5 of kernels.h; out0: the tensor accumulated into"""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    scb, shb = _bc(sc, x), _bc(sh, x)
    y = scb * x + shb
    ya = (scb * x).abs() + shb.abs()
    if kind == 0:
        r = ya if absolute else y
    elif kind == 4:
        r = act_f(y, act).abs() + act_d(y, act).abs() * ya if absolute else act_f(y, act)
    else:
        mean, rstd = _bc(_pc(mr[..., 0], cpg), x), _bc(_pc(mr[..., 1], cpg), x)
        m1, m2 = _bc(_pc(tst[..., 0], cpg), x), _bc(_pc(tst[..., 1], cpg), x)
        xh = (x - mean) * rstd
        ds = act_d(y, act)
        if absolute:
            xh = (x.abs() + mean.abs()) * rstd.abs()
            ds = ds.abs() + act_d2(y, act).abs() * ya
        gm = scb / rstd
        if kind == 1:
            r = ab(scb) * (ab(d) + ab(m1) + ab(xh * m2)) if absolute else scb * (d - m1 - xh * m2)
        elif kind == 5:
            r = ds * ab(scb) * (ab(d) + ab(m1) + ab(xh * m2)) if absolute else ds * scb * (d - m1 - xh * m2)
        else:
            zz = ab(gm) * (ds if kind == 2 else 1.0) * ab(d)
            r = ab(rstd) * (zz + ab(m1) + ab(xh * m2)) if absolute else rstd * (zz - m1 - xh * m2)
            if base is not None:
                r = r + ab(base_scale * base)
    if out0 is not None:
        r = r + ab(out0)
    return r


def tol_apply(kind, x, sc, sh, cpg, act=ACT_SILU, **kw):
    """tau of |out - ref| <= tau A, A = apply(absolute=True): 8 fp32 roundings of the elementwise expression plus the float32-torch
    error of the same expression relative to A (the activation and its derivative in fp32: conv_oracle.prologue_term's reading)"""
    r64 = apply(kind, x, sc, sh, cpg, act=act, **kw)
    f = lambda t: None if t is None else (t.to(torch.float32) if torch.is_tensor(t) else t)
    r32 = apply(kind, f(x), f(sc), f(sh), cpg, act=act, **{k: f(v) for k, v in kw.items()}).to(D)
    A = apply(kind, x, sc, sh, cpg, act=act, absolute=True, **kw)
    pro = float(((r32 - r64).abs() / A.clamp_min(1e-300)).max())
    return MARGIN * (8 * U + pro), A


def records(x, sc, sh, mr, cpg, act=ACT_SILU):
    """launch_gn_cache: [C][HW][2] = {S = sc act'(sc x + sh), xhat}"""
    xb = x.unsqueeze(0)
    S = _bc(sc.unsqueeze(0), xb) * act_d(_bc(sc.unsqueeze(0), xb) * xb + _bc(sh.unsqueeze(0), xb), act)
    return torch.stack([S[0], xhat_of(xb, mr.unsqueeze(0), cpg)[0]], -1)


def ctx_groupnorm(tok, G, gamma, beta, eps):
    """launch_ctx_groupnorm: tok [L][D], statistics per group of D / G channels over all L tokens"""
    L, Dm = tok.shape
    t = tok.reshape(L, G, Dm // G)
    mean = t.mean((0, 2), keepdim=True)
    var = ((t - mean) ** 2).mean((0, 2), keepdim=True)
    return ((t - mean) / torch.sqrt(var + eps)).reshape(L, Dm) * gamma + beta


def tol_records(x, sc, sh, mr, cpg, act=ACT_SILU):
    """(ref, tau) of launch_gn_cache, both [C][H][W][2], |out - ref| <= tau.
    S = sc act'(fma(sc, x, sh)): the float32-torch error of the expression relative to its absolute form
    A_S = |sc| (|act'(y)| + |act''(y)| (|sc x| + |sh|)) (the activation derivative in fp32, as conv_oracle.prologue_term reads it) plus
    4 roundings (the fma, the product, two for a derivative evaluated by another sequence of operations): MARGIN (4 u + e) A_S.
    xhat = (x - mean) rstd on fp32 operands: the difference is rounded once relative to itself, the product once; one more for a
    contracted or reordered form: MARGIN 3 u |xhat|."""
    ref = records(x, sc, sh, mr, cpg, act)
    f = lambda t: t.to(torch.float32)
    r32 = records(f(x), f(sc), f(sh), f(mr), cpg, act).to(D)
    scb, shb = sc.view(-1, 1, 1), sh.view(-1, 1, 1)
    y = scb * x + shb
    A_S = scb.abs() * (act_d(y, act).abs() + act_d2(y, act).abs() * ((scb * x).abs() + shb.abs()))
    e = float(((r32[..., 0] - ref[..., 0]).abs() / A_S.clamp_min(1e-300)).max())
    return ref, torch.stack([MARGIN * (4 * U + e) * A_S, MARGIN * 3 * U * ref[..., 1].abs()], -1) + EPS_ABS


def tol_ctx(tok, G, gamma, beta, eps):
    """(ref, tau) of launch_ctx_groupnorm, [L][D].  The kernel sums mean and variance in double and rounds {mean, rstd} to fp32 (2
    roundings), then forms (tok - mean) rstd gamma + beta in fp32: a difference, two products, a sum (4).  Relative to
    A = (|tok| + |mean|) rstd |gamma| + |beta| that is MARGIN 6 u A; A does not vanish where tok crosses the mean."""
    L, Dm = tok.shape
    cpg = Dm // G
    t = tok.reshape(L, G, cpg)
    mean = t.mean((0, 2), keepdim=True)
    rstd = 1 / torch.sqrt(((t - mean) ** 2).mean((0, 2), keepdim=True) + eps)
    A = ((t.abs() + mean.abs()) * rstd).reshape(L, Dm) * gamma.abs() + beta.abs()
    return ctx_groupnorm(tok, G, gamma, beta, eps), MARGIN * 6 * U * A + EPS_ABS


# ---------------------------------------------------------------------------------------------------------------------------
# row tiles: a conv workgroup finishes NT pixels of a cout row, a block of min(W, 32) columns x NT / min(W, 32) rows

def row_tiles(t, NT):
    """[..., H, W] -> [..., ntile, NT]; the FIRST entry of a tile is its top-left pixel (the epilogue's pivot)"""
    H, W = t.shape[-2:]
    TW = min(W, 32)
    TH = NT // TW
    assert TW * TH == NT and H % TH == 0 and W % TW == 0, (H, W, NT)
    lead = t.shape[:-2]
    v = t.reshape(*lead, H // TH, TH, W // TW, TW).transpose(-3, -2)
    return v.reshape(*lead, (H // TH) * (W // TW), NT)


def partials_fwd(x, NT):
    """{mean, M2} per (b, c, tile)"""
    v = row_tiles(x, NT)
    m = v.mean(-1)
    return torch.stack([m, ((v - m.unsqueeze(-1)) ** 2).sum(-1)], -1)


def partials_tan(d, prim, NT):
    """raw {sum d, sum x d} per (b, c, tile); prim [C][H][W]"""
    v, xv = row_tiles(d, NT), row_tiles(prim, NT).unsqueeze(0)
    return torch.stack([v.sum(-1), (v * xv).sum(-1)], -1)


def partials_cot(g, rec, NT):
    """{sum S g, sum xhat S g} per (b, c, tile); rec [C][H][W][2] = records()"""
    v = row_tiles(g, NT)
    S, xh = row_tiles(rec[..., 0], NT).unsqueeze(0), row_tiles(rec[..., 1], NT).unsqueeze(0)
    return torch.stack([(S * v).sum(-1), (xh * S * v).sum(-1)], -1)


def merge_fwd(parts, HW, G, eps):
    """the group's {mean, rstd} from the row-tile partials of its channels: parts = [(part [B][Ci][nt][2]), ...] along the channels
    (one entry: gn_fused_finalize; two: gn_fused_finalize_cat).  M2 = sum M2_t + sum n_t (mean_t - mean)^2."""
    B = parts[0].shape[0]
    mean_c = torch.cat([p[..., 0].mean(2) for p in parts], 1)                               # tiles of one part are equally sized
    C = mean_c.shape[1]
    cpg = C // G
    mean = mean_c.reshape(B, G, cpg).mean(2)
    mg = _pc(mean, cpg)
    m2_c, off = [], 0
    for p in parts:
        Ci, nt = p.shape[1], p.shape[2]
        dev = (p[..., 0] - mg[:, off:off + Ci].unsqueeze(-1)) ** 2
        m2_c.append(p[..., 1].sum(2) + (HW / nt) * dev.sum(2))
        off += Ci
    var = torch.cat(m2_c, 1).reshape(B, G, cpg).sum(2) / (cpg * HW)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 2)


def merge_lin(kind, parts, HW, G, mr):
    """gn_lin_fused_finalize: tangent raw sums -> {sum d / n, rstd (sum x d - mean sum d) / n}; cotangent sums of S g -> / rstd"""
    s = torch.cat([p.sum(2) for p in parts], 1)                                             # [B][C][2]
    B, C = s.shape[:2]
    n = (C // G) * HW
    s = s.reshape(B, G, C // G, 2).sum(2)
    mean, rstd = mr[..., 0], mr[..., 1]
    if kind == ST_TAN:
        return torch.stack([s[..., 0] / n, rstd * (s[..., 1] - mean * s[..., 0]) / n], 2)
    return s / (n * rstd.unsqueeze(-1))


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances

def chain(nt: int) -> int:
    """length of the route's fp32 summation chain: the float4-then-double kernels (standalone, split-K epilogue) add 4 values in
    fp32 and go on in double; a conv epilogue adds a lane's 4 values and runs a log2(NT / 4)-deep butterfly over the row's lanes"""
    return 4 if nt == 0 else 4 + int(math.log2(max(nt // 4, 1)))


def _per_sample_nt(nt, B, C):
    """nt: 0 / an int (all samples and channels), [B] per sample, or [B][C] -> LongTensor [B][C]; 0 = centred in double"""
    t = torch.as_tensor(nt, dtype=torch.long)
    if t.dim() == 0:
        return t.expand(B, C)
    if t.dim() == 1:
        return t.view(B, 1).expand(B, C)
    return t


def tol_fwd(x, G, gamma, beta, eps, nt=0, ss_scale=None, ss_shift=None) -> Dict[str, torch.Tensor]:
    """Bounds of the forward statistics of x [B][C][H][W] (float64 of the fp32 tensor), per (sample, group) / (sample, channel):
    tau = MARGIN (format + accumulation) A + 1e-30 with u = 2^-24, n = chain(NT) and A the mean absolute SUMMAND OF THE ROUTE.

    mean   standalone / split-K: the sum of x itself, A = mean|x|, and one rounding of the result: MARGIN (u |mean| + n u mean|x|).
           epilogue: row tiles sum d = v - pivot (pivot = the tile's first value), A = mean|v - pivot| -- it does NOT grow with
           the offset -- and {pivot + m} is rounded when stored and again in the result: MARGIN (2 u |mean| + n u mean|v - pivot|).
           Both are within MARGIN (n + 2) u (|mean| + sigma), the scale of the quantity.
    rstd   relative: d rstd / rstd = -1/2 dM2 / M2 (var / (var + eps) <= 1), plus u for the result.
           standalone / split-K: M2 is summed about the (slice) mean, corrected exactly in double: each (x - mean)^2 carries 3
           roundings, the sum n: dM2 / M2 <= (n + 3) u, kappa = 1.
           epilogue: per row tile M2_t = s2 - s1 m, s2 = sum d^2 (3 + n roundings), s1 m = s1^2 / NT <= s2 (2 n + 4), the
           difference (1): |dM2_t| <= (3 n + 8) u s2_t, s2_t = sum (v - pivot_t)^2; over the group that is (3 n + 8) u kappa,
           kappa = sum_t s2_t / M2.  The between-tiles term n_t (mean_t - mean)^2 is formed in double from tile means rounded to
           fp32: + u sum_t n_t 2 |mean_t| |mean_t - mean| / M2 ("between").
    sc     gamma rstd [(1 + scale)]: relative bound of rstd plus 1 (3) roundings.
    sh     beta - mean rstd gamma [(1 + scale) + shift]: the bounds of mean and rstd propagated, plus 4 roundings of
           A = (|beta| + |mean rstd gamma|) |1 + scale| + |shift|."""
    B, C = x.shape[:2]
    cpg = C // G
    HW = x.shape[2] * x.shape[3]
    ntb = _per_sample_nt(nt, B, C)
    mr, sc, sh = fwd_stats(x, G, gamma, beta, eps, ss_scale, ss_shift)
    mean, rstd = mr[..., 0], mr[..., 1]
    t_mean, t_rstd = torch.zeros(B, G, dtype=D), torch.zeros(B, G, dtype=D)
    kap = torch.ones(B, G, dtype=D)
    for b in range(B):
        mg = _pc(mean[b], cpg)
        sq, ab, btw, nch = (torch.zeros(C, dtype=D) for _ in range(4))
        for NT in sorted(set(ntb[b].tolist())):
            ch = (ntb[b] == NT).nonzero().flatten()
            xc = x[b, ch]
            nch[ch] = float(chain(NT))
            if NT == 0:
                sq[ch] = ((xc - mg[ch].view(-1, 1, 1)) ** 2).sum((1, 2))
                ab[ch] = xc.abs().sum((1, 2))
                continue
            v = row_tiles(xc, NT)                                       # [nch][ntile][NT]
            dv = v - v[..., :1]
            sq[ch] = (dv ** 2).sum((1, 2))
            ab[ch] = dv.abs().sum((1, 2))
            mt = v.mean(-1)
            btw[ch] = (NT * 2 * mt.abs() * (mt - mg[ch].view(-1, 1)).abs()).sum(1)
        g_ = lambda t: t.reshape(G, cpg)
        n = g_(nch).max(1).values
        tiled = g_((ntb[b] > 0).to(D)).max(1).values
        M2 = ((x[b].reshape(G, -1) - mean[b].view(-1, 1)) ** 2).sum(1).clamp_min(1e-300)
        kappa = g_(sq).sum(1) / M2
        kap[b] = kappa
        t_mean[b] = MARGIN * ((1 + tiled) * U * mean[b].abs() + n * U * g_(ab).sum(1) / (cpg * HW))
        c_m2 = torch.where(tiled > 0, 3 * n + 8, n + 3)
        t_rstd[b] = MARGIN * (U + 0.5 * (c_m2 * U * kappa + U * g_(btw).sum(1) / M2))
    f = torch.ones(C, dtype=D) if ss_scale is None else 1 + ss_scale
    shift = torch.zeros(C, dtype=D) if ss_shift is None else ss_shift
    k_sc = 1 if ss_scale is None else 3
    t_sc = sc.abs() * (_pc(t_rstd, cpg) + MARGIN * k_sc * U)
    gr = gamma * _pc(rstd, cpg) * f
    A_sh = (beta.abs() + (_pc(mean * rstd, cpg) * gamma).abs()) * f.abs() + shift.abs()
    t_sh = _pc(t_mean, cpg) * gr.abs() + (_pc(mean, cpg) * gr).abs() * _pc(t_rstd, cpg) + MARGIN * 4 * U * A_sh
    return dict(mean=t_mean + EPS_ABS, rstd=t_rstd * rstd + EPS_ABS, sc=t_sc + EPS_ABS, sh=t_sh + EPS_ABS, kappa=kap,
                ref=dict(mr=mr, sc=sc, sh=sh))


def z_error(kind, d, prim, sc, sh, mr, cpg, act):
    """error of the fp32 evaluation of z relative to its absolute form (0 for the tangent kind, whose z is the tensor itself)"""
    if kind == 0:
        return 0.0
    f = lambda t: t.to(torch.float32)
    z32 = z_of(kind, f(d), f(prim), f(sc), f(sh), f(mr), cpg, act).to(D)
    z64 = z_of(kind, d, prim, sc, sh, mr, cpg, act)
    return float(((z32 - z64).abs() / z_of(kind, d, prim, sc, sh, mr, cpg, act, absolute=True).clamp_min(1e-300)).max())


def tol_lin(kind, d, prim, sc, sh, mr, cpg, act=ACT_SILU, nt=0) -> Dict[str, torch.Tensor]:
    """Bounds of {m1, m2} per (sample, group); d [B][C][H][W], the primal and its arrays [1 or B][...]; kind as z_of.
    tau = MARGIN (u |m| + (accumulation + e_z) A) + 1e-30; e_z = z_error (the activation derivative in fp32, conv_oracle.prologue_term).

    m1     A = mean|z| (absolute form): n roundings of the sum; a route through stored fp32 partials rounds once more.
    m2     routes that sum xhat z (standalone, split-K epilogue, cotangent epilogue from {S, xhat} records): A = mean|xhat z|, xhat
           and the product add 3 roundings: (n + 3) u + e_z (+ 1 for the record's S).
           tangent from raw sums (tangent epilogue, kept partials, both cat finalizes): m2 = rstd (sum x d - mean sum d) / n in
           double from fp32 sums {sum d, sum x d}: A = rstd (mean|x d| + |mean| mean|d|), (n + 2) roundings.  THIS A grows with the
           primal's offset (x d does not know the mean); the A of the other routes does not."""
    B, C = d.shape[:2]
    G = C // cpg
    ntb = _per_sample_nt(nt, B, C)
    z = z_of(kind, d, prim, sc, sh, mr, cpg, act)
    za = z_of(kind, d, prim, sc, sh, mr, cpg, act, absolute=True)
    ez = z_error(kind, d, prim, sc, sh, mr, cpg, act)
    ref = lin_stats(z, prim, mr, cpg)
    xh = xhat_of(prim, mr, cpg)
    gmean = lambda t: t.reshape(B, G, -1).mean(2)
    n = torch.tensor([[float(max(chain(int(v)) for v in ntb[b, g * cpg:(g + 1) * cpg])) for g in range(G)] for b in range(B)], dtype=D)
    tiled = (ntb.reshape(B, G, cpg).max(2).values > 0).to(D)
    t1 = MARGIN * ((1 + tiled) * U * ref[..., 0].abs() + (n * U + ez) * gmean(za))
    A_hat = gmean(xh.abs() * za)
    if kind == 0:
        mean, rstd = mr[..., 0].expand(B, G), mr[..., 1].expand(B, G)
        A_raw = rstd * (gmean((prim * d).abs()) + mean.abs() * gmean(d.abs()))
        A2 = torch.where(tiled > 0, A_raw, A_hat)
        acc2 = torch.where(tiled > 0, (n + 2) * U, (n + 3) * U)
    else:
        A2, acc2 = A_hat, (n + 3 + tiled) * U
    t2 = MARGIN * (U * ref[..., 1].abs() + (acc2 + ez) * A2)
    return dict(m1=t1 + EPS_ABS, m2=t2 + EPS_ABS, ref=ref, A2=A2)


def worst(got, ref, tau, names):
    """(ok, share, message): |got - ref| <= tau elementwise, NaN failing; share = max |err| / tau, the message names its index"""
    err = (got.to(D) - ref).abs()
    ratio = err / tau
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    share = float(ratio.max())
    msg = (f"worst {names} = {idx}: got {float(got[idx])!r} ref {float(ref[idx])!r} |err| = {float(err[idx]):.3e} against tau = "
           f"{float(tau[idx]):.3e}; {int((ratio > 1).sum())} of {ratio.numel()} fail")
    return share <= 1.0, share, msg


def check_fwd(got_mr, got_sc, got_sh, tol):
    """[(name, ok, share, message)] of the four forward quantities against tol_fwd's bounds"""
    ref = tol["ref"]
    out = []
    for name, got, r, tau, idx in (("mean", got_mr[..., 0], ref["mr"][..., 0], tol["mean"], "(sample, group)"),
                                   ("rstd", got_mr[..., 1], ref["mr"][..., 1], tol["rstd"], "(sample, group)"),
                                   ("sc", got_sc, ref["sc"], tol["sc"], "(sample, channel)"),
                                   ("sh", got_sh, ref["sh"], tol["sh"], "(sample, channel)")):
        out.append((name,) + worst(got, r, tau, idx))
    return out


def check_lin(got_tst, tol):
    return [(name,) + worst(got_tst[..., i], tol["ref"][..., i], tol[name], "(sample, group)") for i, name in enumerate(("m1", "m2"))]


def tc_mismatch(got_tc, got_tst, mr, cpg, by_rstd) -> int:
    """entries of the GPU's tc that are not float32(f) * its own tst, bit for bit"""
    want = tc_of(got_tst, mr, cpg, by_rstd)
    return int((got_tc.to(torch.float32).view(torch.int32) != want.view(torch.int32)).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the routes (torch float32 on the CPU; sums of 4 and of a row tile in fp32, everything behind them in double,
# as the kernels do).  `plant`: one of the errors of tests/test_stats_oracle_host.py.

F = torch.float32


def _s4(t):
    """fp32 sums of 4 consecutive values -> double"""
    return t.reshape(-1, 4).sum(1, dtype=F).to(D)


def gn_nsplit(length, BG):
    s = max(1, min(64, length // 16384))
    while s > 1 and s * BG > 8192:
        s >>= 1
    return s


def _slices(length, ns):
    per = ((length // 4 + ns - 1) // ns) * 4
    return [(min(s * per, length), min(s * per + per, length)) for s in range(ns)]


def route32_fwd_alone(x, G, eps, plant=None):
    """gn_partial_kernel + gn_finalize_kernel (and the split-K epilogue's ST_FWD): per slice the mean from fp32 sums of 4, M2 about
    the fp32 mean in fp32 squares, corrected in double; Chan's merge of the slices in double"""
    B, C = x.shape[:2]
    cpg = C // G
    x32 = x.to(F).reshape(B, G, -1)
    length = x32.shape[2]
    ns = gn_nsplit(length, B * G)
    out = torch.zeros(B, G, 2, dtype=D)
    for b in range(B):
        for g in range(G):
            n = mean = M2 = 0.0
            for si, (beg, end) in enumerate(_slices(length, ns)):
                if end <= beg or (plant == "tile_left_out" and si == ns - 1 and ns > 1):
                    continue
                v = x32[b, g, beg:end]
                cnt = end - beg
                mu = float(_s4(v).sum()) / cnt
                mf = torch.tensor(mu, dtype=F)
                a = v - mf
                m2 = float(_s4(a * a).sum()) - cnt * (mu - float(mf)) ** 2
                nn, dl = n + cnt, mu - mean
                mean += dl * cnt / nn
                M2 += m2 + (0.0 if plant == "no_between" else dl * dl * n * cnt / nn)
                n = nn
            out[b, g, 0] = float(torch.tensor(mean, dtype=F))
            out[b, g, 1] = float(torch.tensor(1.0 / math.sqrt(M2 / n + eps), dtype=F))
    return out


def part32_fwd(x, NT):
    """the epilogue's {mean, M2} row-tile partials in fp32: sums about the pivot"""
    v = row_tiles(x.to(F), NT)
    piv = v[..., :1]
    dv = v - piv
    s1, s2 = dv.sum(-1, dtype=F), (dv * dv).sum(-1, dtype=F)
    m = s1 * torch.tensor(1.0 / NT, dtype=F)
    return torch.stack([piv[..., 0] + m, s2 - s1 * m], -1)


def route32_fwd_epi(parts, HW, G, eps, plant=None):
    """gn_fused_finalize_kernel / gn_fused_finalize_cat_kernel on fp32 partials (one or two parts along the channels), in double"""
    parts = [p.to(D) for p in parts]
    if plant == "tile_left_out":
        parts = [p.clone() for p in parts]
        parts[-1][:, -1, -1] = 0.0
    if plant == "one_tile_size" and len(parts) == 2:      # both parts weighted with the first part's tile size
        nt0 = parts[0].shape[2]
        B = parts[0].shape[0]
        mean_c = torch.cat([p[..., 0].mean(2) for p in parts], 1)
        C = mean_c.shape[1]
        cpg = C // G
        mean = mean_c.reshape(B, G, cpg).mean(2)
        mg = _pc(mean, cpg)
        m2c, off = [], 0
        for p in parts:
            dev = (p[..., 0] - mg[:, off:off + p.shape[1]].unsqueeze(-1)) ** 2
            m2c.append(p[..., 1].sum(2) + (HW / nt0) * dev.sum(2))
            off += p.shape[1]
        var = torch.cat(m2c, 1).reshape(B, G, cpg).sum(2) / (cpg * HW)
        mr = torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 2)
    elif plant == "no_between":
        mr = merge_fwd(parts, HW, G, eps)
        C = sum(p.shape[1] for p in parts)
        var = torch.cat([p[..., 1].sum(2) for p in parts], 1).reshape(mr.shape[0], G, C // G).sum(2) / ((C // G) * HW)
        mr = torch.stack([mr[..., 0], 1.0 / torch.sqrt(var + eps)], 2)
    else:
        mr = merge_fwd(parts, HW, G, eps)
    return _f32(mr)


def scsh32(mr, gamma, beta, cpg, ss_scale=None, ss_shift=None):
    """sc, sh as the finalize kernels form them in fp32 from the fp32 {mean, rstd}"""
    m, r = _pc(mr[..., 0].to(F), cpg), _pc(mr[..., 1].to(F), cpg)
    gm, bt = gamma.to(F), beta.to(F)
    a, o = gm * r, bt - m * r * gm
    if ss_scale is not None:
        f = 1 + ss_scale.to(F)
        a, o = a * f, o * f + ss_shift.to(F)
    return a.to(D), o.to(D)


def route32_lin_alone(kind, d, prim, sc, sh, mr, cpg, act=ACT_SILU, plant=None):
    """gn_tstats_partial / the split-K epilogue's ST_TAN, ST_COT: z and xhat z in fp32, sums of 4 in fp32, then double"""
    f = lambda t: t.to(F)
    B, C = d.shape[:2]
    G = C // cpg
    mrp = f(mr)
    if plant == "neighbour_group":
        mrp = torch.roll(mrp, 1, dims=-2)
    z = z_of(kind, f(d), f(prim), f(sc), f(sh), mrp, cpg, act)
    xz = xhat_of(f(prim), mrp, cpg) * z
    n = cpg * d.shape[2] * d.shape[3]
    out = torch.zeros(B, G, 2, dtype=D)
    for b in range(B):
        for g in range(G):
            out[b, g, 0] = float(_s4(z[b, g * cpg:(g + 1) * cpg]).sum()) / n
            out[b, g, 1] = float(_s4(xz[b, g * cpg:(g + 1) * cpg]).sum()) / n
    return _f32(out)


def part32_tan(d, prim, NT):
    v, xv = row_tiles(d.to(F), NT), row_tiles(prim.to(F), NT).unsqueeze(0)
    return torch.stack([v.sum(-1, dtype=F), (v * xv).sum(-1, dtype=F)], -1)


def part32_cot(g, prim, sc, sh, mr, cpg, NT, act=ACT_SILU):
    rec = records(prim.to(F), sc.to(F), sh.to(F), mr.to(F), cpg, act)
    v = row_tiles(g.to(F), NT)
    S, xh = row_tiles(rec[..., 0], NT).unsqueeze(0), row_tiles(rec[..., 1], NT).unsqueeze(0)
    z = S * v
    return torch.stack([z.sum(-1, dtype=F), (xh * z).sum(-1, dtype=F)], -1)


def route32_lin_epi(kind, parts, HW, G, mr, plant=None):
    """gn_lin_fused_finalize_kernel on fp32 partials, in double"""
    parts = [p.to(D) for p in parts]
    mrp = _f32(mr)
    if plant == "tile_left_out":
        parts = [p.clone() for p in parts]
        parts[-1][:, -1, -1] = 0.0
    if plant == "neighbour_group":
        mrp = torch.roll(mrp, 1, dims=-2)
    if plant == "no_mean_sum" and kind == ST_TAN:
        s = torch.cat([p.sum(2) for p in parts], 1)
        B, C = s.shape[:2]
        n = (C // G) * HW
        s = s.reshape(B, G, C // G, 2).sum(2)
        return _f32(torch.stack([s[..., 0] / n, mrp[..., 1] * s[..., 1] / n], 2))
    return _f32(merge_lin(kind, parts, HW, G, mrp))


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def norm_operands(C, G, g, ss=False):
    """gamma, beta (and a scale-shift pair) of a norm, exactly representable in float32"""
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    o = dict(gamma=_f32(1.0 + 0.3 * rn(C)), beta=_f32(0.3 * rn(C)))
    if ss:
        o.update(ss_scale=_f32(0.2 * rn(C)), ss_shift=_f32(0.3 * rn(C)))
    return o


def primal_operands(C, H, W, G, gamma, beta, eps, g, level=0.0):
    """a primal [C][H][W] (unit-variance maps, per-channel offsets of a few units; level: |mean| / std of every second group) and
    its float32 statistics arrays sc, sh [C], mr [G][2]"""
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    cpg = C // G
    prim = rn(C, H, W) * (0.5 + torch.rand(C, generator=g, dtype=D)).view(-1, 1, 1) + 3.0 * rn(C).view(-1, 1, 1)
    if level:
        prim = prim + level * _pc((torch.arange(G) % 2 == 0).to(D), cpg).view(-1, 1, 1)
    prim = _f32(prim)
    mr, sc, sh = fwd_stats(prim.unsqueeze(0), G, gamma, beta, eps)
    return dict(prim=prim, mr=_f32(mr[0]), sc=_f32(sc[0]), sh=_f32(sh[0]))


def tensor_operand(B, C, H, W, G, g, level=0.0):
    """seeded, distinct per sample, per-channel offsets of a few units; level: an offset of level x std on every second group"""
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    x = rn(B, C, H, W) * (0.5 + torch.rand(C, generator=g, dtype=D)).view(1, -1, 1, 1) + 3.0 * rn(B, C).view(B, C, 1, 1)
    if level:
        x = x + level * _pc((torch.arange(G) % 2 == 0).to(D), C // G).view(1, -1, 1, 1)
    return _f32(x)


LEVELS = (0.0, 50.0, 1000.0)      # |mean| / std of the affected groups: the regimes of tests/norm_offsets.py


# ---------------------------------------------------------------------------------------------------------------------------
# conv-carried cases: (conv case of conv_oracle, statistics kind, engine) -> the route the planner must name
#
# engine "g32": the CelebA DDPM config (32 groups); "g4": the same with gn_groups = 4 (cpg 32 at 128 couts: group length 32768 at
# 32 x 32, where gn_nsplit returns 2 and the slice merge behind the split-K epilogue runs; cpg 10 for the ragged 40-cout conv).
# routes: the `stats=` word of each launch of the main operator, in order; ntile likewise (0 behind split-K / alone).

GN_GROUPS = {"g32": 32, "g4": 4}
ROWS: List[dict] = []


def _row(family, d, kinds, routes, precs=("bf16x3", "f16"), engine="g32", probes=None, ss=False, keep=False, kernel=None, cot_rides=None,
         stats_all=0, tag=""):
    for kind in kinds:
        rid = f"{co.case_id(d)}{'_ss' if ss else ''}{'_keep' if keep else ''}{tag}-{kind}-{engine}"
        ROWS.append(dict(family=family, case=d, kind=kind, routes=tuple(routes), precs=tuple(precs), engine=engine, probes=probes, ss=ss,
                         keep=keep, kernel=kernel, cot_rides=cot_rides, stats_all=stats_all, id=rid))


def _build():
    case = co.case
    ALLK = ("fwd", "tan", "cot")
    # 1. epilogue, one launch.  (The 1x1 128-cout tile: 128 input channels at 32 x 32, B = 3 are 8 K chunks on 24 workgroups and
    #    split-K by 2 under the planner -- that case is listed with the split-K rows; 112 input channels stay un-split.)
    _row("epi 1x1 tile 0", case(1, 112, 128, 32, B=3), ALLK, ["epi"], kernel="<1,2,2,2,2")
    _row("epi 3x3 tile 5", case(9, 48, 128, 16, B=2), ALLK, ["epi"], kernel="<9,2,4,2,2")
    _row("epi tile 3", case(9, 48, 64, 32, B=1), ALLK, ["epi"], kernel="<9,2,2,1,1")
    _row("epi tap-pair", case(9, 32, 128, 128, B=2), ALLK, ["epi"], precs=("bf16x3",), kernel="conv_pair", probes=(1,))
    _row("epi kcat", case(9, 64, 128, 64, B=4, mode=1, Cin2=32), ("fwd",), ["epi"], kernel="conv_kcat", probes=(0, 3))
    _row("epi polyphase", case(9, 32, 128, 64, B=2, upsample=1), ("tan",), ["epi"], kernel="<4,2,4,2,2", probes=(1,))
    _row("epi scale-shift", case(9, 48, 128, 16, B=2), ("fwd",), ["epi"], ss=True)
    _row("epi finished tensor", case(9, 48, 128, 16, B=2, res=True, bias2=True, accumulate=1), ("fwd",), ["epi"])
    _row("cot next to cot_d", case(1, 64, 128, 64, B=4, cot=True), ("cot",), ["alone"], cot_rides=1, probes=(0, 3))
    # 2. split-K epilogue
    for hw in (8, 16):
        for B in (1, 2):
            _row("split-K", case(9, 512, 128, hw, B=B), ALLK, ["splitk"])
    _row("split-K", case(1, 128, 128, 32, B=3), ALLK, ["splitk"])
    _row("split-K", case(9, 512, 128, 16, B=1, res=True, res_scale=0.7071067811865476), ALLK, ["splitk"])
    _row("split-K", case(9, 512, 128, 8, B=2, accumulate=1), ALLK, ["splitk"])
    _row("split-K slices", case(9, 512, 128, 32, B=1), ALLK, ["splitk"], engine="g4")
    _row("split-K GEMM", case(1, 320, 1280, 16, B=1), ("fwd",), ["splitk"], precs=("bf16x3",), kernel="conv_gemm")
    # 3. tail-probe split: the main launch by epi, the tail by splitk
    _row("tail split", case(1, 128, 128, 64, B=9), ALLK, ["epi", "splitk"], precs=("bf16x3",), probes=(0, 7, 8))
    _row("tail split", case(9, 128, 128, 128, B=5), ALLK, ["epi", "splitk"], precs=("bf16x3",), probes=(3, 4))
    # 4. standalone behind the conv
    _row("alone f32", case(9, 48, 128, 16, B=2), ALLK, ["alone"], precs=("f32",), tag="_f32")
    _row("alone ragged", case(1, 40, 40, 16, B=2), ALLK, ["alone"], precs=("bf16x3",), engine="g4")
    _row("alone GEMM", case(1, 320, 2560, 32, B=5), ("fwd",), ["alone"], precs=("bf16x3",), kernel="conv_gemm", probes=(0, 4))
    _row("alone polyphase fwd", case(9, 32, 128, 64, B=2, upsample=1), ("fwd",), ["alone"], precs=("bf16x3",), probes=(1,))
    # 5. kept partials: two producers of one concatenation with different row tiles (256 and 128 pixels); their kept buffers go
    #    through the cat finalizes (CAT below)
    _row("keep A", case(9, 48, 128, 16, B=2), ("fwd", "tan"), ["epi"], keep=True)
    _row("keep B", case(1, 48, 256, 16, B=2), ("fwd", "tan"), ["epi"], keep=True)


_build()

# the norm over the concatenation [keep A | keep B]: 384 channels in 4 groups of 96 -- group 0 wholly in A, group 1 straddles
# (96 ... 127 from A, 128 ... 191 from B), groups 2 and 3 wholly in B
CAT = dict(C1=128, C=384, G=4, HW=256, ntA=1, ntB=2)


def find_row(family, kind, prec=None):
    return next(r for r in ROWS if r["family"] == family and r["kind"] == kind and (prec is None or prec in r["precs"]))


def plan_line(row, prec):
    """the row as one input line of tests/c/conv_plan_cases.cpp, with its statistics ask"""
    return co.plan_line(row["case"], prec) + f" {KINDS[row['kind']]} 1 {int(row['keep'])}"


def parse_plan(text):
    """(launches, closing) of a plan text; a shortcut that ran first has a plan of its own ahead: the LAST closing line counts"""
    launches, closing = [], None
    for line in text.splitlines():
        rec = dict(f.split("=", 1) for f in line.split(" ") if f)
        rec = {k: (v if k in ("kernel", "stats") else int(v)) for k, v in rec.items()}
        if "launch" in rec:
            launches.append(rec)
        else:
            closing = rec
    return launches, closing


def check_route(launches, closing, row) -> List[str]:
    """the statistics part of a plan against the row: a list of complaints"""
    d = row["case"]
    main = launches
    if d["taps"] == 9:
        main = [p for p in launches if not (p["kernel"].startswith("conv_mfma") and "<1," in p["kernel"])]
    bad = []
    got = tuple(p["stats"] for p in main)
    if got != row["routes"]:
        bad.append(f"routes: planned {got}, the table says {row['routes']}")
    if row["kernel"] and main and row["kernel"] not in main[0]["kernel"]:
        bad.append(f"kernel: planned {main[0]['kernel']}, the table says {row['kernel']}")
    for p in main:
        if (p["stats"] in ("epi", "keep")) != (p["ntile"] > 0):
            bad.append(f"launch {p['launch']}: stats={p['stats']} with ntile={p['ntile']}")
        if p["stats"] == "splitk" and p["nsplit"] < 2:
            bad.append(f"launch {p['launch']}: stats=splitk without split-K")
    if closing is None:
        bad.append("no closing line")
    else:
        if closing["stats_all"] != row["stats_all"]:
            bad.append(f"stats_all: planned {closing['stats_all']}, the table says {row['stats_all']}")
        if (closing["keep_ntile"] > 0) != bool(row["keep"]):
            bad.append(f"keep_ntile: planned {closing['keep_ntile']}, keep = {row['keep']}")
    if row["cot_rides"] is not None and main and main[0]["cot"] != row["cot_rides"]:
        bad.append(f"cot: planned {main[0]['cot']}, the table says {row['cot_rides']}")
    return bad


def nt_of(launches, d, B):
    """per-sample tile pixels of the statistics route ([B], 0 = centred in double) from the plan's main launches"""
    ho, wo = co.out_hw(d)
    main = launches
    if d["taps"] == 9:
        main = [p for p in launches if not (p["kernel"].startswith("conv_mfma") and "<1," in p["kernel"])]
    nt = [0] * B
    for p in main:
        for b in range(p["s0"], p["s0"] + p["B"]):
            nt[b] = (ho * wo) // p["ntile"] if p["ntile"] > 0 else 0
    return nt


# ---------------------------------------------------------------------------------------------------------------------------
# cases of the standalone launchers (loco_debug_norm)

@dataclasses.dataclass(frozen=True)
class NormCase:
    op: str
    C: int
    G: int
    H: int
    W: int
    B: int = 1
    kind: int = 0
    act: int = ACT_SILU
    level: float = 0.0
    ss: bool = False
    ntA: int = 0          # tile PIXELS of part A / part B of the finalize ops
    ntB: int = 0
    C1: int = 0
    base: bool = False
    acc: bool = False
    bcast: bool = True    # primal broadcast over the samples (x_bs = 0, pbs = 0); False: per-sample primal and statistics

    @property
    def id(self):
        s = f"{self.op}_C{self.C}_G{self.G}_{self.H}x{self.W}_B{self.B}_k{self.kind}"
        s += f"_a{self.act}" if self.act else ""
        s += f"_L{int(self.level)}" if self.level else ""
        s += "_ss" if self.ss else ""
        s += f"_nt{self.ntA}" if self.ntA else ""
        s += f"_{self.ntB}_C1{self.C1}" if self.ntB else ""
        s += "_base" if self.base else ""
        s += "_acc" if self.acc else ""
        s += "" if self.bcast else "_persample"
        return s


NORM_CASES: List[NormCase] = []


def _build_norm():
    N = NORM_CASES.append
    # gn_stats / gn_tstats: one slice; two slices (cpg HW = 32768 = 8 x 4096); three ragged slices (C = 98, G = 2, HW = 1024: 50176 per
    # group in slices of 16728, 16728, 16720); cpg 1, 4, 16; B 1 and 3; the offset levels
    shapes = [(32, 32, 8, 8, 1), (32, 8, 16, 16, 3), (64, 4, 16, 16, 1), (16, 2, 64, 64, 1), (16, 2, 64, 64, 3), (98, 2, 32, 32, 1),
              (98, 2, 32, 32, 3)]
    for (C, G, H, W, B) in shapes:
        for level in LEVELS if (C, B) in ((32, 3), (16, 1), (98, 1)) else (0.0,):
            N(NormCase("gn_stats", C, G, H, W, B, level=level))
            for kind in (0, 1, 2):
                N(NormCase("gn_tstats", C, G, H, W, B, kind=kind, level=level))
    N(NormCase("gn_stats", 32, 8, 16, 16, 3, ss=True))
    N(NormCase("gn_tstats", 32, 8, 16, 16, 3, kind=1, act=ACT_GELU))
    N(NormCase("gn_tstats", 16, 2, 64, 64, 1, kind=1, act=ACT_GELU))
    N(NormCase("gn_tstats", 32, 8, 16, 16, 3, kind=1, bcast=False))
    # the finalize ops on synthetic partials: ntile 1 (16 x 16 in one 256-pixel tile), 4 and 16 (32 x 32 in tiles of 256 and 64 pixels);
    # cpg ntile below and above 64, above 1024 for the lin finalize (both loop forms)
    for (C, G, H, W, nt) in ((32, 8, 16, 16, 256), (32, 8, 32, 32, 256), (32, 8, 32, 32, 64), (64, 2, 32, 32, 64), (256, 2, 32, 32, 64)):
        for level in LEVELS if nt == 64 and C == 32 else (0.0,):
            N(NormCase("gn_fused_finalize", C, G, H, W, 3, ntA=nt, level=level))
            N(NormCase("gn_lin_fused_finalize", C, G, H, W, 3, kind=ST_TAN, ntA=nt, level=level))
            N(NormCase("gn_lin_fused_finalize", C, G, H, W, 3, kind=ST_COT, ntA=nt, level=level))
    N(NormCase("gn_fused_finalize", 32, 8, 32, 32, 3, ntA=64, ss=True))
    for level in LEVELS:      # ntA != ntB; C1 = 40 of 96 in 4 groups of 24: group 0 in A, group 1 straddles, groups 2 and 3 in B
        N(NormCase("gn_fused_finalize_cat", 96, 4, 32, 32, 3, ntA=256, ntB=64, C1=40, level=level))
        N(NormCase("gn_lin_fused_finalize", 96, 4, 32, 32, 3, kind=ST_TAN, ntA=256, ntB=64, C1=40, level=level))
    N(NormCase("gn_fused_finalize_cat", 96, 4, 32, 32, 1, ntA=64, ntB=256, C1=40))
    # gn_apply: all six kinds at C = 32, HW = 64 and 1024; base / accumulate; both activations; per-sample statistics
    for (H, W) in ((8, 8), (32, 32)):
        for kind in range(6):
            N(NormCase("gn_apply", 32, 8, H, W, 3, kind=kind))
    for kind in (2, 3):
        N(NormCase("gn_apply", 32, 8, 8, 8, 3, kind=kind, base=True))
        N(NormCase("gn_apply", 32, 8, 32, 32, 3, kind=kind, base=True, acc=True))
    N(NormCase("gn_apply", 32, 8, 8, 8, 3, kind=1, acc=True))
    for kind in (2, 4, 5):
        N(NormCase("gn_apply", 32, 8, 32, 32, 3, kind=kind, act=ACT_GELU))
    for kind in (0, 1, 2):
        N(NormCase("gn_apply", 32, 8, 8, 8, 3, kind=kind, bcast=False))
    N(NormCase("gn_cache", 32, 8, 32, 32))
    N(NormCase("gn_cache", 32, 8, 8, 8, act=ACT_GELU))
    for G in (4, 32):
        N(NormCase("ctx_groupnorm", 64, G, 77, 1))      # L = H = 77 tokens, D = C = 64


_build_norm()
NORM_EPS = 1e-6


def norm_inputs(n: NormCase) -> Dict[str, torch.Tensor]:
    """seeded operands of a NormCase (float64 holding float32 values)"""
    g = torch.Generator().manual_seed(7 + sum(ord(ch) * (i + 1) for i, ch in enumerate(n.id)) % 100003)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    C, G, H, W, B = n.C, n.G, n.H, n.W, n.B
    o = norm_operands(C, G, g, ss=n.ss)
    if n.op == "ctx_groupnorm":
        o["x"] = _f32(rn(H, C) * (0.5 + torch.rand(C, generator=g, dtype=D)) + 3.0 * rn(C))
        return o
    Bp = 1 if n.bcast else B
    prims = [primal_operands(C, H, W, G, o["gamma"], o["beta"], NORM_EPS, g, n.level) for _ in range(Bp)]
    for k in ("prim", "mr", "sc", "sh"):
        o[k] = torch.stack([p[k] for p in prims])                  # [Bp][...]
    o["x"] = tensor_operand(B, C, H, W, G, g, n.level)            # gn_stats / fused_finalize: the tensor; the other ops: d
    o["d"] = _f32(rn(B, C, H, W) + 0.5)
    if n.base:
        o["base"] = _f32(rn(B, C, H, W))
    if n.acc:
        o["out0"] = _f32(rn(B, C, H, W))
    return o
