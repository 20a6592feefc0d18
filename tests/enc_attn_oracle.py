"""Float64 reference of ONE launch of ONE attention kernel of the encoders (loco_debug_enc_attn, include/loco_hip_diag.h), its
componentwise error scale, the tolerance, the operands and the case table of tests/test_gpu_enc_attn_oracle.py, and a float32 host
emulation of the kernels' fixed-order chunked algorithms with planted faults (tests/test_enc_attn_oracle_host.py).

What is restated (the comments in the product that specify the kernels, not their launch code):
  op 0 / 1 / 2  enc_attn_kernel (encoder_kernels.hip, encoder_common.h EncAttnArgs): every query of a group of nk tokens against the keys
                of its own group, score (q scale) . k, op 2 + relh[h][g nk + i][row j] + relw[h][g nk + i][col j] for key j = (row, col)
                of a size x size group; P = softmax, o = P v.  op 1 also keeps m = row max and l = sum exp(score - m).
  op 3          prompt_attn_kernel<true> (textenc.hip): keys j <= i, score q . k * scale.
  op 4          prompt_attn_kernel<false>: keys j < lens[p], score q . k + bias_tab[h][j - i + L - 1], no scale; every query row i < L.
  op 5 / 6      the attention cotangent of clipvis.hip from the kept m, l:  P = exp((q scale) . k - m) / l,  delta_i = <go_i, o_i>,
                dS = P o (go v^T - delta),  dQ = scale dS k,  dK = scale dS^T q,  dV = P^T go.  op 5 writes dQ and delta, op 6 reads the
                caller's delta and writes dK, dV.
  op 7          seg_attn_kernel (clipseg.hip): plain attention over the T tokens of a mask, score (q scale) . k.
  op 8          sd_t2i_kernel (samdec.hip): the NQ <= 8 token rows of a prompt against its T image keys, score (q scale) . k.
  op 9          sd_i2t_kernel: every image token against the NQ token keys, score q . k * scale; columns T ... Tp - 1 become 0.

A case `c` is a plain dict (op, nk, hd, heads, groups, size, NQ, Tp, profile, lens, per_prompt, inplace, ld); `ops` holds float64 CPU
tensors whose values are exactly representable in float32, in ONE logical layout [group][head][channel][token] (statistics
[group][head][1][token]); pack() lays them out as the kernels read them.

    reference(c, ops)      {output name: tensor}, float64, in the logical layout
    magnitude(c, ops)      the same expression with the operands of the LAST products in absolute value: A.  P stays; the
                           score-shaped intermediate of the cotangent enters as P (|go v^T| + |delta|).
    tolerance(c, ops)      tau of |out - ref| <= tau A + 1e-30 per output tensor, from the reference alone
    emulated(c, ops, fault) the kernels' algorithms in float32 torch: chunks of 64 (or 32) with a running max and the rescale of l and o
                           (ops 0 - 2, 8, with the merge of the four waves for op 8), P rebuilt from m, l per chunk (ops 5, 6), plain
                           rows (ops 3, 4, 7, 9); `fault` plants one of FAULTS

tau = MARGIN (accumulation + row), MARGIN = 4 as for the U-Net attention (tests/attn_oracle.py); every kernel is exact fp32, so there
is no format term.
  accumulation   (n + 8) 2^-24, n = the fp32 additions that meet in one output element:
                   forward out (ops 0 - 4, 7, 8):  hd + nk (the score, then the row sum and the sum over keys ride together) + 2 for
                                                   the two table terms of op 2, + 1 for the bias of op 4;   op 9: hd + NQ
                   op 1 statistics:                m: hd;   m + log l: hd + nk
                   op 5:  g_q: 2 hd + nk (the score, go . v, the sum over keys)      delta: hd
                   op 6:  g_k: 2 hd + nk      g_v: hd + nk (P carries its score)
  row            the row operation -- everything before the last product -- evaluated in float32 torch FROM THE float32 OPERANDS
                 against float64, relative to its absolute-value version: the scores (so the fp32 score chain is inside: an absolute
                 score error of order hd 2^-24 sum |q_c| |k_c| is a relative error of P), then softmax, relative to P itself
                 (|out - ref| <= max |dP / P| sum P |v|, which is the A of the forward); for ops 5 and 6 P = exp(s - m) / l from the
                 given m, l and the Jacobian P (go v^T - delta), relative to P (|go v^T| + |delta|).
  The statistics of op 1: the kernel's m is the exact maximum of its own fp32 scores, so |m - max s| <= the largest score error:
  A_m = max_j sum_c |q_c scale| |k_c|, tau_m = MARGIN (hd + 8) 2^-24.  m + log l against the float64 log-sum-exp: the score error
  plus the relative error of l, A_lse = A_m + 1 + max_j |s_j - m| (the relative error of an fp32 exponential grows with its
  argument), under the tau of the output.
No number here is fitted to the kernels.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

MARGIN = 4.0
EPS_ABS = 1e-30
U = 2.0 ** -24
SENTINEL = 0x7FC0BEEF                 # a quiet NaN with a payload: what an untouched output element holds
KC = 64                               # enc_attn_lds.h: keys per chunk; queries per workgroup
QB = 16
FAULTS = ("l_not_rescaled", "o_not_rescaled", "skip_last_chunk", "pad_p1", "rel_swapped", "bias_shift", "causal_strict", "len_inclusive",
          "drop_c64", "no_delta", "dk_no_scale", "merge_no_factor")


def round16(n: int) -> int:
    return (n + 15) // 16 * 16


def case(op, nk, hd, heads, groups, profile="spread", size=0, NQ=0, Tp=0, lens=None, per_prompt=False, inplace=False, ld=None) -> dict:
    cols = nk if op == 8 else Tp if op == 9 else groups * nk
    return dict(op=op, nk=nk, hd=hd, heads=heads, groups=groups, profile=profile, size=size, NQ=NQ, Tp=Tp, lens=list(lens) if lens else None,
                per_prompt=bool(per_prompt), inplace=bool(inplace), ld=round16(cols) if ld is None else ld)


def scale_of(c) -> float:
    """the float32 scale the launch receives (T5, op 4, has none)"""
    return 1.0 if c["op"] == 4 else float(torch.tensor(1.0 / math.sqrt(c["hd"]), dtype=torch.float32))


def _f32(t):
    return t.to(torch.float32).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the thresholds the units state in comments and in their LDS formulas, restated

def _r4(n):
    return (n + 3) // 4 * 4


def enc_attn_lds_bytes(hd, size) -> int:
    """enc_attn_lds.h: K [hd][64] | V [64][hd + 1] | Q [hd][16] | two tables [16][size] | P [4][64][4]"""
    return 4 * (_r4(hd * KC) + _r4(KC * (hd + 1)) + _r4(hd * QB) + _r4(2 * QB * size) + 4 * KC * 4)


def prompt_attn_lds_bytes(hd, L) -> int:
    """textenc.hip: K and V [hd][L] each, P [4][L]"""
    return 4 * (2 * hd * L + 4 * L)


def cot_chunk(c) -> int:
    """clipvis.hip, the comment above the cotangent kernels: a chunk of 64 tokens, 32 for head widths above 95 (dQ) / 88 (dK, dV)"""
    return 32 if c["hd"] > (95 if c["op"] == 5 else 88) else 64


def cot_lds_bytes(hd, kc, tables) -> int:
    """clipvis.hip: two streamed tensors [kc][hd + 1] | two owned ones [hd][16] | `tables` per-wave tables [4][64][4]"""
    return 4 * (2 * _r4(kc * (hd + 1)) + 2 * _r4(hd * QB) + tables * 4 * 64 * 4)


def sd_t2i_lds_bytes(hd) -> int:
    """samdec.hip: Q [8][hd] | per wave V [64][hd + 1], P [64][8], corr [8] | m, l [4][8] each | o [4][8][hd]"""
    return 4 * (_r4(8 * hd) + 4 * (_r4(KC * (hd + 1)) + KC * 8 + 8) + 2 * 4 * 8 + 4 * 8 * hd)


def expected_route(c) -> List[dict]:
    """the route line of the case, from the case alone"""
    op = c["op"]
    if op <= 2:
        return [dict(kernel="enc_attn", bias=int(op == 2), keep=int(op == 1))]
    if op <= 4:
        return [dict(kernel="prompt_attn", causal=int(op == 3))]
    if op <= 6:
        return [dict(kernel="clipvis_attn_cot_q" if op == 5 else "clipvis_attn_cot_kv", chunk=cot_chunk(c))]
    if op == 7:
        return [dict(kernel="seg_attn", hd=c["hd"])]
    return [dict(kernel="sd_t2i" if op == 8 else "sd_i2t")]


def parse_route(text: str) -> List[dict]:
    out = []
    for line in text.splitlines():
        rec = dict(f.split("=", 1) for f in line.split(" "))
        out.append({k: (v if k == "kernel" else int(v)) for k, v in rec.items()})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def _dims(c):
    """(query groups, query tokens, key groups, key tokens) of the logical q and k / v"""
    op, G, nk, NQ = c["op"], c["groups"], c["nk"], c["NQ"]
    if op == 8:
        return G, NQ, (G if c["per_prompt"] else 1), nk
    if op == 9:
        return (G if c["per_prompt"] else 1), nk, G, NQ
    return G, nk, G, nk


def make_operands(c, seed=0) -> Dict[str, torch.Tensor]:
    """Seeded operands, exactly representable in float32; q, k, v [group][head][hd][token] carry per-channel offsets of 0.5, 2 and 3
    units as in attn_oracle.make_operands (they cancel in exact arithmetic and are the hazard in fp32).
      spread     q and k scaled so that the scores have variance about 3 over a row
      late       k_j = (noise + offset) + alpha_j w with w the sign pattern of q's offsets and alpha_j growing linearly with the key
                 index, q = (noise + offset) + w: the key norms grow with j, the scores ramp up by about 30 over a full row, so the row
                 maximum lies in the last chunk and every earlier chunk raises the running maximum (the noise moves a score by about a
                 tenth: less than the ramp's step from the last full chunk to a last chunk of two keys)
    The tables (relh, relw, bias_tab) are standard normal.  go is standard normal.  For ops 5 and 6 o, m, l (and delta for op 6) are
    the float64 forward rounded to float32: what the launch is handed."""
    op, H, hd = c["op"], c["heads"], c["hd"]
    g = torch.Generator().manual_seed(7000 + 101 * (0 if op == 1 else op) + seed)      # op 1 on the operands of op 0: their outs must agree
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Gq, Tq, Gk, Tk = _dims(c)
    s = scale_of(c)
    sgn = lambda: torch.sign(rn(H, hd, 1))
    mag = lambda: 0.75 + 0.5 * torch.rand(H, hd, 1, generator=g, dtype=torch.float64)
    unit = (1.0 / (s * s * hd)) ** 0.25      # 1 for the scaled kernels; T5's unscaled scores take smaller q and k, offsets included
    off_q, off_k, off_v = 0.5 * unit * sgn() * mag(), 2.0 * unit * sgn() * mag(), 3.0 * sgn() * mag()
    if c["profile"] == "late":
        w = torch.sign(off_q)
        w = unit * w
        gain = ((off_q + w) * w).sum(1, keepdim=True)                       # (off_q + w) . w per head
        alpha = 30.0 * torch.arange(Tk, dtype=torch.float64) / max(Tk - 1, 1) / (s * gain)      # [H][1][Tk]
        sig = 1.0 / (16.0 * s * math.sqrt(hd))
        q = sig * rn(Gq, H, hd, Tq) + off_q + w
        k = sig * rn(Gk, H, hd, Tk) + off_k + alpha * w
    else:
        amp = 3.0 ** 0.25 * unit      # var(score) = s^2 hd amp^4 = 3
        q = amp * rn(Gq, H, hd, Tq) + off_q
        k = amp * rn(Gk, H, hd, Tk) + off_k
    v = rn(Gk, H, hd, Tk) + off_v
    ops = dict(q=_f32(q), k=_f32(k), v=_f32(v))
    if op == 2:
        ops.update(relh=_f32(rn(H, Gq * Tq, c["size"])), relw=_f32(rn(H, Gq * Tq, c["size"])))
    if op == 4:
        ops["bias_tab"] = _f32(rn(H, 2 * Tq - 1))
    if op in (5, 6):
        S = scores(c, ops, torch.float64)
        m = S.max(-1).values
        l = torch.exp(S - m.unsqueeze(-1)).sum(-1)
        P = torch.exp(S - m.unsqueeze(-1)) / l.unsqueeze(-1)
        o = _f32(torch.einsum("ghij,ghcj->ghci", P, ops["v"]))
        go = _f32(rn(Gq, H, hd, Tq))
        ops.update(o=o, go=go, m=_f32(m).unsqueeze(2), l=_f32(l).unsqueeze(2))
        if op == 6:
            ops["delta"] = _f32((go * o).sum(2, keepdim=True))
    return ops


def scores(c, ops, dt, fault=None, q=None, k=None) -> torch.Tensor:
    """S [group][head][query][key] in dtype dt, dead keys at -inf, by the arithmetic the kernel's comment states"""
    op, s = c["op"], scale_of(c)
    q = (ops["q"] if q is None else q).to(dt)
    k = (ops["k"] if k is None else k).to(dt)
    if fault == "drop_c64":
        q = q[:, :, :64]
        k = k[:, :, :64]
    sc = torch.tensor(s, dtype=dt)
    if op in (3, 9):
        S = torch.einsum("ghci,ghcj->ghij", q, k) * sc
    elif op == 4:
        S = torch.einsum("ghci,ghcj->ghij", q, k)
    else:
        S = torch.einsum("ghci,ghcj->ghij", q * sc, k)
    Tq, Tk = S.shape[-2:]
    i, j = torch.arange(Tq).unsqueeze(1), torch.arange(Tk).unsqueeze(0)
    if op == 2:
        size, G, H = c["size"], c["groups"], c["heads"]
        relh, relw = ops["relh"].to(dt).reshape(H, G, Tq, size), ops["relw"].to(dt).reshape(H, G, Tq, size)
        if fault == "rel_swapped":
            relh, relw = relw, relh
        row, col = torch.arange(Tk) // size, torch.arange(Tk) % size
        S = S + relh[..., row].permute(1, 0, 2, 3) + relw[..., col].permute(1, 0, 2, 3)
    if op == 3:
        dead = (j >= i) if fault == "causal_strict" else (j > i)
        S = S.masked_fill(dead, -math.inf)
    if op == 4:
        L = Tq
        idx = j - i + L - 1 + (1 if fault == "bias_shift" else 0)
        S = S + ops["bias_tab"].to(dt)[:, idx.clamp(0, 2 * L - 2)].unsqueeze(0)
        lens = torch.tensor(c["lens"]).reshape(-1, 1, 1, 1) + (1 if fault == "len_inclusive" else 0)
        S = S.masked_fill(j.reshape(1, 1, 1, Tk) >= lens, -math.inf)
    return S


# ---------------------------------------------------------------------------------------------------------------------------
# reference and error scale

def _eval(c, ops, absolute) -> Dict[str, torch.Tensor]:
    op = c["op"]
    x = (lambda t: t.abs()) if absolute else (lambda t: t)
    S = scores(c, ops, torch.float64)
    if op in (5, 6):
        s = scale_of(c)
        P = torch.exp(S - ops["m"].squeeze(2).unsqueeze(-1)) / ops["l"].squeeze(2).unsqueeze(-1)
        go, q, k, v = ops["go"], ops["q"], ops["k"], ops["v"]
        gP = torch.einsum("ghci,ghcj->ghij", go, v)
        delta = (x(go) * x(ops["o"])).sum(2, keepdim=True) if op == 5 else ops["delta"]      # [g][h][1][i]
        d_row = ((go * ops["o"]).sum(2, keepdim=True) if op == 5 else ops["delta"]).squeeze(2).unsqueeze(-1)
        dS = P * (gP.abs() + d_row.abs()) if absolute else P * (gP - d_row)
        if op == 5:
            return dict(gq=s * torch.einsum("ghij,ghcj->ghci", dS, x(k)), delta=delta)
        return dict(gk=s * torch.einsum("ghij,ghci->ghcj", dS, x(q)), gv=torch.einsum("ghij,ghci->ghcj", P, x(go)))
    m = S.max(-1, keepdim=True).values
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / l
    out = dict(out=torch.einsum("ghij,ghcj->ghci", P, x(ops["v"])))
    if op == 1:
        if absolute:
            Am = torch.einsum("ghci,ghcj->ghij", (ops["q"] * scale_of(c)).abs(), ops["k"].abs()).max(-1).values.unsqueeze(2)
            out.update(m=Am, lse=Am + 1.0 + (S - m).abs().max(-1).values.unsqueeze(2))
        else:
            out.update(m=m.squeeze(-1).unsqueeze(2), lse=(m + torch.log(l)).squeeze(-1).unsqueeze(2))
    return out


def reference(c, ops):
    return _eval(c, ops, False)


def magnitude(c, ops):
    return _eval(c, ops, True)


def additions(c) -> Dict[str, int]:
    op, hd, nk = c["op"], c["hd"], c["nk"]
    if op == 5:
        return dict(gq=2 * hd + nk, delta=hd)
    if op == 6:
        return dict(gk=2 * hd + nk, gv=hd + nk)
    if op == 9:
        return dict(out=hd + c["NQ"])
    n = dict(out=hd + nk + (2 if op == 2 else 1 if op == 4 else 0))
    if op == 1:
        n.update(m=hd, lse=hd + nk)
    return n


def row_term(c, ops) -> float:
    """the row operation in float32 torch from the float32 operands against float64, relative to its absolute-value version"""
    op = c["op"]
    S64, S32 = scores(c, ops, torch.float64), scores(c, ops, torch.float32)
    if op in (5, 6):
        m, l = ops["m"].squeeze(2).unsqueeze(-1), ops["l"].squeeze(2).unsqueeze(-1)
        go, v = ops["go"], ops["v"]
        d = ((go * ops["o"]).sum(2, keepdim=True) if op == 5 else ops["delta"]).squeeze(2).unsqueeze(-1)
        P64 = torch.exp(S64 - m) / l
        gP64 = torch.einsum("ghci,ghcj->ghij", go, v)
        f = lambda t: t.to(torch.float32)
        P32 = torch.exp(S32 - f(m)) * (1.0 / f(l))
        d32 = (f(go) * f(ops["o"])).sum(2).unsqueeze(-1) if op == 5 else f(d)
        j32 = (P32 * (torch.einsum("ghci,ghcj->ghij", f(go), f(v)) - d32)).to(torch.float64)
        j64 = P64 * (gP64 - d)
        jabs = P64 * (gP64.abs() + d.abs())
        keep = jabs > 0
        rel_j = float(((j32 - j64).abs()[keep] / jabs[keep]).max())
        rel_p = float(((P32.to(torch.float64) - P64).abs() / P64.clamp_min(1e-300)).max())      # g_v takes P itself
        return max(rel_j, rel_p)
    P64 = torch.softmax(S64, -1)
    P32 = torch.softmax(S32, -1).to(torch.float64)
    keep = P64 > 0
    return float(((P32 - P64).abs()[keep] / P64[keep]).max())


def tolerance(c, ops) -> Dict[str, dict]:
    """per output tensor: dict(accumulation, row, tau)"""
    row = row_term(c, ops)
    out = {}
    for name, n in additions(c).items():
        acc = (n + 8) * U
        r = 0.0 if name in ("m", "delta") else row      # m and delta are sums of products: no row operation before them
        out[name] = dict(accumulation=acc, row=r, tau=MARGIN * (acc + r))
    return out


def worst(name, out, ref, A, tau):
    """(ok, message, max |out - ref| / A): |out - ref| <= tau A + EPS_ABS on every element of a logical tensor [group][head][channel]
    [token], NaN counting as a failure; the message names the worst element"""
    err = (out.to(torch.float64) - ref).abs()
    ratio = err / (tau * A + EPS_ABS)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    bad = int((ratio > 1).sum())
    a = float(A[idx])
    msg = (f"worst element of {name}: group %d head %d channel %d token %d: out {float(out[idx])!r} ref {float(ref[idx])!r} |err| / A = "
           f"{float(err[idx]) / a if a > 0 else float('inf'):.3e} against tau = {tau:.3e}; {bad} of {ratio.numel()} elements fail") % idx
    keep = A > 0
    measured = float((err[keep] / A[keep]).nan_to_num(nan=float("inf")).max())
    if bool((err[~keep] > EPS_ABS).any()) or bool(torch.isnan(err).any()):
        measured = float("inf")
    return bad == 0, msg, measured


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' layouts

def _cm(X, ld, fill):
    """logical [G][H][hd][T] -> channel-major [H hd][ld], group g at columns g T + [0, T); `fill` [H hd][ld] supplies the rest"""
    G, H, hd, T = X.shape
    buf = fill.clone()
    buf[:, :G * T] = X.permute(1, 2, 0, 3).reshape(H * hd, G * T).to(buf.dtype)
    return buf


def _uncm(buf, G, H, hd, T):
    return buf[:, :G * T].reshape(H, hd, G, T).permute(2, 0, 1, 3)


def _tm(X, fill):
    """logical [P][H][hd][NQ] -> token-major [P][8][H hd], rows NQ ... 7 from `fill`"""
    P, H, hd, NQ = X.shape
    buf = fill.clone()
    buf[:, :NQ] = X.permute(0, 3, 1, 2).reshape(P, NQ, H * hd).to(buf.dtype)
    return buf


def _untm(buf, H, hd, NQ):
    P = buf.shape[0]
    return buf[:, :NQ].reshape(P, NQ, H, hd).permute(0, 2, 3, 1)


def sentinel(*shape) -> torch.Tensor:
    return torch.full(shape, SENTINEL, dtype=torch.int32).view(torch.float32)


def pack(c, ops, seed=0) -> Dict[str, torch.Tensor]:
    """the launch's INPUT tensors (float32 CPU, lens int32) as the kernel reads them; the columns beyond the groups hold finite noise
    (l: positive), the token rows NQ ... 7 of ops 8 and 9 NaN: neither is read"""
    op, H, hd, G, nk, ld = c["op"], c["heads"], c["hd"], c["groups"], c["nk"], c["ld"]
    D = H * hd
    g = torch.Generator().manual_seed(9000 + seed)
    noise = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    t = {}
    if op <= 7:
        t["qkv"] = torch.cat([_cm(ops[n], ld, noise(D, ld)) for n in ("q", "k", "v")], 0)
    if op == 2:
        t.update(relh=ops["relh"].to(torch.float32).contiguous(), relw=ops["relw"].to(torch.float32).contiguous())
    if op == 4:
        t.update(bias_tab=ops["bias_tab"].to(torch.float32).contiguous(), lens=torch.tensor(c["lens"], dtype=torch.int32))
    if op in (5, 6):
        t["go"] = _cm(ops["go"], ld, noise(D, ld))
        t["ml"] = torch.cat([_cm(ops["m"], ld, noise(H, ld)), _cm(ops["l"], ld, 1.0 + noise(H, ld).abs())], 0)
        if op == 5:
            t["o"] = _cm(ops["o"], ld, noise(D, ld))
        else:
            t["delta"] = _cm(ops["delta"], ld, noise(H, ld))
    if op == 8:
        t["q"] = _tm(ops["q"], torch.full((G, 8, D), float("nan")))
        for n in ("k", "v"):
            t[n] = torch.stack([_cm(ops[n][p:p + 1], ld, noise(D, ld)) for p in range(ops[n].shape[0])])
    if op == 9:
        t["q"] = torch.stack([_cm(ops["q"][p:p + 1], ld, noise(D, ld)) for p in range(ops["q"].shape[0])])
        for n in ("k", "v"):
            t[n] = _tm(ops[n], torch.full((G, 8, D), float("nan")))
    return t


def out_shapes(c) -> Dict[str, tuple]:
    """the launch's OUTPUT buffers"""
    op, D, H, G, ld = c["op"], c["heads"] * c["hd"], c["heads"], c["groups"], c["ld"]
    if op == 1:
        return dict(out=(D, ld), ml=(2 * H, ld))
    if op == 5:
        return dict(gqkv=(3 * D, ld), delta=(H, ld))
    if op == 6:
        return dict(gqkv=(3 * D, ld))
    if op == 8:
        return dict(out=(G, 8, D))
    if op == 9:
        return dict(out=(G, D, ld))
    return dict(out=(D, ld))


def unpack(c, bufs) -> (Dict[str, torch.Tensor], int, int):
    """(the logical outputs of the launch's buffers, the count of assigned elements that still hold the sentinel, the count of
    elements outside the contract that lost it).  Columns T ... Tp - 1 of op 9 are assigned: they come back as `zeros`."""
    op, H, hd, G, nk, NQ = c["op"], c["heads"], c["hd"], c["groups"], c["nk"], c["NQ"]
    D = H * hd
    got, assigned = {}, {}
    mask = lambda name: torch.zeros(bufs[name].shape, dtype=torch.bool)
    if op <= 7 and op not in (5, 6):
        got["out"] = _uncm(bufs["out"], G, H, hd, nk)
        a = mask("out")
        a[:, :G * nk] = True
        assigned["out"] = a
        if op == 1:
            got["m"] = _uncm(bufs["ml"][:H], G, H, 1, nk)
            got["l"] = _uncm(bufs["ml"][H:], G, H, 1, nk)
            a = mask("ml")
            a[:, :G * nk] = True
            assigned["ml"] = a
    elif op in (5, 6):
        a = mask("gqkv")
        if op == 5:
            got["gq"] = _uncm(bufs["gqkv"][:D], G, H, hd, nk)
            got["delta"] = _uncm(bufs["delta"], G, H, 1, nk)
            a[:D, :G * nk] = True
            d = mask("delta")
            d[:, :G * nk] = True
            assigned["delta"] = d
        else:
            got["gk"] = _uncm(bufs["gqkv"][D:2 * D], G, H, hd, nk)
            got["gv"] = _uncm(bufs["gqkv"][2 * D:], G, H, hd, nk)
            a[D:, :G * nk] = True
        assigned["gqkv"] = a
    elif op == 8:
        got["out"] = _untm(bufs["out"], H, hd, NQ)
        a = mask("out")
        a[:, :NQ] = True
        assigned["out"] = a
    else:
        got["out"] = torch.stack([_uncm(bufs["out"][p], 1, H, hd, nk)[0] for p in range(G)])
        got["zeros"] = bufs["out"][:, :, nk:c["Tp"]]
        a = mask("out")
        a[:, :, :c["Tp"]] = True
        assigned["out"] = a
    unwritten = outside = 0
    if not c["inplace"]:
        for name, a in assigned.items():
            held = bufs[name].view(torch.int32) == SENTINEL
            unwritten += int((held & a).sum())
            outside += int((~held & ~a).sum())
    return got, unwritten, outside


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' algorithms, with planted faults

def _f(t):
    return t.to(torch.float32)


def _stream(S, v, fault, chunk=KC, start=0, step=1):
    """the running max / sum / output of the chunks start, start + step, ... of the keys: S [..][Tq][Tk] float32 with dead keys at
    -inf, v [..][hd][Tk]; returns (m, l, o [..][Tq][hd]) unnormalised"""
    Tk = S.shape[-1]
    m = torch.full(S.shape[:-1], -math.inf, dtype=torch.float32)
    l = torch.zeros(S.shape[:-1], dtype=torch.float32)
    o = torch.zeros(*S.shape[:-1], v.shape[-2], dtype=torch.float32)
    nchunk = (Tk + chunk - 1) // chunk
    for ch in range(start, nchunk, step):
        k0, k1 = ch * chunk, min((ch + 1) * chunk, Tk)
        if fault == "skip_last_chunk" and k1 - k0 < chunk and ch == nchunk - 1:
            continue
        Sc = S[..., k0:k1]
        mn = torch.maximum(m, Sc.max(-1).values)
        corr = torch.exp(m - mn)
        p = torch.exp(Sc - mn.unsqueeze(-1))
        psum = p.sum(-1)
        if fault == "pad_p1":
            psum = psum + float(chunk - (k1 - k0))
        l = (l if fault == "l_not_rescaled" else l * corr) + psum
        o = (o if fault == "o_not_rescaled" else o * corr.unsqueeze(-1)) + torch.einsum("...ij,...cj->...ic", p, v[..., k0:k1])
        m = mn
    return m, l, o


def emulated(c, ops, fault: Optional[str] = None) -> Dict[str, torch.Tensor]:
    op, s = c["op"], torch.tensor(scale_of(c), dtype=torch.float32)
    q, k, v = _f(ops["q"]), _f(ops["k"]), _f(ops["v"])
    S = scores(c, ops, torch.float32, fault)
    if op in (5, 6):
        kc = cot_chunk(c)
        m, il = _f(ops["m"]).squeeze(2).unsqueeze(-1), (1.0 / _f(ops["l"])).squeeze(2).unsqueeze(-1)
        go, o = _f(ops["go"]), _f(ops["o"])
        d = (go * o).sum(2).unsqueeze(-1) if op == 5 else _f(ops["delta"]).squeeze(2).unsqueeze(-1)
        go_, v_ = (go[:, :, :64], v[:, :, :64]) if fault == "drop_c64" else (go, v)
        gP = torch.einsum("ghci,ghcj->ghij", go_, v_)
        P = torch.exp(S - m) * il
        dS = P * (gP if fault == "no_delta" else gP - d)
        T = S.shape[-1]
        if op == 5:
            acc = torch.zeros_like(q)
            for k0 in range(0, T, kc):
                acc = acc + torch.einsum("ghij,ghcj->ghci", dS[..., k0:k0 + kc], k[..., k0:k0 + kc])
            return dict(gq=acc * s, delta=(go * o).sum(2, keepdim=True))
        gk, gv = torch.zeros_like(k), torch.zeros_like(v)
        qs = q if fault == "dk_no_scale" else q * s
        for i0 in range(0, T, kc):
            gk = gk + torch.einsum("ghij,ghci->ghcj", dS[..., i0:i0 + kc, :], qs[..., i0:i0 + kc])
            gv = gv + torch.einsum("ghij,ghci->ghcj", P[..., i0:i0 + kc, :], go[..., i0:i0 + kc])
        return dict(gk=gk, gv=gv)
    if op <= 2:
        m, l, o = _stream(S, v, fault)
        out = dict(out=(o * (1.0 / l).unsqueeze(-1)).transpose(-1, -2))
        if op == 1:
            out.update(m=m.unsqueeze(2), lse=(m.to(torch.float64) + torch.log(l.to(torch.float64))).unsqueeze(2))
        return out
    if op == 8:
        parts = [_stream(S, v, fault, start=w, step=4) for w in range(4)]
        M = torch.stack([p[0] for p in parts])
        mx = M.max(0).values
        f = torch.ones_like(M) if fault == "merge_no_factor" else torch.exp(M - mx)
        num = sum(f[w].unsqueeze(-1) * parts[w][2] for w in range(4))
        den = sum(f[w] * parts[w][1] for w in range(4))
        return dict(out=(num / den.unsqueeze(-1)).transpose(-1, -2))
    m = S.max(-1, keepdim=True).values
    e = torch.exp(S - m)
    l = e.sum(-1, keepdim=True)
    if op == 7:
        return dict(out=torch.einsum("ghij,ghcj->ghci", e, v) / l.transpose(-1, -2))
    if op == 9:
        return dict(out=torch.einsum("ghij,ghcj->ghci", e, v) * (1.0 / l).transpose(-1, -2))
    return dict(out=torch.einsum("ghij,ghcj->ghci", e * (1.0 / l), v))


# ---------------------------------------------------------------------------------------------------------------------------
# the case table

def _row(rid, family, c, refused=None, null=None, twin=None):
    return dict(id=rid, family=family, case=c, refused=refused, null=null, twin=twin)


def _build_table():
    R = []

    def add(prefix, family, op, shapes, both=lambda nk: nk > 64, late_only=(), **kw):
        for sh in shapes:
            name = prefix + "_" + "x".join(str(x) for x in sh["id"])
            args = {k: v for k, v in sh.items() if k != "id"}
            profs = ("late",) if sh["id"] in late_only else (("spread", "late") if both(args["nk"]) else ("spread",))
            for prof in profs:
                R.append(_row(f"{name}_{prof}", family, case(op, profile=prof, **args, **kw)))

    fwd = [dict(id=(nk, hd, h, g), nk=nk, hd=hd, heads=h, groups=g)
           for nk, hd, h, g in ((17, 16, 2, 3), (64, 64, 1, 1), (82, 80, 2, 2), (130, 8, 1, 1), (33, 5, 3, 1), (70, 106, 1, 1))]
    # (70, 106): the widest head whose carve-up passes the 64 KiB refusal (hd = 128 takes 78080 bytes: a refused row below)
    add("plain", "enc_attn", 0, fwd)
    add("keep", "enc_attn keep", 1, fwd)
    for r in R:
        if r["case"]["op"] == 1:
            r["twin"] = r["id"].replace("keep_", "plain_")      # the out of op 1 must equal the out of op 0 bit for bit
    add("bias", "enc_attn bias", 2, [dict(id=(sz, hd, h, g), nk=sz * sz, size=sz, hd=hd, heads=h, groups=g)
                                     for sz, hd, h, g in ((3, 16, 2, 4), (4, 32, 2, 9), (10, 80, 2, 1), (14, 32, 1, 2))])
    txt = ((7, 16, 2, 3), (65, 32, 1, 2), (77, 64, 2, 2), (128, 32, 2, 1), (77, 80, 1, 1))
    add("causal", "prompt_attn causal", 3, [dict(id=s, nk=s[0], hd=s[1], heads=s[2], groups=s[3]) for s in txt])
    lens = {7: (1, 6, 7), 65: (64, 65), (77, 64): (63, 76), 128: (128,), (77, 80): (2,)}      # 1, 2, 63, 64, 65, L - 1, L
    add("t5", "prompt_attn bias", 4, [dict(id=s, nk=s[0], hd=s[1], heads=s[2], groups=s[3], lens=lens.get(s[0]) or lens[s[:2]]) for s in txt])
    cot = ((17, 16, 2, 2), (82, 80, 2, 2), (82, 92, 1, 2), (82, 96, 1, 1), (50, 106, 1, 2))
    for op, pre, fam in ((5, "cotq", "clipvis cot q"), (6, "cotkv", "clipvis cot kv")):
        add(pre, fam, op, [dict(id=s, nk=s[0], hd=s[1], heads=s[2], groups=s[3]) for s in cot])
    add("seg", "seg_attn", 7, [dict(id=s, nk=s[0], hd=s[1], heads=s[2], groups=s[3])
                               for s in ((10, 4, 2, 3), (37, 8, 2, 2), (82, 16, 4, 2), (65, 32, 1, 1), (130, 64, 1, 2))])
    # (400, 32): the issue's hd = 64 takes 85376 bytes of LDS, which loco_samdec_create refuses; 32 is the widest head the kernel
    # can be launched with (a refused row below pins the 64)
    t2i = ((36, 16, 2, 2, 7), (196, 32, 2, 3, 8), (400, 32, 1, 1, 5), (64, 4, 2, 1, 1))
    for pp in (False, True):
        add("t2i" + ("_kbs" if pp else ""), "sd_t2i", 8, [dict(id=s, nk=s[0], hd=s[1], heads=s[2], groups=s[3], NQ=s[4]) for s in t2i],
            late_only=((400, 32, 1, 1, 5),), per_prompt=pp)
    i2t = ((36, 48, 16, 2, 2, 7), (300, 304, 32, 1, 1, 8), (64, 64, 8, 2, 3, 1))
    for pp in (False, True):
        add("i2t" + ("_qbs" if pp else ""), "sd_i2t", 9, [dict(id=s, nk=s[0], Tp=s[1], hd=s[2], heads=s[3], groups=s[4], NQ=s[5]) for s in i2t],
            both=lambda nk: False, per_prompt=pp)
    R.append(_row("i2t_inplace", "sd_i2t", case(9, 36, 16, 2, 1, Tp=48, NQ=7, inplace=True)))

    ref = lambda rid, c, msg, **kw: R.append(_row("refused_" + rid, "refused", c, refused=msg, **kw))
    ref("null", case(0, 17, 16, 2, 3), "a required operand is null", null="qkv")
    ref("dims", case(0, 17, 16, 2, 0, ld=64), "must be positive")
    ref("relh_ml", dict(case(2, 9, 16, 2, 4, size=3), with_ml=True), "relh together with ml is not built")
    ref("hd130", case(0, 17, 130, 1, 1), "hd > 128")
    ref("lds_enc", case(0, 70, 128, 1, 1), "the LDS carve-up exceeds 65536 bytes")
    ref("lds_prompt", case(3, 128, 64, 1, 1), "the LDS carve-up exceeds 65536 bytes")
    ref("lds_t2i", case(8, 64, 64, 1, 1, NQ=5), "the LDS carve-up exceeds 65536 bytes")
    ref("L129", case(3, 129, 16, 1, 1), "L > 128")
    ref("lens0", case(4, 7, 16, 2, 3, lens=(1, 0, 7)), "lens[1] = 0 outside [1, L]")
    ref("lens8", case(4, 7, 16, 2, 3, lens=(1, 6, 8)), "lens[2] = 8 outside [1, L]")
    ref("seg_hd12", case(7, 10, 12, 2, 1), "head width")
    ref("seg_T2049", case(7, 2049, 4, 1, 1), "T > 2048")
    ref("t2i_hd24", case(8, 36, 24, 2, 1, NQ=7), "hd must be a power of two <= 64")
    ref("i2t_nq9", case(9, 36, 16, 2, 1, Tp=48, NQ=9), "NQ outside [1, 8]")
    ref("ld", case(0, 17, 16, 2, 3, ld=48), "ld is smaller than the columns addressed")
    return R


ROWS = _build_table()
