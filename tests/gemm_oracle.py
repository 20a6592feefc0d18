"""Float64 reference of ONE call of ONE strided batched GEMM launcher (loco_debug_gemm, include/loco_hip_diag.h), its componentwise
error scale, the error the split-bf16 number format alone causes, the launchers' routing rules restated, the operands and the case
table of tests/test_gpu_gemm_oracle.py.

What a launcher computes (kernels.h GemmArgs; the epilogue order is that of every kernel of gemm.hip):

    out(b, h, m, n) = act( alpha (A B + A2 B2) + beta C0 + bias[m] + colbias[n] + R )

over strided views: every operand lives in a wider flat buffer and is addressed through (row, column, batch, head) strides in floats.
A2 / B2 share the row, k and head strides of A / B and have batch strides of their own; R shares C's row, column and head strides
and has its own batch stride; R may BE C (the encoders' in-place residual h = W f + b + h).

A problem `p` is a plain dict (problem(...) below); `ops` holds one flat float64 CPU buffer per operand whose values are exactly
representable in float32 (make_operands).  A case is dict(id, family, op, act, probs = [p] or [p0, p1] for the pair, expect).

    reference(case, ops)        [out per problem], float64, shape [batch][heads][M][N]
    magnitude(case, ops)        the same expression with every operand and term in absolute value, BEFORE the activation: A
    emulated(case, ops)         both operands of every product split into bf16 hi + lo, the lo lo product dropped (ops 2 and 3)
    kernel_emulation(...)       what a fault-free kernel (or one with a planted fault) would return: float32 arithmetic in the
                                kernels' order -- K in chunks, alpha, beta, bias, colbias, R, activation (tests/test_gemm_oracle_host.py)
    route_of(case)              the launch lines loco_debug_gemm must report, from the routing rules RESTATED here
    tolerance(case, ops, ...)   tau of |out - ref| <= tau A_out + 1e-30 per problem, from the reference alone

tau = MARGIN (format + accumulation + activation), MARGIN = 4 as for the convolutions and the attention passes:
  format         max |emulated - reference| / A   (0 on the exact-fp32 ops 0, 1, 4)
  accumulation   (n + 8) 2^-24, n = the fp32 additions that meet in one output element: nseg K, plus ksplit where the K range is
                 split over workgroups (the reduce pass), plus one per epilogue term present (beta C0, bias, colbias, R)
  activation     A_out = Lip A with Lip the activation's Lipschitz constant (found numerically in float64: LIP), and the term is the
                 float32-torch evaluation of the activation on the float32-rounded pre-activation reference against float64,
                 relative to A_out (as conv_oracle.prologue_term)
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

MARGIN = 4.0
EPS_ABS = 1e-30
GUARD = 256                                   # floats of guard band on both sides of every output buffer
OPS = ("gemm", "gemm_fixed", "gemm_bf16x3", "gemm_rec", "gemm_pair")      # loco_gemm_desc.op 0 ... 4
ACTS = ("none", "quick_gelu", "gelu")
SENTINEL_BITS = 0x7FC5A5A5                    # a NaN no kernel produces: what an output float holds before the launch


# ---------------------------------------------------------------------------------------------------------------------------
# problems and their strided views

def _layout(order: str, sizes: Dict[str, int], pitch: Optional[Dict[str, int]]):
    """dense strides of the axes of `order` (outermost first) over their allocated sizes (`pitch` overrides a size); an axis that
    is not named has stride 0 (an operand shared by the batch or by the heads)"""
    alloc = dict(sizes)
    alloc.update(pitch or {})
    st, run = {}, 1
    for ax in reversed(order):
        assert alloc[ax] >= sizes[ax]
        st[ax] = run
        run *= alloc[ax]
    return {ax: st.get(ax, 0) for ax in "bhmkn" if ax in sizes}


def problem(M, N, K, batch=1, heads=1, A="bhmk", B="bhnk", C="bhmn", pitchA=None, pitchB=None, pitchC=None, offA=0, offB=0,
            seg2=None, bias=False, colbias=None, R=None, alpha=1.0, beta=0.0) -> dict:
    """A / B / C: axis order of the operand's buffer, outermost first ("bhmk": k contiguous; "bhkm": m contiguous; no "b": shared by
    the batch).  offA / offB: floats between the (256-byte aligned) buffer and the operand's base.  seg2: None or a pair of "own" /
    "bcast" for A2 and B2 (own: a batch stride 16 floats longer than the first segment's; bcast: batch stride 0).  colbias: None,
    "plain" or "mask" (ordinary values plus a few -1e30 columns).  R: None, "own" (batch stride 64 floats longer than C's) or
    "alias" (R is C, in place)."""
    p = dict(M=M, N=N, K=K, batch=batch, heads=heads, alpha=float(alpha), beta=float(beta), bias=bool(bias), colbias=colbias, R=R,
             seg2=seg2, offA=offA, offB=offB)
    a = _layout(A, dict(b=batch, h=heads, m=M, k=K), pitchA)
    b = _layout(B, dict(b=batch, h=heads, k=K, n=N), pitchB)
    c = _layout(C, dict(b=batch, h=heads, m=M, n=N), pitchC)
    p.update(sam=a["m"], sak=a["k"], sab=a["b"], sah=a["h"], sbk=b["k"], sbn=b["n"], sbb=b["b"], sbh=b["h"],
             scm=c["m"], scn=c["n"], scb=c["b"], sch=c["h"], srb=0, sab2=0, sbb2=0)
    if seg2:
        for name, kind, sb in (("sab2", seg2[0], p["sab"]), ("sbb2", seg2[1], p["sbb"])):
            assert kind in ("own", "bcast") and (kind == "bcast" or (order_outer_b(A if name == "sab2" else B) and sb > 0))
            p[name] = sb + 16 if kind == "own" else 0
    if R == "own":
        assert order_outer_b(C)
        p["srb"] = p["scb"] + 64
    elif R == "alias":
        p["srb"] = p["scb"]
    else:
        assert R is None
    return p


def order_outer_b(order: str) -> bool:
    return order[0] == "b"


def nseg_of(p) -> int:
    return 2 if p["seg2"] else 1


def _last(p, name) -> int:
    """largest float offset the launch addresses in an operand, from its base"""
    M1, N1, K1, B1, H1 = p["M"] - 1, p["N"] - 1, p["K"] - 1, p["batch"] - 1, p["heads"] - 1
    if name in ("A", "A2"):
        return M1 * p["sam"] + K1 * p["sak"] + H1 * p["sah"] + B1 * p["sab" if name == "A" else "sab2"]
    if name in ("B", "B2"):
        return K1 * p["sbk"] + N1 * p["sbn"] + H1 * p["sbh"] + B1 * p["sbb" if name == "B" else "sbb2"]
    if name in ("C", "R"):
        return M1 * p["scm"] + N1 * p["scn"] + H1 * p["sch"] + B1 * p["scb" if name == "C" else "srb"]
    return M1 if name == "bias" else N1


def operand_names(p) -> List[str]:
    names = ["A", "B"] + (["A2", "B2"] if p["seg2"] else []) + (["bias"] if p["bias"] else []) + (["colbias"] if p["colbias"] else [])
    return names + (["R"] if p["R"] == "own" else [])


def base_of(p, name) -> int:
    """float offset of an operand's base inside its buffer"""
    return {"A": p["offA"], "B": p["offB"], "C": GUARD}.get(name, 0)


def count_of(p, name) -> int:
    """floats of an operand's buffer: base offset + addressed span (+ the guard bands of the output)"""
    return base_of(p, name) + _last(p, name) + 1 + (GUARD if name == "C" else 0)


def _view(buf, p, name):
    """[batch][heads][rows][cols] strided view of an operand inside its buffer"""
    B, H, M, N, K = p["batch"], p["heads"], p["M"], p["N"], p["K"]
    if name in ("A", "A2"):
        shape, st = (B, H, M, K), (p["sab" if name == "A" else "sab2"], p["sah"], p["sam"], p["sak"])
    elif name in ("B", "B2"):
        shape, st = (B, H, K, N), (p["sbb" if name == "B" else "sbb2"], p["sbh"], p["sbk"], p["sbn"])
    else:
        shape, st = (B, H, M, N), (p["scb" if name == "C" else "srb"], p["sch"], p["scm"], p["scn"])
    return torch.as_strided(buf, shape, st, base_of(p, "C" if name == "R" and p["R"] == "alias" else name))


def c_mask(p) -> torch.Tensor:
    """bool [count_of(C)]: the floats of the output buffer the strides address"""
    m = torch.zeros(count_of(p, "C"), dtype=torch.bool)
    _view(m, p, "C")[...] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# operands

def _f32(t):
    return t.to(torch.float32).to(torch.float64)


def make_operands(case, seed=0) -> List[Dict[str, torch.Tensor]]:
    """Per problem: flat float64 buffers A, B (A2, B2, bias, colbias, R) and C0 -- the output buffer's addressed floats before the
    launch where the launch reads them (beta != 0, or R aliasing C), shaped as the C buffer with zeros elsewhere.  Values are seeded
    and exactly representable in float32.  A carries an offset per row m and B one per column n (0.75 ... 1.25, random sign) under
    noise of deviation 0.5, so a dropped row, column or k range moves the result by far more than the tolerance; the floats of an
    input buffer that the strides skip hold 977, so a read through a wrong stride shows."""
    out = []
    for i, p in enumerate(case["probs"]):
        g = torch.Generator().manual_seed(7000 + 31 * seed + i)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        offs = lambda n: torch.sign(rn(n)) * (0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
        ops = {}
        for name in operand_names(p) + ["C0"]:
            if name == "C0":
                buf = torch.zeros(count_of(p, "C"), dtype=torch.float64)
                if p["beta"] != 0.0 or p["R"] == "alias":
                    v = _view(buf, p, "C")
                    v.copy_(_f32(rn(*v.shape)))
            elif name in ("bias", "colbias"):
                buf = _f32(2.0 * rn(count_of(p, name)))
                if p["colbias"] == "mask" and name == "colbias":
                    buf[[1, p["N"] // 2, p["N"] - 1]] = _f32(torch.tensor(-1e30, dtype=torch.float64))
            else:
                buf = torch.full((count_of(p, name),), 977.0, dtype=torch.float64)
                v = _view(buf, p, name)
                uniq = tuple(1 if st == 0 else s for s, st in zip(v.shape, v.stride()))      # a shared operand is stored once
                val = 0.5 * rn(*uniq) if name != "R" else rn(*uniq)
                if name in ("A", "A2"):
                    val = val + offs(p["M"]).reshape(1, 1, -1, 1)
                elif name in ("B", "B2"):
                    val = val + offs(p["N"]).reshape(1, 1, 1, -1)
                torch.as_strided(buf, uniq, v.stride(), v.storage_offset()).copy_(_f32(val))
            ops[name] = buf
        out.append(ops)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the expression

def _act(name, x):
    if name == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if name == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
    return x


def _lipschitz(name) -> float:
    """largest slope of the activation, numerically in float64 (finite differences on a grid of 1e-4 over [-12, 12]; beyond it both
    activations are the identity or zero to float64 accuracy)"""
    if name == "none":
        return 1.0
    x = torch.arange(-120000, 120001, dtype=torch.float64) * 1e-4
    y = _act(name, x)
    return float(((y[1:] - y[:-1]).abs() / 1e-4).max())


LIP = {a: _lipschitz(a) for a in ACTS}


def _bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _split(t):
    hi = _bf16(t)
    return hi, _bf16(t - hi)


def _mm(a, b, split=False, drop_lohi=False):
    """a b over the last two axes; split: both operands as bf16 hi + lo without the lo lo product (the form of attn_oracle._mm;
    drop_lohi: a planted fault, lo hi gone too)"""
    eq = "bhmk,bhkn->bhmn"
    if not split:
        return torch.einsum(eq, a, b)
    ah, al = _split(a)
    bh, bl = _split(b)
    out = torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl)
    if not drop_lohi:
        out = out + torch.einsum(eq, al, bh)
    return out


def _evaluate(p, ops, act="none", absolute=False, split=False, dtype=torch.float64, chunk=0, ksplit=1, fault=None, pre_only=False):
    """one problem: [batch][heads][M][N].  chunk > 0: the contraction in K chunks, accumulated in `dtype` (the kernels' order);
    ksplit > 1: the chunks (of 16) of all segments dealt to ksplit partial sums as gemm_rec_bf16x3 deals them, summed in order."""
    x = (lambda t: t.abs()) if absolute else (lambda t: t)
    view = lambda name: x(_view(ops[name], p, name)).to(dtype)
    K = p["K"]
    segs = [(view("A"), view("B"))]
    if p["seg2"]:
        a2 = view("A2")
        if fault == "seg2_stride":          # the second segment read with the first segment's batch stride
            q = dict(p, sab2=p["sab"])
            a2 = x(_view(ops["A2"], q, "A2")).to(dtype)
        segs.append((a2, view("B2")))
    if fault in ("ktail64", "ktail16"):     # the K tail of the last tile / record dropped
        kt = K - K % (64 if fault == "ktail64" else 16)
        assert kt < K
        segs = [(a[..., :kt], b[..., :kt, :]) for a, b in segs]
        K = kt
    lohi = fault == "drop_lohi"
    if not chunk:
        acc = sum(_mm(a, b, split, lohi) for a, b in segs)
    else:
        steps = [(s, k0) for s in range(len(segs)) for k0 in range(0, K, chunk)]
        sps = (len(steps) + ksplit - 1) // ksplit
        parts = []
        for j in range(ksplit):
            part = torch.zeros(p["batch"], p["heads"], p["M"], p["N"], dtype=dtype)
            for s, k0 in steps[j * sps:(j + 1) * sps]:
                a, b = segs[s]
                part = part + _mm(a[..., k0:k0 + chunk], b[..., k0:k0 + chunk, :], split, lohi)
            parts.append(part)
        if fault == "ksplit_missing":       # one K-split partial never reaches the reduce pass
            assert ksplit > 1
            parts.pop(1)
        acc = parts[0]
        for part in parts[1:]:
            acc = acc + part
    alpha, beta = (abs(p["alpha"]), abs(p["beta"])) if absolute else (p["alpha"], p["beta"])
    v = alpha * acc
    c0 = x(_view(ops["C0"], p, "C")).to(dtype)
    if p["beta"] != 0.0:
        v = v + beta * c0
    if p["bias"]:
        bias = x(ops["bias"]).to(dtype)
        if fault == "bias_n":               # bias indexed by the column
            assert p["N"] <= p["M"]
            v = v + bias[:p["N"]].reshape(1, 1, 1, -1)
        else:
            v = v + bias[:p["M"]].reshape(1, 1, -1, 1)
    if p["colbias"]:
        v = v + x(ops["colbias"]).to(dtype)[:p["N"]].reshape(1, 1, 1, -1)
    r = None
    if p["R"]:
        q = dict(p, sch=0) if fault == "r_nohead" else p      # R read without its head stride
        r = x(_view(ops["C0"] if p["R"] == "alias" else ops["R"], q, "R")).to(dtype)
        if fault == "beta_twice":           # an in-place residual that ALSO enters as beta C
            assert p["R"] == "alias"
            v = v + r
        if fault != "act_before_res":
            v = v + r
    if absolute or pre_only:
        return v
    v = _act(act, v)
    if r is not None and fault == "act_before_res":
        v = v + r
    return v


def _is_split(case) -> bool:
    return case["op"] in ("gemm_bf16x3", "gemm_rec")


def reference(case, ops) -> List[torch.Tensor]:
    return [_evaluate(p, o, case["act"]) for p, o in zip(case["probs"], ops)]


def magnitude(case, ops) -> List[torch.Tensor]:
    return [_evaluate(p, o, absolute=True) for p, o in zip(case["probs"], ops)]


def emulated(case, ops) -> List[torch.Tensor]:
    return [_evaluate(p, o, case["act"], split=_is_split(case)) for p, o in zip(case["probs"], ops)]


def kernel_emulation(case, ops, fault=None) -> List[torch.Tensor]:
    """float32 arithmetic in the kernels' order: K in chunks of 64 (16 and the K split for the records), the epilogue term by term.
    fault: one of FAULTS planted into it."""
    rec = case["op"] == "gemm_rec"
    ks = rec_plan(case["probs"][0])["ksplit"] if rec else 1
    outs = [_evaluate(p, o, case["act"], split=_is_split(case), dtype=torch.float32, chunk=16 if rec else 64, ksplit=ks,
                      fault=fault if fault != "pair_rowblock" else None).to(torch.float64) for p, o in zip(case["probs"], ops)]
    if fault == "pair_rowblock":            # a 32-row block of the smaller problem written by the larger problem's workgroups
        small, big = (0, 1) if case["probs"][0]["M"] < case["probs"][1]["M"] else (1, 0)
        ps, pb = case["probs"][small], case["probs"][big]
        nb, nn = min(ps["batch"], pb["batch"]), min(ps["N"], pb["N"])
        outs[small][:nb, :, ps["M"] - 32:ps["M"], :nn] = outs[big][:nb, :, ps["M"] - 32:ps["M"], :nn]
    return outs


FAULTS = ("ktail64", "ktail16", "drop_lohi", "bias_n", "r_nohead", "beta_twice", "act_before_res", "ksplit_missing", "seg2_stride",
          "pair_rowblock")


# ---------------------------------------------------------------------------------------------------------------------------
# tolerance

def additions(case, p) -> int:
    n = nseg_of(p) * p["K"]
    if case["op"] == "gemm_rec":
        ks = rec_plan(p)["ksplit"]
        n += ks if ks > 1 else 0
    return n + int(p["beta"] != 0.0) + int(p["bias"]) + int(bool(p["colbias"])) + int(bool(p["R"]))


def activation_term(case, p, ops, A) -> float:
    if case["act"] == "none":
        return 0.0
    pre = _evaluate(p, ops, pre_only=True)
    a64 = _act(case["act"], pre)
    a32 = _act(case["act"], pre.to(torch.float32)).to(torch.float64)
    return float(((a32 - a64).abs() / (LIP[case["act"]] * A).clamp_min(1e-300)).max())


def tolerance(case, ops, ref=None, A=None) -> List[dict]:
    """per problem: dict(format, accumulation, activation, tau, lip); the check is |out - ref| <= tau lip A + EPS_ABS"""
    ref = reference(case, ops) if ref is None else ref
    A = magnitude(case, ops) if A is None else A
    emu = emulated(case, ops) if _is_split(case) else None
    out = []
    for i, p in enumerate(case["probs"]):
        fmt = 0.0
        if emu is not None:
            keep = A[i] > 0
            fmt = float(((emu[i] - ref[i]).abs()[keep] / A[i][keep]).max())
        acc = (additions(case, p) + 8) * 2.0 ** -24
        act = activation_term(case, p, ops[i], A[i])
        out.append(dict(format=fmt, accumulation=acc, activation=act, tau=MARGIN * (fmt + acc + act), lip=LIP[case["act"]]))
    return out


def worst(slot, out, ref, A_out, tau):
    """(ok, message, max |out - ref| / A_out): the check |out - ref| <= tau A_out + EPS_ABS on every element, NaN counting as a
    failure; the message names the worst element's problem, batch, head, m and n"""
    err = (out.to(torch.float64) - ref).abs()
    ratio = err / (tau * A_out + EPS_ABS)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    bad = int((ratio > 1).sum())
    a = float(A_out[idx])
    msg = ("worst element: problem %d batch %d head %d m %d n %d: " % ((slot,) + idx) +
           f"out {float(out[idx])!r} ref {float(ref[idx])!r} |err| / A = {float(err[idx]) / a if a > 0 else float('inf'):.3e} "
           f"against tau = {tau:.3e}; {bad} of {ratio.numel()} elements fail")
    keep = A_out > 0
    measured = float((err[keep] / A_out[keep]).nan_to_num(nan=float("inf")).max())
    if bool((err[~keep] > EPS_ABS).any()) or bool(torch.isnan(err).any()):
        measured = float("inf")
    return bad == 0, msg, measured


def check(case, ops, outs, ref=None, A=None, tol=None):
    """(ok, [message per failing problem], [measured per problem]) of the outputs of one call against the oracle"""
    ref = reference(case, ops) if ref is None else ref
    A = magnitude(case, ops) if A is None else A
    tol = tolerance(case, ops, ref, A) if tol is None else tol
    ok, msgs, meas = True, [], []
    for i in range(len(case["probs"])):
        o, m, x = worst(i, outs[i], ref[i], tol[i]["lip"] * A[i], tol[i]["tau"])
        ok = ok and o
        meas.append(x)
        if not o:
            msgs.append(m)
    return ok, msgs, meas


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers' routing rules, restated (gemm.hip: gemm_small_taken, gemm_small_pipe_eligible, launch_gemm_pair,
# launch_gemm_bf16x3; gemm_rec.hip: rec_plan).  A device buffer starts on a 256-byte boundary, so an operand's base is 16-byte
# aligned exactly when its offset inside the buffer is a multiple of 4 floats.

SMALL_WG, REC_NT = 320, 256


def _cdiv(a, b):
    return (a + b - 1) // b


def gemm_small_taken(p) -> bool:
    return _cdiv(p["N"], 64) * _cdiv(p["M"], 64) * p["batch"] * p["heads"] < SMALL_WG and p["K"] >= 128


def gemm_small_pipe_eligible(p) -> bool:
    if p["M"] % 32 or p["N"] % 32 or p["K"] % 64 or p["K"] < 128:
        return False

    def operand(s1, s2, sb, sh, off, sb2):
        so = s2 if s1 == 1 else s1
        if (s1 != 1 and s2 != 1) or so % 4 or sb % 4 or sh % 4 or off % 4:
            return False
        return not p["seg2"] or sb2 % 4 == 0          # (the second segment's buffers start aligned)
    return (operand(p["sam"], p["sak"], p["sab"], p["sah"], p["offA"], p["sab2"]) and
            operand(p["sbn"], p["sbk"], p["sbb"], p["sbh"], p["offB"], p["sbb2"]))


def f32_variant(p) -> str:
    if not gemm_small_taken(p):
        return "gemm_f32_64"
    return "gemm_f32_small_pipe" if gemm_small_pipe_eligible(p) else "gemm_f32_small"


def pair_grouped(p0, p1) -> bool:
    return not p0["seg2"] and not p1["seg2"] and f32_variant(p0) == "gemm_f32_small_pipe" and f32_variant(p1) == "gemm_f32_small_pipe"


def bf16x3_tile(p) -> int:
    big = _cdiv(p["N"], 128) * _cdiv(p["M"], 128) * p["batch"] * p["heads"]
    return 128 if big >= 512 and p["M"] >= 128 and p["N"] >= 128 else 64


def rec_plan(p) -> dict:
    nb2, nck = p["heads"], _cdiv(p["K"], 16)
    z = [(p["batch"] if p["sab"] else 1) * nb2, (p["batch"] if p["sbb"] else 1) * nb2]
    if p["seg2"]:
        z += [(p["batch"] if p["sab2"] else 1) * nb2, (p["batch"] if p["sbb2"] else 1) * nb2]
    tm = 4 if p["M"] % 256 == 0 or p["M"] >= 1024 else 2
    tiles = _cdiv(p["M"], 64 * tm) * _cdiv(p["N"], REC_NT) * p["batch"] * nb2
    nst = nck * nseg_of(p)
    ksplit = 1
    if tiles < 224 and nst >= 64:
        eff = lambda w: w / (256.0 * _cdiv(w, 256))
        best = eff(tiles)
        for k in range(2, 9):
            if nst // k < 16:
                break
            if eff(tiles * k) > best + 0.05:
                ksplit, best = k, eff(tiles * k)
    ksplit = min(ksplit, nst)
    kcontig = [int(p["sak"] == 1), int(p["sbk"] == 1)] * nseg_of(p)
    return dict(tm=tm, ksplit=ksplit, z=z, kcontig=kcontig)


def _line(kernel, p, tm=0, ksplit=0) -> dict:
    return dict(kernel=kernel, M=p["M"], N=p["N"], K=p["K"], batch=p["batch"], heads=p["heads"], nseg=nseg_of(p),
                akm=int(p["sam"] == 1), bkm=int(p["sbn"] == 1), tm=tm, ksplit=ksplit)


def route_of(case) -> List[dict]:
    """the lines loco_debug_gemm must report, in launch order"""
    op, ps = case["op"], case["probs"]
    if op == "gemm":
        return [_line(f32_variant(ps[0]), ps[0])]
    if op == "gemm_fixed":
        return [_line("gemm_f32_fixed", ps[0])]
    if op == "gemm_bf16x3":
        return [_line("gemm_bf16x3_%d" % bf16x3_tile(ps[0]), ps[0])]
    if op == "gemm_rec":
        r = rec_plan(ps[0])
        lines = [dict(kernel="rec_split", operand=i, kcontig=r["kcontig"][i], z=r["z"][i]) for i in range(len(r["z"]))]
        lines.append(_line("gemm_rec", ps[0], r["tm"], r["ksplit"]))
        if r["ksplit"] > 1:
            lines.append(dict(kernel="gemm_rec_reduce", ksplit=r["ksplit"]))
        return lines
    if pair_grouped(ps[0], ps[1]):
        return [_line("gemm_f32_pair", ps[0]), _line("gemm_f32_pair", ps[1])]
    return [_line(f32_variant(ps[0]), ps[0]), _line(f32_variant(ps[1]), ps[1])]


def route_summary(route) -> str:
    """kernel names of a route, with tm / ksplit of a record GEMM: what the table's `expect` column holds"""
    return " ".join(r["kernel"] + (":tm%d:ks%d" % (r["tm"], r["ksplit"]) if r["kernel"] == "gemm_rec" else
                                   ":kc%d:z%d" % (r["kcontig"], r["z"]) if r["kernel"] == "rec_split" else "") for r in route)


# ---------------------------------------------------------------------------------------------------------------------------
# the case table: the smallest shapes at which each route can still go wrong.  `expect` is route_summary(route_of(case)) as derived
# once from the rules above and kept here; tests/test_gemm_oracle_host.py holds the two together.

FULL = dict(alpha=0.75, beta=1.0, bias=True, colbias="plain", R="own")      # the full epilogue


def _case(cid, family, op, probs, expect, act="none") -> dict:
    return dict(id=cid, family=family, op=op, act=act, probs=probs if isinstance(probs, list) else [probs], expect=expect)


def _cases() -> List[dict]:
    c = []
    add = lambda *a, **k: c.append(_case(*a, **k))
    # ---- exact fp32, 64 x 64 tiling (K < 128, or a grid of 320 workgroups and more)
    for K in (37, 64, 65, 127):      # every dimension ragged; one partial K-step, one whole, one whole + 1, two with a tail of 63
        add("f64_70x45_k%d" % K, "f32 64x64", "gemm", problem(70, 45, K, batch=2), "gemm_f32_64")
    add("f64_grid320_heads", "f32 64x64", "gemm",
        problem(128, 128, 128, batch=20, heads=4, A="bhmk", B="bkhn", C="bmhn", R="own"), "gemm_f32_64")
    add("f64_kstrided", "f32 64x64", "gemm", problem(70, 45, 37, batch=2, A="bhkm", B="bhkn"), "gemm_f32_64")
    add("f64_transposed_c", "f32 64x64", "gemm", problem(70, 45, 37, batch=2, C="bhnm"), "gemm_f32_64")
    # ---- exact fp32, the 32 x 32 scalar-load loop: the context K/V projection's form (N = 77 tokens, B k-major, C row pitch 128)
    add("small_ctx_kv", "f32 small", "gemm", problem(96, 77, 200, batch=2, pitchC=dict(n=128)), "gemm_f32_small")
    add("small_ctx_kv_seg2", "f32 small", "gemm", problem(96, 77, 200, batch=2, pitchC=dict(n=128), seg2=("own", "bcast")),
        "gemm_f32_small")
    add("small_misaligned_base", "f32 small", "gemm", problem(64, 96, 128, batch=2, offA=1), "gemm_f32_small")
    # ---- exact fp32, the pipelined 32 x 32 kernel
    add("pipe_k128", "f32 small pipe", "gemm", problem(64, 96, 128, batch=2), "gemm_f32_small_pipe")
    add("pipe_k192", "f32 small pipe", "gemm", problem(64, 96, 192, batch=2), "gemm_f32_small_pipe")
    for akm in (0, 1):
        for bkm in (0, 1):
            for seg2 in (None, ("own", "own")):
                full = dict(FULL, colbias="mask") if (akm, bkm, seg2) == (0, 0, None) else FULL
                add("pipe_full_a%d_b%d_seg%d" % (akm, bkm, 2 if seg2 else 1), "f32 small pipe", "gemm",
                    problem(64, 96, 192, batch=2, A="bhkm" if akm else "bhmk", B="bhkn" if bkm else "bhnk", seg2=seg2, **full),
                    "gemm_f32_small_pipe")
    add("pipe_full_heads", "f32 small pipe", "gemm", problem(64, 96, 192, batch=2, heads=2, C="bmhn", **FULL), "gemm_f32_small_pipe")
    # ---- the pair launch: two problems of different size and layout in one grid; and the fall-back to two launches
    p1 = problem(128, 32, 256, batch=3, A="bhmk", B="bhkn")
    add("pair_grouped", "f32 pair", "gemm_pair", [problem(64, 128, 128, batch=2, heads=2, A="bhkm", B="bhnk", C="bmhn"), p1],
        "gemm_f32_pair gemm_f32_pair")
    add("pair_fallback_ragged_n", "f32 pair", "gemm_pair", [problem(64, 77, 128, batch=2, A="bhkm", B="bhnk"), p1],
        "gemm_f32_small gemm_f32_small_pipe")
    # ---- launch_gemm_fixed: the encoders' linear layers, h = W f + b + h in place
    for act in ACTS:
        add("fixed_inplace_" + act, "f32 fixed", "gemm_fixed", problem(100, 80, 72, batch=2, bias=True, R="alias"), "gemm_f32_fixed", act=act)
    add("fixed_k136_small_grid", "f32 fixed", "gemm_fixed", problem(100, 80, 136, batch=2, bias=True, R="alias"), "gemm_f32_fixed")
    # ---- split-bf16 operands converted in the kernel
    add("bf16x3_64", "bf16x3 64", "gemm_bf16x3", problem(70, 45, 40, batch=2), "gemm_bf16x3_64")
    add("bf16x3_64_seg2", "bf16x3 64", "gemm_bf16x3", problem(70, 45, 72, batch=2, seg2=("own", "bcast")), "gemm_bf16x3_64")
    add("bf16x3_128_full", "bf16x3 128", "gemm_bf16x3", problem(130, 129, 40, batch=128, A="hmk", **FULL), "gemm_bf16x3_128")
    # ---- split-bf16 records (gemm_rec.hip)
    own = "rec_split:kc1:z%d rec_split:kc1:z%d "      # both operands k-contiguous: the z counts of A and B
    add("rec_min", "rec", "gemm_rec", problem(128, 256, 256), own % (1, 1) + "gemm_rec:tm2:ks1")
    add("rec_ragged_tail", "rec", "gemm_rec", problem(130, 257, 264), own % (1, 1) + "gemm_rec:tm2:ks1")
    add("rec_tm4_heads", "rec", "gemm_rec", problem(256, 512, 264, batch=2, heads=2), own % (4, 4) + "gemm_rec:tm4:ks1")
    add("rec_ksplit4", "rec ksplit", "gemm_rec", problem(128, 256, 1024, batch=5), own % (5, 5) + "gemm_rec:tm2:ks4 gemm_rec_reduce")
    add("rec_tm4_ksplit4", "rec ksplit", "gemm_rec", problem(256, 256, 1024, batch=5), own % (5, 5) + "gemm_rec:tm4:ks4 gemm_rec_reduce")
    add("rec_ksplit3_uneven", "rec ksplit", "gemm_rec", problem(136, 264, 1032, batch=2), own % (2, 2) + "gemm_rec:tm2:ks3 gemm_rec_reduce")
    add("rec_ksplit3_seg2", "rec ksplit", "gemm_rec", problem(136, 264, 520, batch=2, seg2=("own", "bcast")),
        own % (2, 2) + own % (2, 1) + "gemm_rec:tm2:ks3 gemm_rec_reduce")
    add("rec_beta", "rec", "gemm_rec", problem(128, 256, 256, alpha=0.5, beta=1.0), own % (1, 1) + "gemm_rec:tm2:ks1")
    add("rec_b_shared", "rec", "gemm_rec", problem(128, 256, 256, batch=3, B="hnk"), own % (3, 1) + "gemm_rec:tm2:ks1")
    add("rec_a_kstrided", "rec", "gemm_rec", problem(128, 256, 256, batch=2, A="bhkm"),
        "rec_split:kc0:z2 rec_split:kc1:z2 gemm_rec:tm2:ks1")
    add("rec_misaligned_base", "rec", "gemm_rec", problem(128, 256, 256, batch=2, offA=1), own % (2, 2) + "gemm_rec:tm2:ks1")
    return c


CASES = _cases()

# what loco_debug_gemm must refuse before any launch: (id, op, act, problems, what to break, text the error must contain)
_PAIR = [problem(64, 128, 128, batch=2), problem(64, 128, 128, batch=2)]
REFUSALS = [
    ("refuse_oob_stride", "gemm", "none", [problem(70, 45, 37, batch=2)], "double_sbb", "outside its buffer"),
    ("refuse_act_with_a2", "gemm_fixed", "quick_gelu", [problem(70, 45, 37, batch=2, seg2=("own", "own"))], None, "act with A2"),
    ("refuse_rec_bias", "gemm_rec", "none", [problem(128, 256, 256, bias=True)], None, "no bias"),
    ("refuse_rec_k128", "gemm_rec", "none", [problem(128, 256, 128)], None, "K >= 256"),
    ("refuse_pair_a2", "gemm_pair", "none", [_PAIR[0], problem(64, 128, 128, batch=2, seg2=("own", "own"))], None, "A2 set"),
    ("refuse_pair_overlap", "gemm_pair", "none", _PAIR, "share_c", "overlap"),
]


def descriptor(p, buffers) -> dict:
    """the loco_gemm_prob fields of a problem; buffers: {operand name: flat tensor} -> (tensor, offset) pairs as hip.py takes them"""
    d = {k: p[k] for k in ("M", "N", "K", "batch", "alpha", "beta", "sam", "sak", "sab", "sah", "sbk", "sbn", "sbb", "sbh",
                           "scm", "scn", "scb", "sch", "srb", "sab2", "sbb2")}
    d["batch2"] = p["heads"]
    for name in operand_names(p) + ["C"]:
        d[name] = (buffers[name], base_of(p, name))
    if p["R"] == "alias":
        d["R"] = (buffers["C"], base_of(p, "C"))
    return d
