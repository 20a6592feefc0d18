"""GPU: GroupNorm statistics launches of every route against float64 (loco_debug_conv with a statistics request and loco_debug_norm of
the diagnostics build vs tests/stats_oracle.py).

Conv-carried statistics: every row of stats_oracle.ROWS, under every precision it lists, is one launch through run_conv -> plan_conv
with the StatReq the engine's passes attach for the norm that consumes the output tensor.  Asserted per case, in this order:
  1. the plan names the statistics route the table claims for every launch (epi, splitk, alone; epi + splitk across a tail-probe
     split), its closing line the kept partials;
  2. nothing is left unwritten: the tensor and every statistics array are pre-filled with NaN;
  3. the tensor passes the conv check (conv_oracle.reference / tolerance / worst) -- a launch with a statistics sink is another
     template instantiation or another kernel that also writes the tensor;
  4. every statistic is within tau of the float64 statistic of the fp32 tensor the launch wrote, read back (stats_oracle.tol_fwd /
     tol_lin: bounds from the reference alone, per route); the message names the worst (sample, group) or (sample, channel);
  5. tc[b][c] == float32(f) * tst[b][g] bit for bit, f = 1 (tangent) or the primal rstd (cotangent).
The kept partials of the two "keep" producers (row tiles of 256 and of 128 pixels) then go through launch_gn_fused_finalize_cat and
launch_gn_lin_fused_finalize (loco_debug_norm) as the norm over their concatenation: 384 channels in 4 groups, one group wholly in
A, one straddling, two wholly in B, against the statistics of the concatenated read-back tensors.

Standalone launchers: every stats_oracle.NORM_CASES entry is one loco_debug_norm launch (gn_stats, gn_tstats, gn_apply, gn_cache,
the three finalize launchers on synthetic partials of chosen geometry, ctx_groupnorm), at offset levels |mean| / std of 0, 50 and
1000 where the pivot and the raw-sum subtraction matter.

One child process on the diagnostics build (LOCO_HIP_LIB), two engines (32 groups and 4 groups); no LOCO_* switch is set.  The child
is this file run as a script:   LOCO_HIP_LIB=.../libloco_hip_diag.so python tests/test_gpu_stats_oracle.py --worker out.json

Shapes outside the hooks' contracts must be REFUSED before any launch, and a keep buffer too small for the kept partials reported
(test_hooks_refuse_what_the_launchers_cannot_take).

Measured on the MI355X (first run), worst share of tau = max |got - ref| / tau per route and kind, over all cases and precisions:
  route / launcher                   kind    cases  worst share of tau
  conv epi                           fwd        17  mean 0.042  rstd 0.058  sc 0.077  sh 0.040
  conv epi                           tan        13  m1 0.025  m2 0.028
  conv epi                           cot         7  m1 0.016  m2 0.022
  conv splitk                        fwd        17  mean 0.042  rstd 0.060  sc 0.085  sh 0.052
  conv splitk                        tan        16  m1 0.042  m2 0.035
  conv splitk                        cot        16  m1 0.024  m2 0.023
  conv epi + splitk (tail split)     fwd         2  mean 0.043  rstd 0.061  sc 0.079  sh 0.039
  conv epi + splitk (tail split)     tan         2  m1 0.028  m2 0.026
  conv epi + splitk (tail split)     cot         2  m1 0.017  m2 0.022
  conv alone                         fwd         4  mean 0.035  rstd 0.057  sc 0.084  sh 0.054
  conv alone                         tan         2  m1 0.035  m2 0.021
  conv alone                         cot         4  m1 0.020  m2 0.027
  kept partials -> cat finalize      fwd         2  mean 0.004  rstd 0.019  sc 0.041  sh 0.023
  kept partials -> cat finalize      tan         2  m1 0.003  m2 0.004
  gn_stats                                      14  mean 0.041  rstd 0.052  sc 0.077  sh 0.048
  gn_tstats                          0 / 1 / 2  42  m1 0.040  m2 0.014
  gn_fused_finalize                              8  mean 0.071  rstd 0.057  sc 0.071  sh 0.065
  gn_fused_finalize_cat                          4  mean 0.057  rstd 0.040  sc 0.071  sh 0.034
  gn_lin_fused_finalize              tan        10  m1 0.016  m2 0.005
  gn_lin_fused_finalize              cot         7  m1 0.006  m2 0.005
  gn_apply                           0 ... 5    23  0.026  0.060  0.072  0.065  0.250  0.132
  gn_cache                                       2  0.210
  ctx_groupnorm                                  2  0.093
(the bounds are worst-case chains; what they must exclude is in tests/test_stats_oracle_host.py: every planted error there lands above 1)
"""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_oracle as co      # noqa: E402
import stats_oracle as so     # noqa: E402

CONV_KEYS = [(r["id"], p) for r in so.ROWS for p in r["precs"]]
CAT_KEYS = [(f"cat-{kind}", p) for kind in ("fwd", "tan") for p in ("bf16x3", "f16")]
NORM_KEYS = [n.id for n in so.NORM_CASES]
DESC_FIELDS = ("Cin", "Cout", "B", "taps", "stride", "upsample", "zins", "mode", "cpg", "transposed", "accumulate", "in_arena", "pad", "Cin2")
OPERANDS = ("weight", "bias", "in", "bias2", "res", "prim", "sc", "sh", "mr", "gamma", "tst", "tc", "in2", "w2", "bias2nd",
            "cot_d", "cot_prim", "cot_sc", "cot_sh", "cot_mr", "cot_tc")
HOST = ("weight", "bias", "w2", "bias2nd")
EPS = so.NORM_EPS
LIMIT_S = 20.0


def _summary(checks):
    """checks: [(name, ok, share, message)] -> (ok, {name: share}, message of the failures)"""
    return (all(c[1] for c in checks), {c[0]: c[2] for c in checks}, "; ".join(f"{c[0]}: {c[3]}" for c in checks if not c[1]))


def _run_conv_row(engs, torch, row, prec, cache, kept):
    d, kind = row["case"], row["kind"]
    eng = engs[row["engine"]]
    G = so.GN_GROUPS[row["engine"]]
    B, Cout = d["B"], d["Cout"]
    ho, wo = co.out_hw(d)
    cpg = Cout // G
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    dev = lambda t: t.to(torch.float32).cuda()
    cid = co.case_id(d)
    if cache.get("cid") != cid:      # operands, conv reference and its tolerances: once per conv case, shared by its kinds
        cache.clear()
        ops = co.make_operands(d)
        cache.update(cid=cid, ops=ops, dev={k: dev(v) for k, v in ops.items() if k in OPERANDS and k not in HOST})
    if cache.get("id") != row["id"]:
        g = torch.Generator().manual_seed(4241 + 97 * Cout + 13 * ho + so.KINDS[kind])
        no = so.norm_operands(Cout, G, g, ss=row["ss"])
        pr = so.primal_operands(Cout, ho, wo, G, no["gamma"], no["beta"], EPS, g) if kind != "fwd" else None
        cache.update(id=row["id"], no=no, pr=pr)
    ops, no, pr = cache["ops"], cache["no"], cache["pr"]
    kw = {k: d[k] for k in DESC_FIELDS}
    kw.update(Hin=d["H"], Win=d["W"], res_scale=d["res_scale"])
    if d["cot"]:
        kw["cot_cpg"] = d["cot_cpg"]
    for k in OPERANDS:
        if k in ops:
            kw[k] = ops[k].to(torch.float32) if k in HOST else cache["dev"][k]
    out = dev(ops["out0"]) if d["accumulate"] else nan(B, Cout, ho, wo)
    kw.update(st_kind=so.KINDS[kind], st_eps=EPS, st_gamma=dev(no["gamma"]), st_beta=dev(no["beta"]))
    outs = {}
    if kind == "fwd":
        outs = dict(st_o_mr=nan(B, G, 2), st_o_sc=nan(B, Cout), st_o_sh=nan(B, Cout))
        if row["ss"]:
            kw.update(st_ss_scale=dev(no["ss_scale"]), st_ss_shift=dev(no["ss_shift"]))
    else:
        outs = dict(st_o_tst=nan(B, G, 2), st_o_tc=nan(B, Cout, 2))
        kw.update(st_prim=dev(pr["prim"]), st_sc=dev(pr["sc"]), st_sh=dev(pr["sh"]), st_mr=dev(pr["mr"]))
    kw.update(outs)
    keep_out = None
    if row["keep"]:
        keep_out = nan(B * Cout * (ho * wo // 64) * 2)
        kw.update(st_keep=1, st_keep_out=keep_out, st_keep_cap=keep_out.numel())
    eng.set_precision(prec)
    res = dict(id=row["id"], prec=prec, family=row["family"], kind=kind, routes=list(row["routes"]))
    t0 = time.time()
    try:
        plan, rode, closing = eng.debug_conv(out, with_closing=True, **kw)
    except RuntimeError as e:      # refused or failed: the case fails with the library's words
        return dict(res, plan_bad=[str(e)], plan=[], unwritten=0, conv_ok=False, conv_msg="", ok=False, shares={}, msg="", tc_bad=0, nt=[],
                    total_s=time.time() - t0)
    torch.cuda.synchronize()
    res["gpu_s"] = time.time() - t0
    got = out.cpu().to(torch.float64)
    st = {k: v.cpu() for k, v in outs.items()}
    # 1. the route
    res["plan_bad"] = so.check_route(plan, closing, row)
    res["plan"] = [f"{p['kernel']} stats={p['stats']} ntile={p['ntile']}" for p in plan]
    # 2. unwritten
    res["unwritten"] = int(torch.isnan(got).sum()) + sum(int(torch.isnan(v).sum()) for v in st.values())
    # 3. the tensor
    dd, oo, gg = d, ops, got
    if row["probes"]:
        dd, oo = co.sub_case(d, ops, list(row["probes"]))
        gg = got.index_select(0, torch.tensor(list(row["probes"])))
    rk = ("ref", row["probes"])
    if rk not in cache:
        cache[rk] = (co.reference(dd, oo), co.magnitude(dd, oo))
    ref, A = cache[rk]
    tk = ("tol", row["probes"], prec)
    if tk not in cache:
        cache[tk] = co.tolerance(dd, oo, prec, ref, A)
    tol = cache[tk]
    res["conv_ok"], res["conv_msg"] = co.worst(gg, ref, A, tol["tau"])
    if d["cot"] and not rode:
        res["conv_ok"], res["conv_msg"] = False, "the norm-cotangent term was declined"
    # 4. the statistics, against those of the tensor the launch wrote
    nt = so.nt_of(plan, d, B)
    x = torch.nan_to_num(got)
    if kind == "fwd":
        tl = so.tol_fwd(x, G, no["gamma"], no["beta"], EPS, nt, no.get("ss_scale"), no.get("ss_shift"))
        ok, shares, msg = _summary(so.check_fwd(st["st_o_mr"], st["st_o_sc"], st["st_o_sh"], tl))
        res["tc_bad"] = 0
    else:
        P = {k: v.unsqueeze(0) for k, v in pr.items()}
        zk = 0 if kind == "tan" else 1
        tl = so.tol_lin(zk, x, P["prim"], P["sc"], P["sh"], P["mr"], cpg, so.ACT_SILU, nt)
        ok, shares, msg = _summary(so.check_lin(st["st_o_tst"], tl))
        # 5. the per-channel expansion
        res["tc_bad"] = so.tc_mismatch(st["st_o_tc"], st["st_o_tst"], P["mr"], cpg, kind == "cot")
    res.update(ok=ok, shares=shares, msg=msg, nt=nt)
    if row["keep"]:
        kn = closing["keep_ntile"] if closing else 0
        part = keep_out[:B * Cout * kn * 2].reshape(B, Cout, kn, 2).clone() if kn else None
        kept[(row["family"], kind, prec)] = dict(part=part, nt=kn, x=got, prim=None if pr is None else pr["prim"])
        res["unwritten"] += 0 if part is None else int(torch.isnan(part).sum())
    res["total_s"] = time.time() - t0
    return res


def _run_cat(eng, torch, kind, prec, kept):
    """the norm over [keep A | keep B] from the producers' kept partials"""
    c = so.CAT
    a, b = kept.get(("keep A", kind, prec)), kept.get(("keep B", kind, prec))
    res = dict(id=f"cat-{kind}", prec=prec, kind=kind)
    t0 = time.time()
    if not a or not b or a["part"] is None or b["part"] is None:
        return dict(res, ok=False, msg="a producer kept no partials", unwritten=0, tc_bad=0, shares={}, total_s=0.0)
    C, G, C1, HW = c["C"], c["G"], c["C1"], c["HW"]
    cpg = C // G
    B = a["x"].shape[0]
    assert (a["nt"], b["nt"]) == (c["ntA"], c["ntB"]), (a["nt"], b["nt"])
    g = torch.Generator().manual_seed(77)
    no = so.norm_operands(C, G, g)
    x = torch.cat([a["x"], b["x"]], 1)
    nt = torch.cat([torch.full((B, C1), HW // a["nt"]), torch.full((B, C - C1), HW // b["nt"])], 1)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    dev = lambda t: t.to(torch.float32).cuda()
    if kind == "fwd":
        arena = nan(B, 2 * C + 2 * G)
        eng.debug_norm("gn_fused_finalize_cat", B=B, C=C, HW=HW, G=G, C1=C1, ntA=a["nt"], ntB=b["nt"], eps=EPS, partA=a["part"],
                       partB=b["part"], gamma=dev(no["gamma"]), beta=dev(no["beta"]), o_sc=arena[:, :C], o_sh=arena[:, C:2 * C],
                       o_mr=arena[:, 2 * C:], o_bs=arena.shape[1])
        h = arena.cpu()
        tl = so.tol_fwd(x, G, no["gamma"], no["beta"], EPS, nt)
        ok, shares, msg = _summary(so.check_fwd(h[:, 2 * C:].reshape(B, G, 2), h[:, :C], h[:, C:2 * C], tl))
        tc_bad = 0
    else:
        prim = torch.cat([a["prim"], b["prim"]], 0)
        mr, sc, sh = so.fwd_stats(prim.unsqueeze(0), G, no["gamma"], no["beta"], EPS)
        mr, sc, sh = so._f32(mr), so._f32(sc), so._f32(sh)
        arena = nan(B, 2 * G + 2 * C)
        eng.debug_norm("gn_lin_fused_finalize", kind=so.ST_TAN, B=B, C=C, HW=HW, G=G, C1=C1, ntA=a["nt"], ntB=b["nt"], partA=a["part"],
                       partB=b["part"], mr=dev(mr[0]), o_tst=arena[:, :2 * G], o_tc=arena[:, 2 * G:], o_bs=arena.shape[1])
        h = arena.cpu()
        tst, tc = h[:, :2 * G].reshape(B, G, 2), h[:, 2 * G:].reshape(B, C, 2)
        tl = so.tol_lin(0, x, prim.unsqueeze(0), sc, sh, mr, cpg, so.ACT_SILU, nt)
        ok, shares, msg = _summary(so.check_lin(tst, tl))
        tc_bad = so.tc_mismatch(tc, tst, mr, cpg, False)
    return dict(res, ok=ok, msg=msg, shares=shares, tc_bad=tc_bad, unwritten=int(torch.isnan(h).sum()), total_s=time.time() - t0)


def _run_norm(eng, torch, n):
    inp = so.norm_inputs(n)
    C, G, H, W, B = n.C, n.G, n.H, n.W, n.B
    HW, cpg = H * W, C // G
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    dev = lambda t: t.to(torch.float32).cuda().contiguous()
    res = dict(id=n.id, op=n.op, kind=n.kind, tc_bad=0)
    t0 = time.time()
    gamma, beta = inp["gamma"], inp["beta"]
    if n.op == "ctx_groupnorm":
        out = nan(H, C)
        eng.debug_norm(n.op, C=C, HW=H, G=G, eps=EPS, x=dev(inp["x"]), gamma=dev(gamma), beta=dev(beta), out=out)
        got = out.cpu().to(torch.float64)
        ref, tau = so.tol_ctx(inp["x"], G, gamma, beta, EPS)
        ok, share, msg = so.worst(got, ref, tau, "(token, channel)")
        return dict(res, ok=ok, msg=msg, shares={"out": share}, unwritten=int(torch.isnan(got).sum()), total_s=time.time() - t0)
    x, d = inp["x"], inp["d"]
    prim, sc, sh, mr = inp["prim"], inp["sc"], inp["sh"], inp["mr"]           # [Bp][...]
    Bp = prim.shape[0]
    pk = dict(sc=dev(sc), sh=dev(sh), mr=dev(mr), pbs_c=C if Bp > 1 else 0, pbs_g=2 * G if Bp > 1 else 0)
    ss = (inp.get("ss_scale"), inp.get("ss_shift"))
    ssk = dict(ss_scale=dev(ss[0]), ss_shift=dev(ss[1])) if n.ss else {}
    if n.op in ("gn_stats", "gn_fused_finalize", "gn_fused_finalize_cat"):
        arena = nan(B, 2 * C + 2 * G)
        ok_ = dict(o_sc=arena[:, :C], o_sh=arena[:, C:2 * C], o_mr=arena[:, 2 * C:], o_bs=arena.shape[1], eps=EPS, gamma=dev(gamma), beta=dev(beta))
        if n.op == "gn_stats":
            eng.debug_norm(n.op, B=B, C=C, HW=HW, G=G, x=dev(x), x_bs=C * HW, **ok_, **ssk)
            nt = 0
        elif n.op == "gn_fused_finalize":
            eng.debug_norm(n.op, B=B, C=C, HW=HW, G=G, ntA=HW // n.ntA, partA=dev(so.partials_fwd(x, n.ntA)), **ok_, **ssk)
            nt = n.ntA
        else:
            eng.debug_norm(n.op, B=B, C=C, HW=HW, G=G, C1=n.C1, ntA=HW // n.ntA, ntB=HW // n.ntB, partA=dev(so.partials_fwd(x[:, :n.C1], n.ntA)),
                           partB=dev(so.partials_fwd(x[:, n.C1:], n.ntB)), **ok_)
            nt = torch.cat([torch.full((B, n.C1), n.ntA), torch.full((B, C - n.C1), n.ntB)], 1)
        h = arena.cpu()
        tl = so.tol_fwd(x, G, gamma, beta, EPS, nt, *ss)
        ok, shares, msg = _summary(so.check_fwd(h[:, 2 * C:].reshape(B, G, 2), h[:, :C], h[:, C:2 * C], tl))
        return dict(res, ok=ok, msg=msg, shares=shares, unwritten=int(torch.isnan(h).sum()), total_s=time.time() - t0)
    if n.op in ("gn_tstats", "gn_lin_fused_finalize"):
        arena = nan(B, 2 * G + 2 * C)
        ok_ = dict(o_tst=arena[:, :2 * G], o_tc=arena[:, 2 * G:], o_bs=arena.shape[1])
        if n.op == "gn_tstats":
            zk, nt = n.kind, 0
            eng.debug_norm(n.op, kind=n.kind, act=n.act, B=B, C=C, HW=HW, G=G, d=dev(d), d_bs=C * HW, x=dev(prim), x_bs=C * HW if Bp > 1 else 0,
                           **pk, **ok_)
        else:
            zk = 0 if n.kind == so.ST_TAN else 1
            if n.kind == so.ST_TAN:
                pa = so.partials_tan(d[:, :n.C1] if n.ntB else d, prim[0, :n.C1] if n.ntB else prim[0], n.ntA)
            else:
                pa = so.partials_cot(d, so.records(prim[0], sc[0], sh[0], mr[0], cpg, n.act), n.ntA)
            two = dict(C1=n.C1, ntB=HW // n.ntB, partB=dev(so.partials_tan(d[:, n.C1:], prim[0, n.C1:], n.ntB))) if n.ntB else {}
            eng.debug_norm(n.op, kind=n.kind, B=B, C=C, HW=HW, G=G, ntA=HW // n.ntA, partA=dev(pa), mr=dev(mr[0]), **two, **ok_)
            nt = torch.cat([torch.full((B, n.C1), n.ntA), torch.full((B, C - n.C1), n.ntB)], 1) if n.ntB else n.ntA
        h = arena.cpu()
        tst, tc = h[:, :2 * G].reshape(B, G, 2), h[:, 2 * G:].reshape(B, C, 2)
        tl = so.tol_lin(zk, d, prim, sc, sh, mr, cpg, n.act, nt)
        ok, shares, msg = _summary(so.check_lin(tst, tl))
        return dict(res, ok=ok, msg=msg, shares=shares, unwritten=int(torch.isnan(h).sum()), tc_bad=so.tc_mismatch(tc, tst, mr, cpg, zk != 0),
                    total_s=time.time() - t0)
    if n.op == "gn_cache":
        out = nan(C, H, W, 2)
        eng.debug_norm(n.op, act=n.act, C=C, HW=HW, G=G, x=dev(prim[0]), sc=dev(sc[0]), sh=dev(sh[0]), mr=dev(mr[0]), out=out)
        got = out.cpu().to(torch.float64)
        ref, tau = so.tol_records(prim[0], sc[0], sh[0], mr[0], cpg, n.act)
        ok, share, msg = so.worst(got, ref, tau, "(channel, y, x, {S, xhat})")
        return dict(res, ok=ok, msg=msg, shares={"records": share}, unwritten=int(torch.isnan(got).sum()), total_s=time.time() - t0)
    assert n.op == "gn_apply"
    zk = {1: 0, 5: 0, 2: 1, 3: 2}.get(n.kind)
    kw, gk = {}, {}
    if zk is not None:
        tst = so._f32(so.lin_stats(so.z_of(zk, d, prim, sc, sh, mr, cpg, n.act), prim, mr, cpg))
        kw.update(d=d, mr=mr, tst=tst)
        gk.update(d=dev(d), d_bs=C * HW, tst=dev(tst), t_bs=2 * G)
    if n.base:
        kw.update(base=inp["base"], base_scale=0.7071067811865476)
        gk.update(base=dev(inp["base"]), base_bs=C * HW, base_scale=0.7071067811865476)
    if n.acc:
        kw.update(out0=inp["out0"])
    out = dev(inp["out0"]) if n.acc else nan(B, C, H, W)
    xp = prim.expand(B, -1, -1, -1) if Bp == 1 else prim
    eng.debug_norm(n.op, kind=n.kind, act=n.act, B=B, C=C, HW=HW, G=G, accumulate=int(n.acc), x=dev(prim), x_bs=C * HW if Bp > 1 else 0,
                   out=out, out_bs=C * HW, **pk, **gk)
    got = out.cpu().to(torch.float64)
    tau, A = so.tol_apply(n.kind, xp, sc, sh, cpg, act=n.act, **kw)
    ref = so.apply(n.kind, xp, sc, sh, cpg, act=n.act, **kw)
    ok, share, msg = so.worst(got, ref, tau * A + so.EPS_ABS, "(b, c, y, x)")
    return dict(res, ok=ok, msg=msg, shares={"out": share}, unwritten=int(torch.isnan(got).sum()), total_s=time.time() - t0)


REFUSALS = ("conv: Cout not a multiple of gn_groups", "conv: B beyond max_batch", "conv: no gamma", "conv: keep with COT",
            "conv: 4 Cout + 4 G beyond a sample's statistics slot", "conv: COT records beyond the record cache",
            "conv: kept partials beyond st_keep_cap", "norm: kind out of range", "norm: tile count not dividing HW",
            "norm: C not a multiple of G", "norm: HW not a multiple of 4", "norm: more than 256 channels per group",
            "norm: null operand", "norm: B G beyond the reduction buffer")


def _refusals(eng, torch):
    """shapes outside the hooks' contracts: each must raise before any launch -> {name: [refused, message]}"""
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    w = lambda co_, ci: torch.zeros(co_, ci, 1, 1)
    conv = lambda Cout, B=1, **kw: (lambda: eng.debug_conv(z(B, Cout, 8, 8), Cin=16, Cout=Cout, Hin=8, Win=8, B=B, taps=1, weight=w(Cout, 16),
                                                           **{"in": z(B, 16, 8, 8)}, **kw))
    fwd = lambda C, B=1: dict(st_kind=1, st_gamma=z(C), st_beta=z(C), st_o_mr=z(B, 32, 2), st_o_sc=z(B, C), st_o_sh=z(B, C))
    stats = lambda C, G, HW, B=1, **kw: (lambda: eng.debug_norm("gn_stats", **dict(dict(
        B=B, C=C, HW=HW, G=G, eps=EPS, x=z(B, C, HW), x_bs=C * HW, gamma=z(C), beta=z(C), o_mr=z(B, 2 * G), o_sc=z(B, C), o_sh=z(B, C),
        o_bs=C), **kw)))
    nogamma = fwd(64)
    nogamma.pop("st_gamma")
    cot_keep = dict(st_kind=3, st_gamma=z(64), st_beta=z(64), st_prim=z(64, 8, 8), st_sc=z(64), st_sh=z(64), st_mr=z(32, 2),
                    st_o_tst=z(1, 32, 2), st_o_tc=z(1, 64, 2), st_keep=1, st_keep_out=z(4096), st_keep_cap=4096)
    # (Hout Wout % 4 cannot be reached: the maps the conv kernels walk, which the hook admits first, are all multiples of 4)
    big = 1 << 18      # 4 Cout floats: more than every norm of the network takes together in a sample's slot
    def cot_big():     # 8192 channels at 256 x 256: 2^29 records, more than the network's norms cache together
        C, hw = 8192, 256
        return eng.debug_conv(z(1, C, hw, hw), Cin=16, Cout=C, Hin=hw, Win=hw, B=1, taps=1, weight=w(C, 16), **{"in": z(1, 16, hw, hw)},
                              st_kind=3, st_gamma=z(C), st_beta=z(C), st_prim=z(C, hw, hw), st_sc=z(C), st_sh=z(C), st_mr=z(32, 2),
                              st_o_tst=z(1, 32, 2), st_o_tc=z(1, C, 2))
    def keep_short():  # a 128-cout 1x1 launch that keeps 128 x ntile x 2 floats, handed room for 8
        return eng.debug_conv(z(2, 128, 16, 16), Cin=48, Cout=128, Hin=16, Win=16, B=2, taps=1, weight=w(128, 48), **{"in": z(2, 48, 16, 16)},
                              st_keep=1, st_keep_out=z(8), st_keep_cap=8, **fwd(128, 2))
    kind9 = lambda: eng.debug_norm("gn_tstats", kind=9, B=1, C=8, HW=16, G=2, d=z(1, 8, 16), x=z(1, 8, 16), sc=z(8), sh=z(8), mr=z(2, 2),
                                   o_tst=z(1, 4), o_bs=4)
    nt3 = lambda: eng.debug_norm("gn_fused_finalize", B=1, C=8, HW=16, G=2, ntA=3, partA=z(1, 8, 3, 2), eps=EPS, gamma=z(8), beta=z(8),
                                 o_mr=z(1, 4), o_sc=z(1, 8), o_sh=z(1, 8), o_bs=8)
    calls = dict(zip(REFUSALS, (conv(40, **fwd(40)), conv(64, B=11, **fwd(64, 11)), conv(64, **nogamma), conv(64, **cot_keep),
                                conv(big, **fwd(big)), cot_big, keep_short, kind9, nt3,
                                stats(30, 4, 64), stats(8, 2, 6), stats(1024, 2, 16), stats(8, 2, 16, gamma=None),
                                stats(8192, 8192, 4, B=2))))
    out = {}
    for name, call in calls.items():
        try:
            call()
            out[name] = [False, "the hook took it"]
        except RuntimeError as e:
            out[name] = [True, str(e)]
    return out


def _worker(path):
    sys.path.insert(0, ROOT)
    import dataclasses
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import CELEBA_DDPM, synth_params
    torch.set_num_threads(min(16, torch.get_num_threads()))
    assert CELEBA_DDPM.gn_groups == so.GN_GROUPS["g32"]
    engs = {}
    for name, G in so.GN_GROUPS.items():
        cfg = dataclasses.replace(CELEBA_DDPM, gn_groups=G)
        engs[name] = H.LocoEngine(cfg, max_batch=10)
        engs[name].load_state_dict(synth_params(cfg, 0))
    results, cache, kept = [], {}, {}

    def emit(r):
        print(json.dumps({k: v for k, v in r.items() if k not in ("msg", "conv_msg")}), flush=True)
        results.append(r)
    for row in so.ROWS:
        for prec in row["precs"]:
            emit(_run_conv_row(engs, torch, row, prec, cache, kept))
    for cid, prec in CAT_KEYS:
        emit(_run_cat(engs["g32"], torch, cid.split("-")[1], prec, kept))
    for n in so.NORM_CASES:
        emit(_run_norm(engs["g32"], torch, n))
    emit(dict(id="refusals", refusals=_refusals(engs["g32"], torch)))
    with open(path, "w") as f:
        json.dump(results, f)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    _worker(sys.argv[2])
    sys.exit(0)


def _diag_lib():
    path = os.path.join(ROOT, "loco-edit_amd", "libloco_hip_diag.so")
    assert os.path.exists(path), "libloco_hip_diag.so is missing: run `make -C loco-edit_amd/csrc diag` (or __graft_entry__.build())"
    return path


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every table on two engines of the diagnostics build, in one child process"""
    out = str(tmp_path_factory.mktemp("stats_oracle") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env["LOCO_HIP_LIB"] = _diag_lib()
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out], env=env, capture_output=True, text=True, timeout=1500)
    done = r.stdout.count("\n")
    total = len(CONV_KEYS) + len(CAT_KEYS) + len(NORM_KEYS) + 1
    assert r.returncode == 0, f"the worker ended with {r.returncode} after {done} of {total} cases:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    with open(out) as f:
        return {(x["id"], x.get("prec")): x for x in json.load(f)}


def _assert_stats(r, what):
    assert r["unwritten"] == 0, f"{what}: {r['unwritten']} entries were never written (NaN sentinel left); {r['msg']}"
    print(f"{what}: worst share of tau " + ", ".join(f"{k} {v:.3f}" for k, v in r["shares"].items()))
    assert r["ok"], f"{what}: {r['msg']}"
    assert r["tc_bad"] == 0, f"{what}: {r['tc_bad']} entries of tc are not float32(f) * tst"
    assert r["total_s"] < LIMIT_S, f"the case took {r['total_s']:.1f} s"


@pytest.mark.gpu
@pytest.mark.parametrize("cid, prec", CONV_KEYS, ids=[f"{c}-{p}" for c, p in CONV_KEYS])
def test_conv_carried_statistics_match_float64(results, cid, prec):
    r = results[(cid, prec)]
    assert not r["plan_bad"], f"{r['family']}: {r['plan_bad']} (planned {r['plan']})"
    assert r["unwritten"] == 0, f"{r['unwritten']} entries were never written (NaN sentinel left); planned {r['plan']}; {r['conv_msg']}; {r['msg']}"
    assert r["conv_ok"], f"{r['family']} ({', '.join(r['plan'])}): the tensor: {r['conv_msg']}"
    _assert_stats(r, f"{r['family']} {r['kind']} via {'+'.join(r['routes'])} (tile pixels per sample {r['nt']})")


@pytest.mark.gpu
@pytest.mark.parametrize("cid, prec", CAT_KEYS, ids=[f"{c}-{p}" for c, p in CAT_KEYS])
def test_kept_partials_of_two_producers_give_the_statistics_of_the_concatenation(results, cid, prec):
    _assert_stats(results[(cid, prec)], f"{cid} {prec}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", REFUSALS)
def test_hooks_refuse_what_the_launchers_cannot_take(results, name):
    refused, msg = results[("refusals", None)]["refusals"][name]
    assert refused, msg
    assert "debug_conv" in msg or "debug_norm" in msg, msg
    want = {"conv: 4 Cout + 4 G beyond a sample's statistics slot": "statistics slot", "conv: COT records beyond the record cache": "record cache",
            "conv: kept partials beyond st_keep_cap": "st_keep_out too small", "norm: kind out of range": "kind out of range",
            "norm: tile count not dividing HW": "tile counts"}.get(name)
    assert want is None or want in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("nid", NORM_KEYS)
def test_standalone_launcher_matches_float64(results, nid):
    _assert_stats(results[(nid, None)], nid)
