"""CPU: the float64 statistics reference of tests/stats_oracle.py against torch's GroupNorm and torch.func, its conv-carried case
table against the host-compiled planner, and its tolerances against fp32 restatements of every route with and without planted errors.

  - the reference means what the engine means: fwd_stats + apply(0) is F.group_norm, apply(1) / apply(5) are torch.func.jvp through
    the norm (and the activation), apply(3) / apply(2) torch.func.vjp, with {m1, m2} from lin_stats; records and the token-major
    norm likewise; merging the reference's own row-tile partials reproduces the direct statistics to 1e-11;
  - every conv-carried row reaches the statistics route it names under conv_plan.hip compiled with g++ (tests/c/conv_plan_cases.cpp
    with the statistics ask), for every precision the row runs under;
  - an fp32 restatement of each route (stats_oracle.route32_*) stays inside tau on these operands, at every offset level, with no
    bound's scale vanishing;
  - the check rejects on that restatement: a row tile left out of a merge, the M2 merge without its between-tiles term, the cat
    finalize weighting both parts with one tile size, the tangent m2 without - mean sum d, tc not scaled by rstd, a group reading its
    neighbour's {mean, rstd}, a sample's result in the next sample's slot, statistics taken before the residual went in;
  - the bounds of the {S, xhat} records and of the token-major norm hold for their fp32 restatements and reject planted errors.
"""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import conv_oracle as co
import stats_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
D = torch.float64
EPS = 1e-6


def _close(a, b, tol=1e-11):
    scale = max(float(b.abs().max()), 1.0)
    assert float((a - b).abs().max()) <= tol * scale, (float((a - b).abs().max()), scale)


def _setup(B=2, C=8, G=2, H=8, W=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    no = so.norm_operands(C, G, g)
    x = torch.randn(B, C, H, W, generator=g, dtype=D) * 0.7 + 1.5 + torch.randn(1, C, 1, 1, generator=g, dtype=D)
    return g, x, no["gamma"], no["beta"]


# ---- the reference means what the engine means ----------------------------------------------------------------------------------

def test_forward_statistics_are_group_norm():
    g, x, gamma, beta = _setup()
    mr, sc, sh = so.fwd_stats(x, 2, gamma, beta, EPS)
    _close(so.apply(0, x, sc, sh, 4), F.group_norm(x, 2, gamma, beta, eps=EPS))
    _close(so.apply(4, x, sc, sh, 4), F.silu(F.group_norm(x, 2, gamma, beta, eps=EPS)))
    _close(so.apply(4, x, sc, sh, 4, act=so.ACT_GELU), F.gelu(F.group_norm(x, 2, gamma, beta, eps=EPS)))
    s, t = torch.randn(8, generator=g, dtype=D), torch.randn(8, generator=g, dtype=D)
    _, sc2, sh2 = so.fwd_stats(x, 2, gamma, beta, EPS, s, t)
    _close(so.apply(0, x, sc2, sh2, 4), F.group_norm(x, 2, gamma, beta, eps=EPS) * (1 + s).view(1, -1, 1, 1) + t.view(1, -1, 1, 1))
    xg = x.reshape(2, 2, -1)
    _close(mr[..., 0], xg.mean(2))
    _close(mr[..., 1], 1 / torch.sqrt(xg.var(2, unbiased=False) + EPS))


@pytest.mark.parametrize("act", [so.ACT_SILU, so.ACT_GELU])
def test_tangent_kinds_are_the_jvp_and_cotangent_kinds_the_vjp(act):
    g, x, gamma, beta = _setup(B=1)
    B, G, cpg = 3, 2, 4
    mr, sc, sh = so.fwd_stats(x, G, gamma, beta, EPS)
    v = torch.randn(B, 8, 8, 8, generator=g, dtype=D)
    norm = lambda t: F.group_norm(t, G, gamma, beta, eps=EPS)
    fa = (lambda t: F.gelu(t)) if act == so.ACT_GELU else F.silu
    tst = so.lin_stats(so.z_of(0, v, x, sc, sh, mr, cpg), x, mr, cpg)
    want1 = torch.cat([torch.func.jvp(norm, (x,), (v[b:b + 1],))[1] for b in range(B)])
    _close(so.apply(1, x, sc, sh, cpg, d=v, mr=mr, tst=tst), want1)
    want5 = torch.cat([torch.func.jvp(lambda t: fa(norm(t)), (x,), (v[b:b + 1],))[1] for b in range(B)])
    _close(so.apply(5, x, sc, sh, cpg, d=v, mr=mr, tst=tst, act=act), want5)
    base = torch.randn(B, 8, 8, 8, generator=g, dtype=D)
    tst3 = so.lin_stats(so.z_of(2, v, x, sc, sh, mr, cpg), x, mr, cpg)
    want3 = torch.cat([torch.func.vjp(norm, x)[1](v[b:b + 1])[0] for b in range(B)])
    _close(so.apply(3, x, sc, sh, cpg, d=v, mr=mr, tst=tst3, base=base, base_scale=0.5, out0=base), want3 + 1.5 * base)
    tst2 = so.lin_stats(so.z_of(1, v, x, sc, sh, mr, cpg, act), x, mr, cpg)
    want2 = torch.cat([torch.func.vjp(lambda t: fa(norm(t)), x)[1](v[b:b + 1])[0] for b in range(B)])
    _close(so.apply(2, x, sc, sh, cpg, d=v, mr=mr, tst=tst2, act=act), want2)
    rec = so.records(x[0], sc[0], sh[0], mr[0], cpg, act)
    y = sc[0].view(-1, 1, 1) * x[0] + sh[0].view(-1, 1, 1)
    _close(rec[..., 0], sc[0].view(-1, 1, 1) * so.act_d(y, act))
    _close(rec[..., 1], so.xhat_of(x, mr, cpg)[0])
    # act_d2 is the derivative of act_d (the absolute forms use it)
    yy = torch.linspace(-4, 4, 101, dtype=D, requires_grad=True)
    _close(so.act_d2(yy, act).detach(), torch.autograd.grad(so.act_d(yy, act).sum(), yy)[0])


def test_token_major_norm_is_group_norm_on_the_transposed_states():
    g = torch.Generator().manual_seed(3)
    tok = torch.randn(77, 64, generator=g, dtype=D) + 2.0
    no = so.norm_operands(64, 4, g)
    for G in (4, 32):
        want = F.group_norm(tok.t().unsqueeze(0), G, no["gamma"], no["beta"], eps=EPS)[0].t()
        _close(so.ctx_groupnorm(tok, G, no["gamma"], no["beta"], EPS), want)


@pytest.mark.parametrize("NT", [64, 128, 256])
def test_merging_the_row_tile_partials_reproduces_the_direct_statistics(NT):
    g, x, gamma, beta = _setup(B=2, C=12, G=3, H=16, W=32, seed=5)
    G, cpg, HW = 3, 4, 512
    mr, sc, sh = so.fwd_stats(x, G, gamma, beta, EPS)
    _close(so.merge_fwd([so.partials_fwd(x, NT)], HW, G, EPS), mr)
    # a concatenation whose parts have different tiles, a group straddling them (C1 = 6 of 12 in groups of 4)
    _close(so.merge_fwd([so.partials_fwd(x[:, :6], NT), so.partials_fwd(x[:, 6:], 64)], HW, G, EPS), mr)
    p = so.primal_operands(12, 16, 32, G, gamma, beta, EPS, g)
    pr, pmr, psc, psh = p["prim"].unsqueeze(0), p["mr"].unsqueeze(0), p["sc"].unsqueeze(0), p["sh"].unsqueeze(0)
    want = so.lin_stats(x, pr, pmr, cpg)
    _close(so.merge_lin(so.ST_TAN, [so.partials_tan(x, p["prim"], NT)], HW, G, pmr), want)
    _close(so.merge_lin(so.ST_TAN, [so.partials_tan(x[:, :6], p["prim"][:6], NT), so.partials_tan(x[:, 6:], p["prim"][6:], 64)], HW, G, pmr), want)
    rec = so.records(p["prim"], p["sc"], p["sh"], p["mr"], cpg)
    wantc = so.lin_stats(so.z_of(1, x, pr, psc, psh, pmr, cpg), pr, pmr, cpg)
    _close(so.merge_lin(so.ST_COT, [so.partials_cot(x, rec, NT)], HW, G, pmr), wantc)


def test_row_tiles_start_at_the_top_left_pixel_and_cover_the_map_once():
    t = torch.arange(2 * 16 * 64, dtype=D).reshape(2, 16, 64)
    v = so.row_tiles(t, 256)                 # 32 columns x 8 rows
    assert v.shape == (2, 4, 256)
    assert v[0, :, 0].tolist() == [0.0, 32.0, 8 * 64.0, 8 * 64.0 + 32]
    assert sorted(v[1].flatten().tolist()) == t[1].flatten().tolist()


# ---- the case table against the planner ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip(f"HIP headers not found under {ROCM}/include")
    exe = str(tmp_path_factory.mktemp("plan") / "conv_plan_cases")
    subprocess.run([gxx, "-O2", "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                    os.path.join(ROOT, "loco-edit_amd", "csrc", "conv_plan.hip"), os.path.join(ROOT, "tests", "c", "conv_plan_cases.cpp"),
                    "-o", exe], check=True)
    keys = [(r["id"], p) for r in so.ROWS for p in r["precs"]]
    text = "".join(so.plan_line(r, p) + "\n" for r in so.ROWS for p in r["precs"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    r = subprocess.run([exe], input=text, env=env, capture_output=True, text=True, timeout=120, check=True)
    chunks = r.stdout.split("case ")[1:]
    assert len(chunks) == len(keys)
    return {k: so.parse_plan(c.split("\n", 1)[1]) for k, c in zip(keys, chunks)}


def test_every_row_reaches_the_route_it_names(plans):
    bad = []
    for r in so.ROWS:
        for p in r["precs"]:
            launches, closing = plans[(r["id"], p)]
            bad += [f"{r['family']} / {r['id']} / {p}: {m}" for m in so.check_route(launches, closing, r)]
    assert not bad, "\n".join(bad)


def test_table_covers_every_route_and_kind():
    assert len({r["id"] for r in so.ROWS}) == len(so.ROWS)
    seen = {(route, r["kind"]) for r in so.ROWS for route in r["routes"]}
    assert seen >= {(route, kind) for route in ("epi", "splitk", "alone") for kind in ("fwd", "tan", "cot")}
    assert {r["kind"] for r in so.ROWS if r["keep"]} == {"fwd", "tan"}
    assert any(len(r["routes"]) == 2 for r in so.ROWS)
    gemm = {r["routes"] for r in so.ROWS if r["kernel"] == "conv_gemm"}      # the DMA-fed GEMM: split (split-K epilogue) and un-split (standalone)
    assert gemm == {("splitk",), ("alone",)}
    c = so.CAT      # one group wholly in A, one wholly in B, one straddling
    cpg = c["C"] // c["G"]
    where = {("A" if (g + 1) * cpg <= c["C1"] else "B" if g * cpg >= c["C1"] else "AB") for g in range(c["G"])}
    assert where == {"A", "B", "AB"}
    assert len({n.id for n in so.NORM_CASES}) == len(so.NORM_CASES)


def test_old_plan_texts_still_parse():
    old = "launch=0 part=0 kernel=conv_mfma_f32<9,2,2,2,2,0> tile=0 nsplit=1 B=2 s0=0 gemm=0 gemm_tm=0 pair=0 Cin2=0 sc_first=0 cot=0\n"
    new = old[:-1] + " stats=epi ntile=4\nstats_all=0 keep_ntile=4\n"
    assert co.parse_plan(old)[0]["tile"] == 0 and len(co.parse_plan(new)) == 1 and co.parse_plan(new)[0]["stats"] == "epi"
    exp = dict(kernel="conv_mfma_f32", tile=0, split=False, tail=0)
    assert not co.check_plan(co.parse_plan(old), exp, co.case(9, 8, 8, 8, B=2))
    assert not co.check_plan(co.parse_plan(new), exp, co.case(9, 8, 8, 8, B=2))
    assert so.parse_plan(new)[1] == dict(stats_all=0, keep_ntile=4)


# ---- the restatements stay inside tau, planted errors do not --------------------------------------------------------------------

C_, G_, H_, W_, B_ = 16, 4, 16, 32, 3
CPG_ = C_ // G_
HW_ = H_ * W_


def _data(level, seed=11):
    g = torch.Generator().manual_seed(seed)
    no = so.norm_operands(C_, G_, g)
    x = so.tensor_operand(B_, C_, H_, W_, G_, g, level)
    p = so.primal_operands(C_, H_, W_, G_, no["gamma"], no["beta"], EPS, g, level)
    p = {k: v.unsqueeze(0) for k, v in p.items()}
    return no, x, p


def _fwd_ok(mr32, x, no, nt, ss=(None, None)):
    tol = so.tol_fwd(x, G_, no["gamma"], no["beta"], EPS, nt, *ss)
    sc32, sh32 = so.scsh32(mr32, no["gamma"], no["beta"], CPG_, *ss)
    res = so.check_fwd(mr32, sc32, sh32, tol)
    for k in ("mean", "rstd", "sc", "sh"):      # no bound's scale vanishes
        assert float(tol[k].min()) > 1e-12, k
    return all(ok for _, ok, _, _ in res), "; ".join(f"{n}: {m}" for n, ok, _, m in res if not ok)


@pytest.mark.parametrize("level", so.LEVELS)
def test_forward_routes_in_fp32_stay_inside_tau(level):
    no, x, _ = _data(level)
    ok, msg = _fwd_ok(so.route32_fwd_alone(x, G_, EPS), x, no, 0)
    assert ok, f"standalone: {msg}"
    for NT in (64, 256):
        ok, msg = _fwd_ok(so.route32_fwd_epi([so.part32_fwd(x, NT)], HW_, G_, EPS), x, no, NT)
        assert ok, f"epilogue NT = {NT}: {msg}"
    nt = torch.cat([torch.full((B_, 6), 256), torch.full((B_, 10), 64)], 1)      # cat: group 1 straddles the parts
    ok, msg = _fwd_ok(so.route32_fwd_epi([so.part32_fwd(x[:, :6], 256), so.part32_fwd(x[:, 6:], 64)], HW_, G_, EPS), x, no, nt)
    assert ok, f"cat: {msg}"
    g = torch.Generator().manual_seed(2)
    ss = (so._f32(0.2 * torch.randn(C_, generator=g, dtype=D)), so._f32(0.3 * torch.randn(C_, generator=g, dtype=D)))
    ok, msg = _fwd_ok(so.route32_fwd_epi([so.part32_fwd(x, 64)], HW_, G_, EPS), x, no, 64, ss)
    assert ok, f"scale-shift: {msg}"


def test_forward_standalone_with_slices_stays_inside_tau():
    g = torch.Generator().manual_seed(4)
    x = so.tensor_operand(1, 16, 64, 64, 2, g, 50.0)       # cpg HW = 32768: two slices
    no = so.norm_operands(16, 2, g)
    assert so.gn_nsplit(8 * 4096, 2) == 2
    tol = so.tol_fwd(x, 2, no["gamma"], no["beta"], EPS, 0)
    mr32 = so.route32_fwd_alone(x, 2, EPS)
    assert so.worst(mr32[..., 1], tol["ref"]["mr"][..., 1], tol["rstd"], "(b, g)")[0]
    for plant in ("tile_left_out", "no_between"):
        bad = so.route32_fwd_alone(x, 2, EPS, plant=plant)
        assert not so.worst(bad[..., 1], tol["ref"]["mr"][..., 1], tol["rstd"], "(b, g)")[0], plant


@pytest.mark.parametrize("level", so.LEVELS)
def test_tangent_and_cotangent_routes_in_fp32_stay_inside_tau(level):
    no, x, p = _data(level)
    args = (p["prim"], p["sc"], p["sh"], p["mr"], CPG_)
    for kind in (0, 1, 2):
        tol = so.tol_lin(kind, x, *args)
        assert float(tol["m1"].min()) > 1e-12 and float(tol["m2"].min()) > 1e-12
        res = so.check_lin(so.route32_lin_alone(kind, x, *args), tol)
        assert all(ok for _, ok, _, _ in res), f"standalone kind {kind}: {[m for _, ok, _, m in res if not ok]}"
    for NT in (64, 256):
        tol = so.tol_lin(0, x, *args, nt=NT)
        res = so.check_lin(so.route32_lin_epi(so.ST_TAN, [so.part32_tan(x, p["prim"][0], NT)], HW_, G_, p["mr"]), tol)
        assert all(ok for _, ok, _, _ in res), f"tangent epilogue NT = {NT}: {[m for _, ok, _, m in res if not ok]}"
        tol = so.tol_lin(1, x, *args, nt=NT)
        parts = [so.part32_cot(x, p["prim"][0], p["sc"][0], p["sh"][0], p["mr"][0], CPG_, NT)]
        res = so.check_lin(so.route32_lin_epi(so.ST_COT, parts, HW_, G_, p["mr"]), tol)
        assert all(ok for _, ok, _, _ in res), f"cotangent epilogue NT = {NT}: {[m for _, ok, _, m in res if not ok]}"
    nt = torch.cat([torch.full((B_, 6), 256), torch.full((B_, 10), 64)], 1)
    tol = so.tol_lin(0, x, *args, nt=nt)
    parts = [so.part32_tan(x[:, :6], p["prim"][0, :6], 256), so.part32_tan(x[:, 6:], p["prim"][0, 6:], 64)]
    res = so.check_lin(so.route32_lin_epi(so.ST_TAN, parts, HW_, G_, p["mr"]), tol)
    assert all(ok for _, ok, _, _ in res), f"tangent cat: {[m for _, ok, _, m in res if not ok]}"


def test_the_raw_sum_scale_grows_with_the_offset_and_the_others_do_not():
    """the statement under test: A of the tangent m2 from raw sums follows |mean| / std, A of the routes that sum xhat z does not"""
    A = {}
    x = _data(0.0)[1]      # one tangent for all levels: the offset is the primal's
    for level in so.LEVELS:
        p = _data(level)[2]
        args = (p["prim"], p["sc"], p["sh"], p["mr"], CPG_)
        A[level] = (float(so.tol_lin(0, x, *args, nt=64)["A2"][:, 0].mean()), float(so.tol_lin(0, x, *args, nt=0)["A2"][:, 0].mean()))
    assert A[1000.0][0] > 100 * A[0.0][0] and A[50.0][0] > 5 * A[0.0][0]
    assert A[1000.0][1] < 3 * A[0.0][1]
    no, x, _ = _data(1000.0)
    k_epi = so.tol_fwd(x, G_, no["gamma"], no["beta"], EPS, 64)["kappa"]
    assert float(k_epi.max()) < 10.0      # the pivot keeps the epilogue's M2 conditioned at |mean| / std = 1000


PLANTS_FWD = ["tile_left_out", "no_between", "one_tile_size", "next_sample", "before_residual"]
PLANTS_LIN = ["tile_left_out", "no_mean_sum", "neighbour_group", "next_sample", "tc_unscaled"]


@pytest.mark.parametrize("level", so.LEVELS)
@pytest.mark.parametrize("plant", PLANTS_FWD)
def test_planted_forward_errors_are_rejected(plant, level):
    no, x, _ = _data(level)
    nt = torch.cat([torch.full((B_, 6), 256), torch.full((B_, 10), 64)], 1)
    parts = lambda t: [so.part32_fwd(t[:, :6], 256), so.part32_fwd(t[:, 6:], 64)]
    if plant == "next_sample":
        mr32 = torch.roll(so.route32_fwd_epi(parts(x), HW_, G_, EPS), 1, dims=0)
    elif plant == "before_residual":      # the tensor is x = conv + res; the statistics saw conv alone
        g = torch.Generator().manual_seed(9)
        res = so._f32(0.5 * torch.randn(B_, C_, H_, W_, generator=g, dtype=D))
        mr32 = so.route32_fwd_epi(parts(so._f32(x - res)), HW_, G_, EPS)
    else:
        mr32 = so.route32_fwd_epi(parts(x), HW_, G_, EPS, plant=plant)
    ok, msg = _fwd_ok(mr32, x, no, nt)
    assert not ok, f"{plant} passes at level {level}"


@pytest.mark.parametrize("level", so.LEVELS)
@pytest.mark.parametrize("plant", PLANTS_LIN)
def test_planted_tangent_and_cotangent_errors_are_rejected(plant, level):
    no, x, p = _data(level)
    args = (p["prim"], p["sc"], p["sh"], p["mr"], CPG_)
    if plant == "tc_unscaled":      # bit equality of the per-channel expansion: the cotangent kind carries rstd
        tst = so.route32_lin_alone(1, x, *args)
        good, bad = so.tc_of(tst, p["mr"], CPG_, True), so.tc_of(tst, p["mr"], CPG_, False)
        assert so.tc_mismatch(good, tst, p["mr"], CPG_, True) == 0
        assert so.tc_mismatch(bad, tst, p["mr"], CPG_, True) > 0
        assert so.tc_mismatch(so.tc_of(tst, p["mr"], CPG_, False), tst, p["mr"], CPG_, False) == 0
        return
    tol = so.tol_lin(0, x, *args, nt=64)
    parts = [so.part32_tan(x, p["prim"][0], 64)]
    if plant == "next_sample":
        got = torch.roll(so.route32_lin_epi(so.ST_TAN, parts, HW_, G_, p["mr"]), 1, dims=0)
    else:
        got = so.route32_lin_epi(so.ST_TAN, parts, HW_, G_, p["mr"], plant=plant)
    res = so.check_lin(got, tol)
    assert not all(ok for _, ok, _, _ in res), f"{plant} passes at level {level} (tangent epilogue)"
    if plant in ("neighbour_group", "tile_left_out"):      # the same on the routes that sum xhat z
        tolc = so.tol_lin(1, x, *args, nt=64)
        partsc = [so.part32_cot(x, p["prim"][0], p["sc"][0], p["sh"][0], p["mr"][0], CPG_, 64)]
        if plant == "tile_left_out":
            resc = so.check_lin(so.route32_lin_epi(so.ST_COT, partsc, HW_, G_, p["mr"], plant=plant), tolc)
        else:
            resc = so.check_lin(so.route32_lin_alone(1, x, *args, plant=plant), so.tol_lin(1, x, *args))
        assert not all(ok for _, ok, _, _ in resc), f"{plant} passes at level {level} (cotangent)"


def test_apply_tolerance_holds_in_fp32_and_rejects_a_dropped_m2():
    no, x, p = _data(0.0)
    cpg = CPG_
    tst = so._f32(so.lin_stats(so.z_of(1, x, p["prim"], p["sc"], p["sh"], p["mr"], cpg), p["prim"], p["mr"], cpg))
    kw = dict(d=x, mr=p["mr"], tst=tst)
    xp = p["prim"].expand(B_, -1, -1, -1)
    tau, A = so.tol_apply(2, xp, p["sc"], p["sh"], cpg, **kw)
    ref = so.apply(2, xp, p["sc"], p["sh"], cpg, **kw)
    f = lambda t: t.to(torch.float32)
    r32 = so.apply(2, f(xp), f(p["sc"]), f(p["sh"]), cpg, d=f(x), mr=f(p["mr"]), tst=f(tst)).to(D)
    assert float(((r32 - ref).abs() / A).max()) <= tau
    t0 = tst.clone()
    t0[..., 1] = 0
    bad = so.apply(2, xp, p["sc"], p["sh"], cpg, d=x, mr=p["mr"], tst=t0)
    assert float(((bad - ref).abs() / A).max()) > tau
    assert float(A.min()) >= 1e-6 * float(A.max())


@pytest.mark.parametrize("act", [so.ACT_SILU, so.ACT_GELU])
def test_record_and_token_norm_bounds_hold_in_fp32_and_reject_planted_errors(act):
    no, x, p = _data(50.0)
    prim, sc, sh, mr = p["prim"][0], p["sc"][0], p["sh"][0], p["mr"][0]
    ref, tau = so.tol_records(prim, sc, sh, mr, CPG_, act)
    f = lambda t: t.to(torch.float32)
    r32 = so.records(f(prim), f(sc), f(sh), f(mr), CPG_, act).to(D)
    assert so.worst(r32, ref, tau, "(c, y, x, k)")[0]
    bad = r32.clone()      # xhat of one group against its neighbour's {mean, rstd}
    bad[:CPG_, ..., 1] = so.records(prim, sc, sh, torch.roll(mr, 1, 0), CPG_, act)[:CPG_, ..., 1]
    assert not so.worst(bad, ref, tau, "(c, y, x, k)")[0]
    bad = r32.clone()      # S without the channel's gain
    bad[..., 0] = bad[..., 0] / sc.view(-1, 1, 1)
    assert not so.worst(bad, ref, tau, "(c, y, x, k)")[0]
    # token-major norm: {mean, rstd} from double, rounded; the elementwise expression in fp32
    g = torch.Generator().manual_seed(6)
    tok = so._f32(torch.randn(77, 64, generator=g, dtype=D) * (0.5 + torch.rand(64, generator=g, dtype=D)) + 3.0 * torch.randn(64, generator=g, dtype=D))
    nn = so.norm_operands(64, 4, g)
    for G in (4, 32):
        ref, tau = so.tol_ctx(tok, G, nn["gamma"], nn["beta"], EPS)
        assert float(tau.min()) > 1e-12
        t = tok.reshape(77, G, 64 // G)
        mean = t.mean((0, 2), keepdim=True)
        rstd = 1 / torch.sqrt(((t - mean) ** 2).mean((0, 2), keepdim=True) + EPS)
        o32 = (((f(t) - f(mean)) * f(rstd)).reshape(77, 64) * f(nn["gamma"]) + f(nn["beta"])).to(D)
        assert so.worst(o32, ref, tau, "(token, channel)")[0]
        # statistics over 76 of the 77 tokens
        m76 = t[:76].mean((0, 2), keepdim=True)
        r76 = 1 / torch.sqrt(((t[:76] - m76) ** 2).mean((0, 2), keepdim=True) + EPS)
        bad = ((t - m76) * r76).reshape(77, 64) * nn["gamma"] + nn["beta"]
        assert not so.worst(bad, ref, tau, "(token, channel)")[0]
