"""GPU: the polyphase up / down-sampling conv launches (conv_bf16_kernel.h TAPS = 4, planned by conv_plan.hip conv_poly_ok) as
single launches through loco_debug_conv of the diagnostics build against float64, exactly as tests/test_gpu_conv_oracle.py does
(conv_oracle.reference / magnitude / tolerance / worst; the tolerance comes from the reference alone, margin 4), and the whole
network's adjointness with the polyphase routes against a child process on the 3x3 routes (LOCO_POLYPHASE=0).

Cases (Cin = 48: three 16-channel chunks, an odd count; Cout = 128: one row phase = two 128-virtual-cout tiles; low-resolution maps
of 64 x 64 and 32 x 128 to tell rows from columns; B = 2 and 3; bf16x3 and f16):
  - upsample = 1 (the up conv's forward / tangent form, with bias);
  - zins = 1, transposed = 1 with pad 2 and pad 1, with and without accumulate (the stride-2 conv's data gradient);
  - pool2 = 1, transposed = 1 (the up conv's cotangent: transposed 3x3 conv + 2x2 sum-pool as ONE 4x4 stride-2 launch) against the
    float64 4x4 stride-2 conv with W4 = w (*) ones(2, 2), with and without accumulate; tau and A are the 3x3 launch's own (A summed
    over the pooled pixels: the bound of a sum of four outputs is the sum of their bounds);
  - one ineligible neighbour each (Cout = 64) that must stay on today's 3x3 kernel (the pooled one: the 3x3 launch + pooling pass);
  - one launch with a tangent statistics request: the {m1, m2} merged from the row partials its epilogue kept must equal the
    standalone pass over the finished tensor (loco_conv_desc::st_out) to 3e-5 of the group's mean |d| / mean |xhat d| -- the bound
    of the fused-vs-standalone statistics tests in tests/test_gpu_parity.py; both routes sum the same fp32 tensor.
`out` is pre-filled with NaN (with the tensor the reference adds once where accumulate = 1): an element that is not written, or
written twice on top of itself, fails the comparison.

One child process owns the engine of the diagnostics build and runs all cases (hip.py binds one library per process); two more
run the adjointness check, one per setting of LOCO_POLYPHASE (the switch is read once per process).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_oracle as co      # noqa: E402

POLY = {"bf16x3": "conv_mfma_bf16x3<4,2,4,2,2,0>", "f16": "conv_mfma_f16<4,2,4,2,2,0>"}
POOLED = {p: k + "+pool" for p, k in POLY.items()}
TODAY = {"bf16x3": "conv_mfma_bf16x3<9,2,4,2,2,0>", "f16": "conv_mfma_f16<9,2,4,2,2,0>"}
PRECS = ("bf16x3", "f16")


def _cases():
    c = {}
    c["up_64x64_B2"] = (co.case(9, 48, 128, 64, 64, B=2, upsample=1), True)
    c["up_32x128_B3"] = (co.case(9, 48, 128, 32, 128, B=3, upsample=1), True)
    c["zins_pad2_64x64_B3"] = (co.case(9, 48, 128, 64, 64, B=3, zins=1, transposed=1, pad=2, bias=False), True)
    c["zins_pad2_32x128_B2_acc"] = (co.case(9, 48, 128, 32, 128, B=2, zins=1, transposed=1, pad=2, accumulate=1, bias=False), True)
    c["zins_pad1_64x64_B2_acc"] = (co.case(9, 48, 128, 64, 64, B=2, zins=1, transposed=1, pad=1, accumulate=1, bias=False), True)
    c["zins_pad1_32x128_B3"] = (co.case(9, 48, 128, 32, 128, B=3, zins=1, transposed=1, pad=1, bias=False), True)
    c["up_64x64_B2_cout64"] = (co.case(9, 48, 64, 64, 64, B=2, upsample=1), False)      # the ineligible neighbour
    # conv + pool: H x W is the launch's INPUT map (twice the low-resolution map); `pool_acc`: accumulate into the pooled output
    c["pool_64x64_B2"] = (dict(co.case(9, 48, 128, 128, 128, B=2, transposed=1, bias=False), pool2=1, pool_acc=0), True)
    c["pool_32x128_B3_acc"] = (dict(co.case(9, 48, 128, 64, 256, B=3, transposed=1, bias=False), pool2=1, pool_acc=1), True)
    c["pool_64x64_B2_cout64"] = (dict(co.case(9, 48, 64, 128, 128, B=2, transposed=1, bias=False), pool2=1, pool_acc=0), False)
    return c


CASES = _cases()
STATS_CASE, STATS_CPG = "up_64x64_B2", 16
KEYS = [(cid, p) for cid in CASES for p in PRECS]
DESC_FIELDS = ("Cin", "Cout", "B", "taps", "stride", "upsample", "zins", "mode", "cpg", "transposed", "accumulate", "in_arena", "pad", "Cin2")


def _pooled_reference(torch, d, ops):
    """(ref, A) of conv + 2x2 sum-pool: the float64 4x4 stride-2 conv; A = the 3x3 launch's magnitude summed over the pooled pixels"""
    import torch.nn.functional as F
    w = ops["weight"].flip(2, 3).transpose(0, 1)      # the launch's correlation operator (transposed = 1)
    w4 = w.new_zeros(w.shape[0], w.shape[1], 4, 4)
    for a in range(2):
        for b in range(2):
            w4[:, :, a:a + 3, b:b + 3] += w
    ref = F.conv2d(ops["in"], w4, stride=2, padding=1)
    A = 4.0 * F.avg_pool2d(co.magnitude(d, ops), 2)
    if d["pool_acc"]:
        ref, A = ref + ops["pool_out0"], A + ops["pool_out0"].abs()
    return ref, A


def _launch(eng, torch, d, ops, prec, extra=None):
    ho, wo = co.out_hw(d)
    if d.get("pool2"):
        ho, wo = ho // 2, wo // 2
        extra = dict(extra or {}, pool2=1, accumulate=d["pool_acc"])
    kw = {k: d[k] for k in DESC_FIELDS}
    kw.update(Hin=d["H"], Win=d["W"], res_scale=d["res_scale"], weight=ops["weight"].to(torch.float32))
    if "bias" in ops:
        kw["bias"] = ops["bias"].to(torch.float32)
    kw["in"] = ops["in"].to(torch.float32).cuda()
    kw.update(extra or {})
    if d.get("pool_acc"):
        out = ops["pool_out0"].to(torch.float32).cuda()
    elif d["accumulate"]:
        out = ops["out0"].to(torch.float32).cuda()
    else:
        out = torch.full((d["B"], d["Cout"], ho, wo), float("nan"), dtype=torch.float32, device="cuda")
    eng.set_precision(prec)
    plan, _ = eng.debug_conv(out, **kw)
    torch.cuda.synchronize()
    return out, plan


def _worker(path):
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import CELEBA_DDPM, synth_params
    torch.set_num_threads(min(16, torch.get_num_threads()))
    eng = H.LocoEngine(CELEBA_DDPM, max_batch=10)
    eng.load_state_dict(synth_params(CELEBA_DDPM, 0))
    results = []
    for cid, (d, eligible) in CASES.items():
        ops = co.make_operands(d)
        if d.get("pool2"):
            g = torch.Generator().manual_seed(91)
            ops["pool_out0"] = (torch.randn(d["B"], d["Cout"], d["H"] // 2, d["W"] // 2, generator=g, dtype=torch.float64) + 1.5).float().double()
            ref, A = _pooled_reference(torch, d, ops)
            ref_hi, A_hi = co.reference(d, ops), co.magnitude(d, ops)
        else:
            ref, A = co.reference(d, ops), co.magnitude(d, ops)
            ref_hi, A_hi = ref, A
        for prec in PRECS:
            out, plan = _launch(eng, torch, d, ops, prec)
            got = out.cpu().to(torch.float64)
            tol = co.tolerance(d, ops, prec, ref_hi, A_hi)
            ok, msg = co.worst(got, ref, A, tol["tau"])
            r = dict(id=cid, prec=prec, kernels=[p["kernel"] for p in plan], nsplit=[p["nsplit"] for p in plan],
                     unwritten=int(torch.isnan(got).sum()), ok=ok, msg=msg,
                     measured=float(((got - ref).abs() / A).nan_to_num(nan=float("inf")).max()), **tol)
            if cid == STATS_CASE:
                # the same launch with the tangent statistics request of one part of a concatenation
                g = torch.Generator().manual_seed(77)
                C, (ho, wo), B = d["Cout"], co.out_hw(d), d["B"]
                G = C // STATS_CPG
                prim = (torch.randn(C, ho, wo, generator=g, dtype=torch.float64) + 2.0 * torch.randn(C, 1, 1, generator=g, dtype=torch.float64)).float()
                pg = prim.double().reshape(G, -1)
                mean, rstd = pg.mean(1), 1.0 / torch.sqrt(pg.var(1, unbiased=False) + 1e-6)
                mr = torch.stack([mean, rstd], 1).float().contiguous()
                st_out = torch.zeros(2, B, G, 2, dtype=torch.float32, device="cuda")
                out2, plan2 = _launch(eng, torch, d, ops, prec, extra=dict(st_prim=prim.cuda(), st_mr=mr.cuda(), st_out=st_out, st_cpg=STATS_CPG))
                so = st_out.cpu().double()
                dd = out2.cpu().double().reshape(B, G, -1)
                xh = ((prim.double().reshape(G, -1) - mr[:, :1].double()) * mr[:, 1:].double()).unsqueeze(0)
                scale = torch.stack([dd.abs().mean(2), (dd * xh).abs().mean(2)], 2)      # mean |d|, mean |xhat d| per (sample, group)
                exact = torch.stack([dd.mean(2), (dd * xh).mean(2)], 2)
                r.update(stats_kernel=[p["kernel"] for p in plan2], stats_same_out=bool(torch.equal(out2, out)),
                         stats_nan=int(torch.isnan(so).sum()),
                         stats_fused_vs_alone=float(((so[0] - so[1]).abs() / scale).nan_to_num(nan=float("inf")).max()),
                         stats_alone_vs_f64=float(((so[1] - exact).abs() / scale).nan_to_num(nan=float("inf")).max()))
            print(json.dumps({k: v for k, v in r.items() if k != "msg"}), flush=True)
            results.append(r)
    with open(path, "w") as f:
        json.dump(results, f)


def _adjoint_worker(path):
    """defect |<Jv, u> - <v, J^T u>| / (|Jv| |u|) of the CelebA-HQ DDPM network, synthetic weights, 2 probes, default arithmetic"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import loco_oracle as orc
    from loco_edit_amd.config import CELEBA_DDPM, synth_params
    from loco_edit_amd.hip import LocoEngine
    cfg = CELEBA_DDPM
    eng = LocoEngine(cfg, max_batch=4, device=torch.device("cuda:0"))
    eng.load_state_dict(synth_params(cfg, 0))
    s = orc.Scheduler()
    s.set_timesteps(100)
    t = s.timesteps[40]
    x = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(1)).cuda()
    mask = torch.zeros(3, 256, 256, dtype=torch.bool)
    mask[:, 110:130, 70:110] = True
    eng.pmp_primal(x, float(t), float(s.alpha_at(t)), mask.cuda())
    V = torch.randn(2, cfg.n, generator=torch.Generator().manual_seed(5)).cuda()
    U = torch.randn(2, cfg.n, generator=torch.Generator().manual_seed(6)).cuda() * mask.reshape(1, -1).cuda()
    JV, JtU = eng.pmp_jvp(V).double(), eng.pmp_vjp(U).double()
    lhs, rhs = (JV * U.double()).sum(dim=1), (V.double() * JtU).sum(dim=1)
    defect = float(((lhs - rhs).abs() / (JV.norm(dim=1) * U.double().norm(dim=1))).max())
    with open(path, "w") as f:
        json.dump(dict(defect=defect, jv_norm=float(JV.norm()), finite=bool(torch.isfinite(JV).all() and torch.isfinite(JtU).all())), f)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] in ("--worker", "--adjoint"):
    (_worker if sys.argv[1] == "--worker" else _adjoint_worker)(sys.argv[2])
    sys.exit(0)


def _child(args, env_extra, timeout):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env.update(env_extra)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"the worker ended with {r.returncode}:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    return r


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    lib = os.path.join(ROOT, "loco-edit_amd", "libloco_hip_diag.so")
    assert os.path.exists(lib), "libloco_hip_diag.so is missing: run `make -C loco-edit_amd/csrc diag` (or __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("polyphase") / "results.json")
    _child(["--worker", out], {"LOCO_HIP_LIB": lib}, 600)
    with open(out) as f:
        return {(x["id"], x["prec"]): x for x in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("cid, prec", KEYS, ids=[f"{c}-{p}" for c, p in KEYS])
def test_polyphase_launch_matches_float64(results, cid, prec):
    r = results[(cid, prec)]
    eligible = CASES[cid][1]
    want = (POOLED[prec] if CASES[cid][0].get("pool2") else POLY[prec]) if eligible else TODAY[prec]
    assert len(r["kernels"]) == 1 and r["kernels"][0] == want and r["nsplit"] == [1], f"planned {r['kernels']} (nsplit {r['nsplit']}), expected {want}"
    assert r["unwritten"] == 0, f"{r['unwritten']} output elements were never written (NaN sentinel left); {r['msg']}"
    print(f"{cid} {prec}: max |out - ref| / A = {r['measured']:.3e}, tau = {r['tau']:.3e}")
    assert r["ok"], f"{r['kernels']}: {r['msg']}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_polyphase_epilogue_statistics_equal_the_standalone_pass(results, prec):
    r = results[(STATS_CASE, prec)]
    assert POLY[prec] in r["stats_kernel"][0], r["stats_kernel"]
    assert r["stats_same_out"], "the statistics request changed the launch's output"
    assert r["stats_nan"] == 0, "the launch kept no partials (or the standalone pass left NaN)"
    print(f"{prec}: fused vs standalone {r['stats_fused_vs_alone']:.2e}, standalone vs float64 {r['stats_alone_vs_f64']:.2e} (of mean |d|, mean |xhat d|)")
    assert r["stats_fused_vs_alone"] < 3e-5


@pytest.mark.gpu
def test_network_adjointness_with_polyphase_routes(tmp_path):
    """|<Jv, u> - <v, J^T u>| / (|Jv| |u|), CelebA-HQ DDPM at 256 x 256, synthetic weights, 2 probes, bf16x3: the defect with the
    polyphase routes must not exceed twice the defect of a child process on the 3x3 routes (LOCO_POLYPHASE=0), same inputs.
    Measured on the MI355X: 1.443e-07 with the polyphase routes, 1.290e-07 on the 3x3 routes (profiles/r07_experiments.md)."""
    res = {}
    for mode in ("1", "0"):
        out = str(tmp_path / f"adjoint_{mode}.json")
        _child(["--adjoint", out], {"LOCO_POLYPHASE": mode}, 600)
        with open(out) as f:
            res[mode] = json.load(f)
    print(f"adjointness defect: polyphase {res['1']['defect']:.3e}, 3x3 routes {res['0']['defect']:.3e}")
    assert res["1"]["finite"] and res["0"]["finite"]
    assert res["1"]["defect"] <= 2.0 * res["0"]["defect"]
