"""GPU: single conv launches of every kernel family against float64 (loco_debug_conv of the diagnostics build vs tests/conv_oracle.py).

Every row of conv_oracle.ROWS, under every precision it lists, is one launch through run_conv -> plan_conv on seeded operands
(per-sample data, per-channel offsets of a few units, statistics arrays from the float64 statistics of the primal).  Per case:
  1. the plan text names the kernel family the table claims (conv_oracle.check_plan) -- a planner change that reroutes a case
     fails here instead of silently testing another kernel;
  2. |out - ref| <= tau A + 1e-30 on EVERY output element, tau from the reference alone (conv_oracle.tolerance: 4 x (format +
     accumulation + prologue)); the message names the worst element's (b, cout, y, x);
  3. `out` is pre-filled with NaN (with a second random tensor where accumulate = 1, which the reference adds once): an element
     that is not written, or is accumulated twice, fails 2.
The rows whose output map no conv kernel can walk (48 x 48, 128 x 144: DESIGN.md) must be REFUSED by loco_debug_conv.

One child process owns the engine (hip.py binds one library per process; the diagnostics build is chosen through LOCO_HIP_LIB)
and runs the whole table; no environment switch is set: the kernels under test are the product's defaults.  The child is this
file run as a script:   LOCO_HIP_LIB=.../libloco_hip_diag.so python tests/test_gpu_conv_oracle.py --worker out.json

Measured on the MI355X, max |out - ref| / A per precision over the modes' cases (tau of the same cases alongside; margin 4):
  precision  mode          cases  max |out - ref| / A   tau (min ... max)        worst share of tau
  f32        0 raw            37  2.78e-07             8.3e-06 ... 1.1e-03    0.030
  f32        1 GN+SiLU        11  3.76e-07             7.1e-05 ... 1.1e-03    0.005
  f32        2 GN              3  1.20e-07             2.9e-05 ... 3.3e-05    0.004
  f32        3 tangent         9  2.03e-07             7.1e-05 ... 1.5e-04    0.003
  f32        4 cotangent      10  1.19e-07             7.1e-05 ... 1.4e-04    0.002
  f32        5 GN+GELU         1  2.62e-07             1.1e-04 ... 1.1e-04    0.002
  bf16x3     0 raw            47  7.76e-06             3.0e-05 ... 1.1e-03    0.194
  bf16x3     1 GN+SiLU         9  5.58e-06             7.6e-05 ... 1.1e-03    0.039
  bf16x3     2 GN              4  3.52e-06             4.0e-05 ... 8.5e-05    0.088
  bf16x3     3 tangent         7  3.21e-06             7.5e-05 ... 1.6e-04    0.020
  bf16x3     4 cotangent       6  1.39e-06             7.5e-05 ... 1.4e-04    0.019
  bf16x3     5 GN+GELU         1  2.35e-06             1.1e-04 ... 1.1e-04    0.022
  f16        0 raw            31  3.95e-04             4.3e-04 ... 1.6e-03    0.249
  f16        1 GN+SiLU         7  2.36e-04             3.0e-04 ... 1.2e-03    0.440
  f16        2 GN              3  1.94e-04             5.6e-04 ... 6.3e-04    0.319
  f16        3 tangent         5  1.57e-04             2.4e-04 ... 6.3e-04    0.278
  f16        4 cotangent       5  7.85e-05             2.8e-04 ... 3.5e-04    0.241
  f16        5 GN+GELU         1  1.35e-04             2.7e-04 ... 2.7e-04    0.505
(ratios from the first run, taken against the A of that run: A of the prologue modes has grown since, so for modes 1 - 5 they are upper bounds)
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

KEYS = [(r["id"], p) for r in co.ROWS for p in r["precs"]]
DESC_FIELDS = ("Cin", "Cout", "B", "taps", "stride", "upsample", "zins", "mode", "cpg", "transposed", "accumulate", "in_arena", "pad", "Cin2")
OPERANDS = ("weight", "bias", "in", "bias2", "res", "prim", "sc", "sh", "mr", "gamma", "tst", "tc", "in2", "w2", "bias2nd",
            "cot_d", "cot_prim", "cot_sc", "cot_sh", "cot_mr", "cot_tc")
HOST = ("weight", "bias", "w2", "bias2nd")


def _run_case(eng, torch, row, prec, cache):
    d = row["case"]
    if row["id"] not in cache:
        cache.clear()
        ops = co.make_operands(d)
        cache[row["id"]] = dict(ops=ops, dev={k: v.to(torch.float32).cuda() for k, v in ops.items() if k in OPERANDS and k not in HOST})
    ops, dev = cache[row["id"]]["ops"], cache[row["id"]]["dev"]
    ho, wo = co.out_hw(d)
    kw = {k: d[k] for k in DESC_FIELDS}
    kw.update(Hin=d["H"], Win=d["W"], res_scale=d["res_scale"])
    if d["cot"]:
        kw["cot_cpg"] = d["cot_cpg"]
    for k in OPERANDS:
        if k in ops:
            kw[k] = ops[k].to(torch.float32) if k in HOST else dev[k]
    if d["accumulate"]:
        out = ops["out0"].to(torch.float32).cuda()
    else:
        out = torch.full((d["B"], d["Cout"], ho, wo), float("nan"), dtype=torch.float32, device="cuda")
    eng.set_precision(prec)
    res = dict(id=row["id"], prec=prec, family=row["family"], mode=d["mode"])
    t0 = time.time()
    if row["refused"]:
        try:
            eng.debug_conv(out, **kw)
            res.update(refused=False, error="loco_debug_conv launched a map no conv kernel can walk")
        except RuntimeError as e:
            res.update(refused="tile geometry" in str(e), error=str(e))
        return res
    plan, rode = eng.debug_conv(out, **kw)
    torch.cuda.synchronize()
    res["gpu_s"] = time.time() - t0
    got = out.cpu().to(torch.float64)
    res["plan_bad"] = co.check_plan(plan, row["expect"][prec], d)
    res["plan"] = [p["kernel"] for p in plan]
    res["unwritten"] = int(torch.isnan(got).sum())
    if d["cot"] and not rode:      # declined: the plain result
        d = dict(d, cot=False)
        ops = {k: v for k, v in ops.items() if not k.startswith("cot_")}
    if row["probes"]:
        d, ops = co.sub_case(d, ops, list(row["probes"]))
        got = got.index_select(0, torch.tensor(list(row["probes"])))
    c = cache[row["id"]]
    if ("ref", d["cot"]) not in c:
        c[("ref", d["cot"])] = (co.reference(d, ops), co.magnitude(d, ops))
    ref, A = c[("ref", d["cot"])]
    tol = co.tolerance(d, ops, prec, ref, A)
    ok, msg = co.worst(got, ref, A, tol["tau"])
    res.update(ok=ok, msg=msg, measured=float(((got - ref).abs() / A).nan_to_num(nan=float("inf")).max()), **tol)
    res["total_s"] = time.time() - t0
    return res


def _worker(path):
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import CELEBA_DDPM, synth_params
    torch.set_num_threads(min(16, torch.get_num_threads()))
    eng = H.LocoEngine(CELEBA_DDPM, max_batch=10)
    eng.load_state_dict(synth_params(CELEBA_DDPM, 0))
    results, cache = [], {}
    for row in co.ROWS:
        for prec in row["precs"]:
            r = _run_case(eng, torch, row, prec, cache)
            print(json.dumps({k: v for k, v in r.items() if k != "msg"}), flush=True)
            results.append(r)
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
    """the whole table on one engine of the diagnostics build, in one child process"""
    out = str(tmp_path_factory.mktemp("conv_oracle") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env["LOCO_HIP_LIB"] = _diag_lib()
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out], env=env, capture_output=True, text=True, timeout=1500)
    done = r.stdout.count("\n")
    assert r.returncode == 0, f"the worker ended with {r.returncode} after {done} of {len(KEYS)} cases:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    with open(out) as f:
        return {(x["id"], x["prec"]): x for x in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("cid, prec", KEYS, ids=[f"{c}-{p}" for c, p in KEYS])
def test_conv_launch_matches_float64(results, cid, prec):
    r = results[(cid, prec)]
    if "refused" in r:
        assert r["refused"], r["error"]
        return
    assert not r["plan_bad"], f"{r['family']}: {r['plan_bad']} (planned {r['plan']})"
    assert r["unwritten"] == 0, f"{r['unwritten']} output elements were never written (NaN sentinel left); {r['msg']}"
    print(f"{cid} {prec}: max |out - ref| / A = {r['measured']:.3e}, tau = {r['tau']:.3e} "
          f"(format {r['format']:.2e} accumulation {r['accumulation']:.2e} prologue {r['prologue']:.2e})")
    assert r["ok"], f"{r['family']} ({', '.join(r['plan'])}): {r['msg']}"
    assert r["total_s"] < 20.0, f"the case took {r['total_s']:.1f} s"
