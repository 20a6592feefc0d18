"""GPU: single GEMM launches of every route against float64 (loco_debug_gemm of the diagnostics build vs tests/gemm_oracle.py).

Every row of gemm_oracle.CASES is one call of loco_debug_gemm: one call of launch_gemm, launch_gemm_fixed, launch_gemm_bf16x3,
launch_gemm_rec or launch_gemm_pair on seeded operands that live inside wider buffers and are addressed through the row's strides.
Per case:
  1. the route text equals gemm_oracle.route_of (the launchers' predicates restated in Python) and the table's `expect` column -- a
     changed predicate that reroutes a case fails here instead of silently testing another kernel;
  2. |out - ref| <= tau A_out + 1e-30 on EVERY element, tau from the reference alone (gemm_oracle.tolerance: 4 x (format +
     accumulation + activation)); the message names the worst element's problem, batch, head, m, n;
  3. the output buffer is pre-filled with a NaN of a bit pattern no kernel produces (gemm_oracle.SENTINEL_BITS); the addressed floats
     hold C0 instead where the launch reads them (beta != 0, or the residual aliasing the output);
  4. every float of the output buffer that the strides do NOT address still holds the sentinel's bits afterwards: the 256-float guard
     bands on both sides, row-pitch gaps, the gaps of the transposed and head-interleaved layouts, the pair's second output;
  5. the case stays under 20 s.
The rows of gemm_oracle.REFUSALS must be refused by loco_debug_gemm before any launch, the output untouched.

One child process owns the engine (hip.py binds one library per process; the diagnostics build is chosen through LOCO_HIP_LIB) and
runs the whole table under one timeout.  No LOCO_* switch is set: the parent strips them.  The child is this file run as a script:
    LOCO_HIP_LIB=.../libloco_hip_diag.so python tests/test_gpu_gemm_oracle.py --worker out.json

Measured on the MI355X, max |out - ref| / A_out per (route, op) over the cases (tau of the same cases alongside; margin 4; a pair
counts once per problem slot):
  route                        op           cases  max |out - ref| / A_out  tau (min ... max)      worst share of tau
  gemm_f32_64                  gemm             7  8.71e-07                 1.1e-05 ... 3.3e-05    0.031
  gemm_f32_small               gemm             3  3.17e-07                 3.2e-05 ... 9.7e-05    0.007
  gemm_f32_small_pipe          gemm            11  3.94e-07                 3.2e-05 ... 9.4e-05    0.007
  gemm_f32_pair                gemm_pair        2  2.88e-07                 3.2e-05 ... 6.3e-05    0.007
  gemm_f32_small               gemm_pair        1  2.08e-07                 3.2e-05 ... 3.2e-05    0.006
  gemm_f32_small_pipe          gemm_pair        1  2.88e-07                 6.3e-05 ... 6.3e-05    0.005
  gemm_f32_fixed               gemm_fixed       4  6.74e-07                 2.0e-05 ... 3.5e-05    0.027
  gemm_bf16x3_64               gemm_bf16x3      2  4.26e-06                 2.8e-05 ... 4.3e-05    0.151
  gemm_bf16x3_128              gemm_bf16x3      1  4.52e-06                 3.0e-05 ... 3.0e-05    0.150
  gemm_rec tm 2                gemm_rec         6  1.74e-06                 6.9e-05 ... 7.1e-05    0.025
  gemm_rec tm 4                gemm_rec         1  1.97e-06                 7.2e-05 ... 7.2e-05    0.028
  gemm_rec tm 2 ksplit 4       gemm_rec         1  8.80e-07                 2.5e-04 ... 2.5e-04    0.004
  gemm_rec tm 4 ksplit 4       gemm_rec         1  9.02e-07                 2.5e-04 ... 2.5e-04    0.004
  gemm_rec tm 2 ksplit 3       gemm_rec         2  8.93e-07                 2.5e-04 ... 2.5e-04    0.004
(every case routed as the table expects; no family's worst share of tau is above 0.5; the split launches end in gemm_rec_reduce)
"""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as go      # noqa: E402

CASE = {c["id"]: c for c in go.CASES}
IDS = list(CASE) + [r[0] for r in go.REFUSALS]


def _device_buffers(torch, p, ops):
    """the operands of one problem on the device, and the output buffer: sentinel bits everywhere, C0 on the addressed floats where
    the launch reads them"""
    bufs = {n: ops[n].to(torch.float32).cuda() for n in go.operand_names(p)}
    c = torch.full((go.count_of(p, "C"),), go.SENTINEL_BITS, dtype=torch.int32).view(torch.float32)
    if p["beta"] != 0.0 or p["R"] == "alias":
        m = go.c_mask(p)
        c[m] = ops["C0"].to(torch.float32)[m]
    bufs["C"] = c.cuda()
    return bufs


def _run_case(eng, torch, case):
    res = dict(id=case["id"], family=case["family"], op=case["op"], act=case["act"])
    ops = go.make_operands(case)
    t0 = time.time()
    bufs = [_device_buffers(torch, p, o) for p, o in zip(case["probs"], ops)]
    route = eng.debug_gemm(case["op"], [go.descriptor(p, b) for p, b in zip(case["probs"], bufs)], act=case["act"])
    torch.cuda.synchronize()
    got = [b["C"].cpu() for b in bufs]
    res["gpu_s"] = time.time() - t0
    want = go.route_of(case)
    res["route"] = go.route_summary(route)
    res["route_bad"] = [] if route == want and res["route"] == case["expect"] else [f"reported {route}, the rules give {want}, the table {case['expect']}"]
    outs, stray, unwritten = [], 0, 0
    for p, c in zip(case["probs"], got):
        m = go.c_mask(p)
        bits = c.view(torch.int32)
        stray += int((bits[~m] != go.SENTINEL_BITS).sum())
        unwritten += int((bits[m] == go.SENTINEL_BITS).sum())
        outs.append(torch.as_strided(c, (p["batch"], p["heads"], p["M"], p["N"]), (p["scb"], p["sch"], p["scm"], p["scn"]), go.GUARD).clone())
    res.update(stray=stray, unwritten=unwritten)
    ref, A = go.reference(case, ops), go.magnitude(case, ops)
    tol = go.tolerance(case, ops, ref, A)
    ok, msgs, meas = go.check(case, ops, outs, ref, A, tol)
    res.update(ok=ok, msg="; ".join(msgs), measured=meas, tol=tol, total_s=time.time() - t0)
    return res


def _run_refusal(eng, torch, row):
    rid, op, act, probs, breakage, text = row
    case = dict(id=rid, family="refused", op=op, act=act, probs=probs)
    bufs = [_device_buffers(torch, p, o) for p, o in zip(probs, go.make_operands(case))]
    if breakage == "share_c":         # both problems of the pair write one buffer
        bufs[1]["C"] = bufs[0]["C"]
    ds = [go.descriptor(p, b) for p, b in zip(probs, bufs)]
    if breakage == "double_sbb":      # the last batch sample of B then lies beyond B's buffer
        ds[0]["sbb"] = 2 * ds[0]["sbb"]
    before = [b["C"].cpu().view(torch.int32).clone() for b in bufs]
    try:
        eng.debug_gemm(op, ds, act=act)
        return dict(id=rid, refused=False, error="loco_debug_gemm took what its contract excludes")
    except RuntimeError as e:
        torch.cuda.synchronize()
        same = all(torch.equal(b["C"].cpu().view(torch.int32), x) for b, x in zip(bufs, before))
        return dict(id=rid, refused=text in str(e) and same, error=str(e) + ("" if same else " -- and the output was touched"))


def _worker(path):
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import TINY_DDPM, synth_params
    torch.set_num_threads(min(16, torch.get_num_threads()))
    eng = H.LocoEngine(TINY_DDPM, max_batch=1)      # the engine's own config is irrelevant: every tensor is the caller's
    eng.load_state_dict(synth_params(TINY_DDPM, 0))
    results = []
    for row in go.REFUSALS:      # first: a refusal that launched would show in the cases behind it
        results.append(_run_refusal(eng, torch, row))
        print(json.dumps(results[-1]), flush=True)
    for case in go.CASES:
        r = _run_case(eng, torch, case)
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
    out = str(tmp_path_factory.mktemp("gemm_oracle") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env["LOCO_HIP_LIB"] = _diag_lib()
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out], env=env, capture_output=True, text=True, timeout=300)
    done = r.stdout.count("\n")
    assert r.returncode == 0, f"the worker ended with {r.returncode} after {done} of {len(IDS)} cases:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    with open(out) as f:
        return {x["id"]: x for x in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_gemm_launch_matches_float64(results, cid):
    r = results[cid]
    if "refused" in r:
        assert r["refused"], r["error"]
        return
    assert not r["route_bad"], f"{r['family']}: {r['route_bad']}"
    for i, (m, t) in enumerate(zip(r["measured"], r["tol"])):
        print(f"{cid} [{r['route']}] {r['op']} problem {i}: max |out - ref| / A_out = {m:.3e}, tau = {t['tau']:.3e} "
              f"(format {t['format']:.2e} accumulation {t['accumulation']:.2e} activation {t['activation']:.2e}; Lip {t['lip']:.4f})")
    assert r["unwritten"] == 0, f"{r['unwritten']} addressed output floats still hold the sentinel; {r['msg']}"
    assert r["ok"], f"{r['family']} ({r['route']}): {r['msg']}"
    assert r["stray"] == 0, f"{r['stray']} floats of the output buffer outside the strides' reach lost their sentinel bits ({r['route']})"
    assert r["total_s"] < 20.0, f"the case took {r['total_s']:.1f} s"
