"""GPU: single attention passes of every route against float64 (loco_debug_attn of the diagnostics build vs tests/attn_oracle.py).

Every row of attn_oracle.ROWS, for every pass and precision it lists (flash rows with and without the record workspace), is one
call of loco_debug_attn: one pass of one attention stage through the engine's own attn_forward / attn_tangent / attn_cotangent or
xa_forward / xa_linear, on seeded operands (scores of variance about 3, per-channel offsets on q, k, v; P and o of the linear passes
are the float64 forward rounded to float32).  Per case:
  1. the route text names the launches the table expects (attn_oracle.route_of / check_route) -- a change of a predicate that
     reroutes a case fails here instead of silently testing another kernel;
  2. |out - ref| <= tau A + 1e-30 on EVERY element of every output tensor, tau from the reference alone (attn_oracle.tolerance:
     4 x (format + accumulation + row operation)); outputs are pre-filled with NaN; the message names the worst element's
     tensor, probe, head, channel, token;
  3. the case stays under 20 s.
The rows the kernels' contracts exclude (T = 96, Lt = 80) must be REFUSED by loco_debug_attn before any launch.  One flash row
also runs under f16 and must equal its bf16x3 output bit for bit: attention has no f16 arithmetic.

One child process owns the engine (hip.py binds one library per process; the diagnostics build is chosen through LOCO_HIP_LIB) and
runs the whole table.  No environment switch is set, except LOCO_GEMM_REC=0 around the one row that pins the converting bf16x3
GEMM (read per launch; the product falls back this way when the record workspace cannot be allocated).  The child is this file run
as a script:   LOCO_HIP_LIB=.../libloco_hip_diag.so python tests/test_gpu_attn_oracle.py --worker out.json

Measured on the MI355X, max |out - ref| / A per (family, pass, precision) over the cases (tau of the same cases alongside; margin 4):
  family                   pass  prec    cases  max |out - ref| / A  tau (min ... max)      worst share of tau
  flash 4/2                tan   f32         1  1.55e-07             9.4e-05 ... 9.4e-05    0.002
  flash 4/2                tan   bf16x3      2  5.61e-06             1.2e-04 ... 1.2e-04    0.048
  flash 4/2                cot   f32         1  3.70e-07             3.4e-05 ... 6.4e-05    0.008
  flash 4/2                cot   bf16x3      2  3.65e-05             6.9e-05 ... 2.1e-04    0.175
  flash 3/2                tan   f32         3  2.36e-07             1.3e-04 ... 2.1e-04    0.001
  flash 3/2                tan   bf16x3      6  8.11e-06             1.6e-04 ... 2.3e-04    0.047
  flash 3/2                cot   f32         3  5.89e-07             6.4e-05 ... 1.1e-04    0.009
  flash 3/2                cot   bf16x3      6  4.12e-05             8.2e-05 ... 2.8e-04    0.165
  flash 5/3                tan   f32         2  2.23e-07             1.6e-04 ... 1.6e-04    0.001
  flash 5/3                tan   bf16x3      4  7.12e-06             1.8e-04 ... 1.9e-04    0.037
  flash 5/3                cot   f32         2  3.68e-07             6.4e-05 ... 1.0e-04    0.006
  flash 5/3                cot   bf16x3      4  3.24e-05             9.4e-05 ... 2.3e-04    0.139
  flash 6/3                tan   f32         1  1.78e-07             1.1e-04 ... 1.1e-04    0.002
  flash 6/3                tan   bf16x3      2  8.86e-06             1.4e-04 ... 1.4e-04    0.062
  flash 6/3                cot   f32         1  3.48e-07             3.3e-05 ... 7.9e-05    0.010
  flash 6/3                cot   bf16x3      2  2.52e-05             6.7e-05 ... 1.8e-04    0.139
  flash long               tan   f32         1  2.80e-07             5.2e-04 ... 5.2e-04    0.001
  flash long               tan   bf16x3      2  5.60e-06             5.4e-04 ... 5.4e-04    0.010
  flash long               cot   f32         1  4.66e-07             2.5e-04 ... 2.8e-04    0.002
  flash long               cot   bf16x3      2  2.37e-05             3.0e-04 ... 3.7e-04    0.064
  flash text               tan   f32         3  3.11e-07             1.2e-04 ... 2.0e-04    0.002
  flash text               tan   bf16x3      6  1.10e-05             1.7e-04 ... 2.4e-04    0.065
  flash text               cot   f32         3  4.59e-07             3.3e-05 ... 1.1e-04    0.008
  flash text               cot   bf16x3      6  3.74e-05             7.5e-05 ... 2.2e-04    0.167
  generic                  fwd   f32         2  1.89e-06             1.8e-05 ... 2.5e-05    0.075
  generic                  fwd   bf16x3      2  1.89e-06             1.8e-05 ... 2.5e-05    0.075
  generic                  tan   f32         4  3.11e-07             4.1e-05 ... 1.9e-04    0.005
  generic                  tan   bf16x3      3  2.28e-07             4.1e-05 ... 1.9e-04    0.005
  generic                  cot   f32         4  5.29e-07             1.8e-05 ... 1.2e-04    0.022
  generic                  cot   bf16x3      3  5.29e-07             1.8e-05 ... 1.2e-04    0.022
  generic text             fwd   f32         1  1.64e-06             4.8e-05 ... 6.4e-05    0.026
  generic text             fwd   bf16x3      1  1.64e-06             4.8e-05 ... 6.4e-05    0.026
  generic text             tan   f32         1  2.97e-07             1.2e-04 ... 1.2e-04    0.002
  generic text             tan   bf16x3      1  2.97e-07             1.2e-04 ... 1.2e-04    0.002
  generic text             cot   f32         1  5.26e-07             1.8e-05 ... 7.9e-05    0.029
  generic text             cot   bf16x3      1  5.26e-07             1.8e-05 ... 7.9e-05    0.029
  long rows                fwd   f32         1  2.13e-06             2.6e-04 ... 2.7e-04    0.008
  long rows                tan   f32         1  3.00e-07             5.3e-04 ... 5.3e-04    0.001
  long rows                cot   f32         1  5.30e-07             2.5e-04 ... 2.7e-04    0.002
  record GEMM              tan   bf16x3      1  1.02e-05             6.4e-04 ... 6.4e-04    0.016
  record GEMM              cot   bf16x3      1  1.34e-05             2.8e-04 ... 4.8e-04    0.028
  converting bf16x3 GEMM   tan   bf16x3      1  7.47e-07             6.1e-04 ... 6.1e-04    0.001
  converting bf16x3 GEMM   cot   bf16x3      1  1.34e-05             2.8e-04 ... 4.8e-04    0.029
  cross                    fwd   f32         6  2.78e-06             1.8e-05 ... 7.1e-05    0.079
  cross                    fwd   bf16x3      6  2.78e-06             1.8e-05 ... 7.1e-05    0.079
  cross                    tan   f32         6  3.38e-07             3.6e-05 ... 1.0e-04    0.006
  cross                    tan   bf16x3      6  3.38e-07             3.6e-05 ... 1.0e-04    0.006
  cross                    cot   f32         6  5.97e-07             3.6e-05 ... 1.0e-04    0.011
  cross                    cot   bf16x3      6  5.97e-07             3.6e-05 ... 1.0e-04    0.011
  cross generic            fwd   f32         2  2.07e-06             3.3e-05 ... 9.4e-05    0.037
  cross generic            fwd   bf16x3      2  2.07e-06             3.3e-05 ... 9.4e-05    0.037
  cross generic            tan   f32         2  1.37e-07             1.0e-04 ... 1.2e-04    0.001
  cross generic            tan   bf16x3      2  1.37e-07             1.0e-04 ... 1.2e-04    0.001
  cross generic            cot   f32         2  2.73e-07             1.0e-04 ... 1.2e-04    0.002
  cross generic            cot   bf16x3      2  2.73e-07             1.0e-04 ... 1.2e-04    0.002
(the bf16x3 rows of the generic, cross and long-row families run exact-fp32 kernels: their products are below the bf16 pipe's
threshold, so the figures equal the f32 ones; the f16 bit-identity cases carry no ratio)
"""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as ao      # noqa: E402

KEYS = ao.keys()
ROW = {r["id"]: r for r in ao.ROWS}
PASS_ID = {"fwd": 0, "tan": 1, "cot": 2}
IN_SELF = {"fwd": ("fq", "fk", "fv"), "tan": ("q", "k", "v", "P", "o", "dq", "dk", "dv"), "cot": ("q", "k", "v", "P", "o", "go")}
IN_CROSS = {"fwd": ("fq",), "tan": ("P", "dq"), "cot": ("P", "go")}
DESC_NAME = {"fq": "q", "fk": "k", "fv": "v"}


def _run_case(eng, torch, key, cache, bits):
    rid, pas, prec, ws = key
    row = ROW[rid]
    d = ao.case_of(row, pas)
    cross = d["kind"] == "cross"
    ck = (rid, pas)
    if ck not in cache:
        cache.clear()
        cache[ck] = dict(ops=ao.make_operands(d) if not row["refused"] else None)
    c = cache[ck]
    ops = c["ops"]
    res = dict(id=rid, pas=pas, prec=prec, ws=ws, family=row["family"])
    C, T, B, Tk = d["NH"] * d["CH"], d["T"], d["B"], ao.tk_of(d)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    kw = dict(kind=1 if cross else 0, pass_=PASS_ID[pas], T=T, NH=d["NH"], CH=d["CH"], B=B, Lt=d["Lt"], L=d["L"], pair=int(d["pair"]),
              no_workspace=0 if ws else 1)
    eng.set_precision(prec)
    t0 = time.time()
    if row["refused"]:
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
        kw.update(q=z(C, T), k=z(C, T), v=z(C, T), P=z(d["NH"], T, Tk), o=z(C, T), dq=z(B, C, T), dk=z(B, C, T), dv=z(B, C, T), out=nan(B, C, T))
        if d["Lt"]:
            kw.update(kt=z(C, d["Lt"]), vt=z(C, d["Lt"]))
        try:
            eng.debug_attn(**kw)
            res.update(refused=False, error="loco_debug_attn took a shape the kernels' contracts exclude")
        except RuntimeError as e:
            torch.cuda.synchronize()
            res.update(refused=row["refused"] in str(e) and bool(torch.isnan(kw["out"]).all()), error=str(e))
        return res
    if "dev" not in c:
        c["dev"] = {k: v.to(torch.float32).cuda() for k, v in ops.items()}
    dev = c["dev"]
    for k in (IN_CROSS if cross else IN_SELF)[pas]:
        kw[DESC_NAME.get(k, k)] = dev[k]
    if "kt" in dev:
        kw.update(kt=dev["kt"], vt=dev["vt"])
    if pas == "fwd":
        outs = dict(P=nan(B, d["NH"], T, Tk), o=nan(B, C, T))
    elif pas == "tan":
        outs = dict(out=nan(B, C, T))
    else:
        outs = dict(gq=nan(B, C, T)) if cross else dict(gq=nan(B, C, T), gk=nan(B, C, T), gv=nan(B, C, T))
    kw.update(outs)
    if not row["rec"]:
        os.environ["LOCO_GEMM_REC"] = "0"
    try:
        route = eng.debug_attn(**kw)
    finally:
        os.environ.pop("LOCO_GEMM_REC", None)
    torch.cuda.synchronize()
    res["gpu_s"] = time.time() - t0
    got = {k: v.cpu() for k, v in outs.items()}
    if prec == "f16":      # the bit-identity case: against the bf16x3 output of the same (row, pass)
        want = bits.get((rid, pas))
        res.update(ok=want is not None and all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in got),
                   msg="the f16 output differs from the bf16x3 output", route_bad=[], route=[r["kernel"] for r in route], unwritten=0,
                   total_s=time.time() - t0, outputs={})
        return res
    if row["f16"] and prec == "bf16x3" and ws:
        bits[(rid, pas)] = got
    expected, flags, flash = ao.route_of(d, pas, prec, ws, row["rec"])
    res["route_bad"] = ao.check_route(route, expected)
    res["route"] = [r["kernel"] for r in route]
    res["unwritten"] = int(sum(torch.isnan(v).sum() for v in got.values()))
    dd, oo = d, ops
    pr = ao.probes_of(row, pas)
    if pr:
        dd, oo = ao.sub_case(d, ops, pr)
        got = {k: v.index_select(0, torch.tensor(list(pr))) for k, v in got.items()}
    if "ref" not in c:
        c["ref"] = (ao.reference(dd, oo, pas), ao.magnitude(dd, oo, pas))
    ref, A = c["ref"]
    tk = ("tol", tuple(sorted(k for k, v in flags.items() if v)), flash)
    if tk not in c:
        c[tk] = ao.tolerance(dd, oo, pas, flags, ref, A, flash)
    tol = c[tk]
    ok, msgs, per = True, [], {}
    for name in ref:
        o, m, measured = ao.worst(name, got[name].to(torch.float64), ref[name], A[name], tol[name]["tau"], dd)
        ok = ok and o
        if not o:
            msgs.append(m)
        per[name] = dict(measured=measured, **tol[name])
    res.update(ok=ok, msg="; ".join(msgs), outputs=per, total_s=time.time() - t0)
    return res


def _worker(path):
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import TINY_DDPM, synth_params
    torch.set_num_threads(min(16, torch.get_num_threads()))
    eng = H.LocoEngine(TINY_DDPM, max_batch=1)      # the engine's own config is irrelevant: every tensor is the caller's
    eng.load_state_dict(synth_params(TINY_DDPM, 0))
    results, cache, bits = [], {}, {}
    for key in KEYS:
        r = _run_case(eng, torch, key, cache, bits)
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
    out = str(tmp_path_factory.mktemp("attn_oracle") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env["LOCO_HIP_LIB"] = _diag_lib()
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out], env=env, capture_output=True, text=True, timeout=300)
    done = r.stdout.count("\n")
    assert r.returncode == 0, f"the worker ended with {r.returncode} after {done} of {len(KEYS)} cases:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    with open(out) as f:
        return {(x["id"], x["pas"], x["prec"], x["ws"]): x for x in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("rid, pas, prec, ws", KEYS, ids=[f"{r}-{p}-{q}-{'ws' if w else 'nows'}" for r, p, q, w in KEYS])
def test_attention_pass_matches_float64(results, rid, pas, prec, ws):
    r = results[(rid, pas, prec, ws)]
    if "refused" in r:
        assert r["refused"], r["error"]
        return
    assert not r["route_bad"], f"{r['family']}: {r['route_bad']}"
    assert r["unwritten"] == 0, f"{r['unwritten']} output elements were never written (NaN sentinel left); {r['msg']}"
    for name, t in r["outputs"].items():
        print(f"{rid} {pas} {prec} {name}: max |out - ref| / A = {t['measured']:.3e}, tau = {t['tau']:.3e} "
              f"(format {t['format']:.2e} accumulation {t['accumulation']:.2e} row {t['row']:.2e})")
    assert r["ok"], f"{r['family']} ({', '.join(r['route'])}): {r['msg']}"
    assert r["total_s"] < 20.0, f"the case took {r['total_s']:.1f} s"
