"""GPU: single launches of every attention kernel of the encoders against float64 (loco_debug_enc_attn of the diagnostics build vs
tests/enc_attn_oracle.py).

Every row of enc_attn_oracle.ROWS is one call of loco_debug_enc_attn: one launch of enc_attn_kernel (plain, keeping m / l, with the
relative-position tables), prompt_attn_kernel (CLIP causal, T5 length mask + bias), the two cotangent kernels of the CLIP image tower,
seg_attn_kernel, sd_t2i_kernel or sd_i2t_kernel through the launcher the product's call site uses, on seeded operands of two score
profiles (spread: variance about 3; late: a ramp of about 30 whose maximum lies in the last chunk).  Per case:
  1. the route text names the kernel form the table expects (enc_attn_oracle.expected_route) -- a predicate that moves, such as the
     chunk thresholds of the cotangent kernels, fails here instead of silently testing another instantiation;
  2. outputs are pre-filled with a NaN sentinel: every element the contract assigns is overwritten, every other element (padding
     columns, the q block of gqkv in op 6, the token rows NQ ... 7 of op 8) keeps the sentinel's bits;
  3. |out - ref| <= tau A + 1e-30 on EVERY element of every output tensor, tau from the reference alone (enc_attn_oracle.tolerance:
     4 x (accumulation + row operation)); the message names the worst element's tensor, group, head, channel, token;
  4. the bit identities: op 1's out equals op 0's on the same operands; row 0 of every causal prompt (one live key) equals v[:, 0],
     as does every row of a T5 prompt of length 1 and the image -> token output with NQ = 1; columns T ... Tp - 1 of op 9 are 0;
  5. the case stays under 20 s.
The rows the contracts exclude must be REFUSED before any launch, with the message the table names and the outputs untouched.

One child process loads the diagnostics build (LOCO_HIP_LIB) and runs the whole table.  The child is this file run as a script:
    LOCO_HIP_LIB=.../libloco_hip_diag.so python tests/test_gpu_enc_attn_oracle.py --worker out.json

Measured on the MI355X, max |out - ref| / A per (family, profile, tensor) over the cases (tau of the same cases alongside; margin 4):
  family               profile  tensor  cases  max |out - ref| / A  tau (min ... max)      worst share of tau
  enc_attn             spread   out         6  1.66e-06             1.6e-05 ... 6.6e-05    0.025
  enc_attn             late     out         3  4.87e-06             5.0e-05 ... 9.7e-05    0.052
  enc_attn keep        spread   out         6  1.66e-06             1.6e-05 ... 6.6e-05    0.025
  enc_attn keep        spread   m           6  1.15e-07             3.1e-06 ... 2.7e-05    0.027
  enc_attn keep        spread   lse         6  4.59e-08             1.6e-05 ... 6.6e-05    0.001
  enc_attn keep        late     out         3  4.87e-06             5.0e-05 ... 9.7e-05    0.052
  enc_attn keep        late     m           3  3.72e-07             3.8e-06 ... 2.7e-05    0.033
  enc_attn keep        late     lse         3  8.55e-08             5.0e-05 ... 9.7e-05    0.001
  enc_attn bias        spread   out         4  1.11e-06             1.4e-05 ... 7.1e-05    0.031
  enc_attn bias        late     out         2  4.81e-06             9.2e-05 ... 1.1e-04    0.045
  prompt_attn causal   spread   out         5  1.26e-06             1.3e-05 ... 5.6e-05    0.041
  prompt_attn causal   late     out         4  2.98e-06             5.4e-05 ... 7.9e-05    0.050
  prompt_attn bias     spread   out         5  8.28e-07             1.4e-05 ... 5.6e-05    0.024
  prompt_attn bias     late     out         4  5.21e-06             4.1e-05 ... 9.7e-05    0.060
  clipvis cot q        spread   gq          5  9.67e-07             2.0e-05 ... 4.2e-04    0.025
  clipvis cot q        spread   delta       5  8.78e-08             5.7e-06 ... 2.7e-05    0.015
  clipvis cot q        late     gq          3  6.42e-06             1.2e-04 ... 1.5e-04    0.045
  clipvis cot q        late     delta       3  2.75e-08             2.1e-05 ... 2.5e-05    0.001
  clipvis cot kv       spread   gk          5  6.35e-07             2.2e-05 ... 2.5e-04    0.011
  clipvis cot kv       spread   gv          5  2.82e-06             1.9e-05 ... 2.3e-04    0.041
  clipvis cot kv       late     gk          3  2.51e-07             1.1e-04 ... 2.0e-04    0.002
  clipvis cot kv       late     gv          3  2.07e-06             8.3e-05 ... 1.8e-04    0.018
  seg_attn             spread   out         5  1.09e-06             9.3e-06 ... 7.0e-05    0.025
  seg_attn             late     out         3  1.89e-06             5.0e-05 ... 8.6e-05    0.036
  sd_t2i               spread   out         6  9.00e-07             1.9e-05 ... 6.9e-05    0.020
  sd_t2i               late     out         4  1.18e-06             9.1e-05 ... 1.3e-04    0.013
  sd_i2t               spread   out         7  9.39e-07             4.1e-06 ... 1.9e-05    0.049
(lse = m + log l of op 1, formed in float64 from the kernel's m and l; the refused rows and the bit identities carry no ratio)
"""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_attn_oracle as eo      # noqa: E402

IDS = [r["id"] for r in eo.ROWS]
ROW = {r["id"]: r for r in eo.ROWS}


def _desc(c):
    op, D = c["op"], c["heads"] * c["hd"]
    kw = dict(op=op, D=D, hd=c["hd"], heads=c["heads"], nk=c["nk"], groups=c["groups"], size=c["size"], NQ=c["NQ"], Tp=c["Tp"], ld=c["ld"],
              Tall=c["groups"] * c["nk"] if op == 2 else 0, scale=eo.scale_of(c))
    if op == 8 and c["per_prompt"]:
        kw["kbs"] = D * c["ld"]
    if op == 9 and c["per_prompt"]:
        kw["qbs"] = D * c["ld"]
    return kw


def _refused(H, torch, row, res):
    c = row["case"]
    zin = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    outs = {n: eo.sentinel(1 << 20).cuda() for n in ("out", "ml", "gqkv", "delta")}
    kw = _desc(c)
    op = c["op"]
    ins = {0: ("qkv",), 1: ("qkv",), 2: ("qkv", "relh", "relw"), 3: ("qkv",), 4: ("qkv", "bias_tab"), 5: ("qkv", "o", "go"), 6: ("qkv", "go"),
           7: ("qkv",), 8: ("q", "k", "v"), 9: ("q", "k", "v")}[op]
    kw.update({n: zin for n in ins})
    if op == 4:
        kw["lens"] = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    if op in (5, 6):
        kw.update(ml=zin, delta=outs["delta"] if op == 5 else zin, gqkv=outs["gqkv"])
    else:
        kw["out"] = outs["out"]
    if op == 1 or c.get("with_ml"):
        kw["ml"] = outs["ml"]
    if row["null"]:
        kw[row["null"]] = None
    try:
        H.debug_enc_attn(**kw)
        res.update(refused=False, error="loco_debug_enc_attn took a case the kernels' contracts exclude")
    except RuntimeError as e:
        torch.cuda.synchronize()
        clean = all(bool((v.view(torch.int32) == eo.SENTINEL).all()) for v in outs.values())
        res.update(refused=row["refused"] in str(e) and "(-2)" in str(e) and clean, error=str(e) + ("" if clean else "; an output was touched"))
    return res


def _run_case(H, torch, row, kept):
    c = row["case"]
    res = dict(id=row["id"], family=row["family"], profile=c["profile"])
    if row["refused"]:
        return _refused(H, torch, row, res)
    t0 = time.time()
    op = c["op"]
    ops = eo.make_operands(c)
    ins = {k: v.cuda() for k, v in eo.pack(c, ops).items()}
    outs = {k: eo.sentinel(*s).cuda() for k, s in eo.out_shapes(c).items()}
    kw = dict(_desc(c), **ins)
    if op == 5:
        kw.update(ml=ins["ml"], gqkv=outs["gqkv"], delta=outs["delta"])
    elif op == 6:
        kw.update(gqkv=outs["gqkv"])
    else:
        kw.update(outs)
    if c["inplace"]:
        outs["out"] = kw["out"] = ins["q"]
    route = H.debug_enc_attn(**kw)
    torch.cuda.synchronize()
    res["gpu_s"] = time.time() - t0
    bufs = {k: v.cpu() for k, v in outs.items()}
    exp = eo.expected_route(c)
    res["route"] = route
    res["route_bad"] = [] if route == exp else [f"route {route}, expected {exp}"]
    got, res["unwritten"], res["outside"] = eo.unpack(c, bufs)
    bits = []
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if op == 0:
        kept[row["id"]] = bufs["out"]
    if row["twin"]:
        if not (row["twin"] in kept and same(bufs["out"], kept[row["twin"]])):
            bits.append("the out of op 1 differs from the out of op 0 on the same operands")
    v32 = ops["v"].to(torch.float32)
    if op == 3 and not same(got["out"][..., 0], v32[..., 0]):
        bits.append("row 0 of a causal prompt (one live key) is not v[:, 0]")
    if op == 4:
        for p, n in enumerate(c["lens"]):
            if n == 1 and not same(got["out"][p], v32[p, :, :, :1].expand(-1, -1, c["nk"])):
                bits.append(f"prompt {p} of length 1: a row is not v[:, 0]")
    if op == 9:
        if c["NQ"] == 1 and not same(got["out"], v32.expand(-1, -1, -1, c["nk"])):
            bits.append("NQ = 1: the output is not vx row 0")
        if not bool((got["zeros"].view(torch.int32) == 0).all()):
            bits.append("columns T ... Tp - 1 are not exactly 0")
    res["bits_bad"] = bits
    if op == 1:
        got["lse"] = got["m"].to(torch.float64) + torch.log(got.pop("l").to(torch.float64))
    ref, A, tol = eo.reference(c, ops), eo.magnitude(c, ops), eo.tolerance(c, ops)
    ok, msgs, per = True, [], {}
    for name in ref:
        o, m, measured = eo.worst(name, got[name].to(torch.float64), ref[name], A[name], tol[name]["tau"])
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
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.zeros(1, device="cuda")
    results, kept = [], {}
    for row in eo.ROWS:
        r = _run_case(H, torch, row, kept)
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
    """the whole table on the diagnostics build, in one child process"""
    out = str(tmp_path_factory.mktemp("enc_attn_oracle") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env["LOCO_HIP_LIB"] = _diag_lib()
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out], env=env, capture_output=True, text=True, timeout=300)
    done = r.stdout.count("\n")
    assert r.returncode == 0, f"the worker ended with {r.returncode} after {done} of {len(IDS)} cases:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    with open(out) as f:
        return {x["id"]: x for x in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("rid", IDS)
def test_encoder_attention_launch_matches_float64(results, rid):
    r = results[rid]
    if ROW[rid]["refused"]:
        assert r["refused"], r["error"]
        return
    assert not r["route_bad"], f"{r['family']}: {r['route_bad']}"
    assert r["unwritten"] == 0, f"{r['unwritten']} output elements were never written (the sentinel is left)"
    assert r["outside"] == 0, f"{r['outside']} elements outside the launch's contract were overwritten"
    for name, t in r["outputs"].items():
        print(f"{rid} {name}: max |out - ref| / A = {t['measured']:.3e}, tau = {t['tau']:.3e} "
              f"(accumulation {t['accumulation']:.2e} row {t['row']:.2e})")
    assert r["ok"], f"{r['family']} ({r['route']}): {r['msg']}"
    assert not r["bits_bad"], f"{r['family']}: {r['bits_bad']}"
    assert r["total_s"] < 20.0, f"the case took {r['total_s']:.1f} s"
