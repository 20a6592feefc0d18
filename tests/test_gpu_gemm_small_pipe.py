"""GPU: the pipelined form of the exact-fp32 small GEMM and the two-problem launch of the cotangent (csrc/gemm.hip
gemm_f32_small_pipe_kernel / launch_gemm_pair) against float64 and, bit for bit, against the scalar-load loop they replace.

Every case is a self-attention stage with `pair` set, no text keys, precision f32, run through loco_debug_attn of the diagnostics
build, so every product is a gemm_f32 launch of the small tiling (64 x 64 grid < 320 workgroups, K >= 128).  Forward, tangent and
cotangent of

  case          (T, NH, CH, B)    covers
  smallest      (128, 1, 128, 2)  K = 128 in every product (two K-steps: the shortest pipeline); both segment counts; the four
                                  layout combinations (scores: both operands k-major, values: both unit stride along k, keys: mixed)
  two_heads     (128, 2, 128, 1)  the batch2 / head stride path
  headline      (256, 1, 512, 3)  the shapes of the benchmark (K = 256 / 512 per segment, 4 - 16 K-steps)
  fallback      (192, 1, 160, 2)  K = 160 in the score products is no multiple of 64: the scalar-load loop is still taken and still
                                  right; the value products (K = 192) run three K-steps, an odd count.  loco_debug_attn refuses
                                  T = 160 (T must be a multiple of 64), so the ragged K sits in CH and T is the nearest accepted size
  wide_fallback (128, 1, 136, 2)  ragged M = 136 in the value products, K = 136 in the scores: the scalar-load loop throughout

Two child processes, one after the other, each under its own timeout and the second only if the first ended with 0: the first
with LOCO_GEMM_SMALL_PIPE=0 LOCO_GEMM_GROUP=0 (the loop and the launches of before), the second with the defaults.  The parent
makes the operands once (tests/attn_oracle.make_operands) and hands them over in a file; each child fills every output with NaN
inside a guard band of a sentinel value, runs the passes and dumps the outputs.  Per (case, pass):
  1. the route text is attn_oracle.route_of's (in both children: the switches change no route line);
  2. |out - ref| <= tau A + 1e-30 on every element, reference and tau from tests/attn_oracle.py (f32 route) -- for both children;
  3. no NaN is left in an output and the guard bands around every output hold the sentinel;
  4. the bytes of the two children's outputs are equal.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as ao      # noqa: E402

CASES = {
    "smallest": ao.case("self", 128, 1, 128, 2, pair=True),
    "two_heads": ao.case("self", 128, 2, 128, 1, pair=True),
    "headline": ao.case("self", 256, 1, 512, 3, pair=True),
    "fallback": ao.case("self", 192, 1, 160, 2, pair=True),
    "wide_fallback": ao.case("self", 128, 1, 136, 2, pair=True),
}
KEYS = [(c, p) for c in CASES for p in ao.PASSES]
PASS_ID = {"fwd": 0, "tan": 1, "cot": 2}
INPUTS = {"fwd": ("fq", "fk", "fv"), "tan": ("q", "k", "v", "P", "o", "dq", "dk", "dv"), "cot": ("q", "k", "v", "P", "o", "go")}
DESC_NAME = {"fq": "q", "fk": "k", "fv": "v"}
GUARD, SENTINEL = 256, 12345.0      # floats on either side of an output (a multiple of 4: the outputs stay 16-byte aligned)
MODES = {"loop": {"LOCO_GEMM_SMALL_PIPE": "0", "LOCO_GEMM_GROUP": "0"}, "pipe": {}}
CHILD_TIMEOUT = 240


def _out_shapes(d, pas):
    C, T, B, NH = d["NH"] * d["CH"], d["T"], d["B"], d["NH"]
    if pas == "fwd":
        return dict(P=(B, NH, T, ao.tk_of(d)), o=(B, C, T))
    if pas == "tan":
        return dict(out=(B, C, T))
    return dict(gq=(B, C, T), gk=(B, C, T), gv=(B, C, T))


def _worker(work):
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import TINY_DDPM, synth_params
    eng = H.LocoEngine(TINY_DDPM, max_batch=1)      # the engine's own config is irrelevant: every tensor is the caller's
    eng.load_state_dict(synth_params(TINY_DDPM, 0))
    eng.set_precision("f32")
    mode = os.environ["LOCO_TEST_MODE"]
    results = {}
    for cname, d in CASES.items():
        ops = torch.load(os.path.join(work, f"ops-{cname}.pt"))
        dev = {k: v.to(torch.float32).cuda() for k, v in ops.items()}
        for pas in ao.PASSES:
            kw = dict(kind=0, pass_=PASS_ID[pas], T=d["T"], NH=d["NH"], CH=d["CH"], B=d["B"], Lt=0, L=0, pair=1, no_workspace=0)
            for k in INPUTS[pas]:
                kw[DESC_NAME.get(k, k)] = dev[k]
            bufs, outs = {}, {}
            for name, shape in _out_shapes(d, pas).items():
                n = 1
                for s in shape:
                    n *= s
                buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
                buf[GUARD:GUARD + n] = float("nan")
                bufs[name], outs[name] = buf, buf[GUARD:GUARD + n].view(shape)
            kw.update(outs)
            route = eng.debug_attn(**kw)
            torch.cuda.synchronize()
            guards, unwritten = True, 0
            for name, buf in bufs.items():
                n = outs[name].numel()
                guards = guards and bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
                unwritten += int(torch.isnan(outs[name]).sum())
                with open(os.path.join(work, f"{mode}-{cname}-{pas}-{name}.bin"), "wb") as f:
                    f.write(outs[name].cpu().numpy().tobytes())
            results[f"{cname}-{pas}"] = dict(route=route, guards=guards, unwritten=unwritten)
            print(mode, cname, pas, [r["kernel"] for r in route], "guards", guards, "unwritten", unwritten, flush=True)
    with open(os.path.join(work, f"{mode}-results.json"), "w") as f:
        json.dump(results, f)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    _worker(sys.argv[2])
    sys.exit(0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the operands, the float64 references and the two children's results; the references are computed once and only read"""
    import torch
    lib = os.path.join(ROOT, "loco-edit_amd", "libloco_hip_diag.so")
    assert os.path.exists(lib), "libloco_hip_diag.so is missing: run `make -C loco-edit_amd/csrc diag` (or __graft_entry__.build())"
    work = str(tmp_path_factory.mktemp("gemm_small_pipe"))
    ops = {}
    for cname, d in CASES.items():
        ops[cname] = ao.make_operands(d)
        torch.save(ops[cname], os.path.join(work, f"ops-{cname}.pt"))
    res = {}
    for mode, switches in MODES.items():      # one after the other; the second only if the first ended with 0
        env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
        env.update(switches, LOCO_HIP_LIB=lib, LOCO_TEST_MODE=mode)
        env.pop("WORLD_SIZE", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", work], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, f"the {mode} worker ended with {r.returncode}:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
        with open(os.path.join(work, f"{mode}-results.json")) as f:
            res[mode] = json.load(f)
    return dict(work=work, ops=ops, res=res, ref={})


def _reference(runs, cname, pas):
    key = (cname, pas)
    if key not in runs["ref"]:
        d, ops = CASES[cname], runs["ops"][cname]
        expected, flags, flash = ao.route_of(d, pas, "f32")
        assert not flash and not any(flags.values())
        ref, A = ao.reference(d, ops, pas), ao.magnitude(d, ops, pas)
        runs["ref"][key] = (expected, ref, A, ao.tolerance(d, ops, pas, flags, ref, A, flash))
    return runs["ref"][key]


def _load(runs, mode, cname, pas, name):
    import numpy as np
    import torch
    with open(os.path.join(runs["work"], f"{mode}-{cname}-{pas}-{name}.bin"), "rb") as f:
        raw = f.read()
    return raw, torch.from_numpy(np.frombuffer(raw, dtype=np.float32).copy()).view(_out_shapes(CASES[cname], pas)[name])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cname, pas", KEYS, ids=[f"{c}-{p}" for c, p in KEYS])
def test_route_accuracy_and_bounds(runs, cname, pas, mode):
    import torch
    d = CASES[cname]
    r = runs["res"][mode][f"{cname}-{pas}"]
    expected, ref, A, tol = _reference(runs, cname, pas)
    assert not ao.check_route(r["route"], expected), ao.check_route(r["route"], expected)
    assert all(x["kernel"] in ("gemm_f32", "softmax_rows", "softmax_jac") for x in r["route"]), r["route"]
    assert r["unwritten"] == 0, f"{r['unwritten']} output elements were never written (NaN sentinel left)"
    assert r["guards"], "the guard band around an output was written"
    for name in ref:
        _, got = _load(runs, mode, cname, pas, name)
        ok, msg, measured = ao.worst(name, got.to(torch.float64), ref[name], A[name], tol[name]["tau"], d)
        print(f"{mode} {cname} {pas} {name}: max |out - ref| / A = {measured:.3e}, tau = {tol[name]['tau']:.3e}")
        assert ok, msg


@pytest.mark.gpu
@pytest.mark.parametrize("cname, pas", KEYS, ids=[f"{c}-{p}" for c, p in KEYS])
def test_same_bits_as_the_scalar_load_loop(runs, cname, pas):
    import torch
    for name in _out_shapes(CASES[cname], pas):
        a, ta = _load(runs, "loop", cname, pas, name)
        b, tb = _load(runs, "pipe", cname, pas, name)
        ndiff = int((ta.view(torch.int32) != tb.view(torch.int32)).sum())
        assert a == b, f"{name}: {ndiff} of {ta.numel()} elements differ between the pipelined / grouped launches and the loop of before"
