"""GPU: single launches of every token-wise and pointwise launcher against float64 (loco_debug_pointwise of the diagnostics build vs
tests/token_oracle.py).

Every token_oracle.CASES entry is ONE launch of one launcher on this test's device tensors: LayerNorm forward / tangent / cotangent
(the three register forms C = 320, 640, 1280 and the general form at 8 ... 1024 channels, the in-place call, offset levels |mean| / std
of 0, 50 and 1000), GEGLU kinds 0 - 2 (gates over [-8, 8]; one case in the grid-stride loop), temb in all its branches and temb_proj on
its output, the strided 2x2 sum-pool and nearest x2 on non-square maps, copy, the masked seeds with NaN / Inf planted outside the
mask, ddim_step, latent_sample, lincomb, add -- each launcher with a grid cap once above it.  Batched tensors sit in buffers whose
batch strides exceed the dense size; the padding, like every output, is pre-filled with NaN.  Asserted per case, in this order:
  1. nothing is left unwritten (NaN sentinel, or the seeded accumulate operand) and nothing is written into the padding;
  2. |out - ref| <= tau on every element of every output (ln_fwd's statistics included), tau from the reference alone
     (token_oracle docstrings); the message names the worst element's tensor and index and prints the worst share of tau;
  3. the launches that only move data (copy without accumulate, upsample2x with scale 1 or with 0.25 without accumulate) are bit for
     bit, and the masked-out elements of masked_axpby / cot_seed are exact zeros;
  4. the adjoint identities <ln_tan(d), g> = <d, ln_cot(g)>, <geglu_1(d), g> = <d, geglu_2(g)>, <pool(x), y> = <x, up(y)> hold in
     float64 on the GPU outputs within sum |weight| tau (test_adjoint_identities_hold);
  5. the case stays under 20 s.
What the kernels cannot take must be REFUSED before any launch, with an error that names debug_pointwise
(test_hook_refuses_what_the_launchers_cannot_take).

One child process on the diagnostics build (LOCO_HIP_LIB), one engine (CELEBA_DDPM, synthetic parameters: the hook needs only a
context); no LOCO_* switch is set.  The child is this file run as a script:
    LOCO_HIP_LIB=.../libloco_hip_diag.so python tests/test_gpu_token_oracle.py --worker out.json

Measured on the MI355X (first run), worst share of tau = max |got - ref| / tau per launcher and kind over its cases:
  launcher               cases  worst share of tau
  ln_fwd                    60  y 0.033  stats 0.088
  ln_tan                    30  out 0.012
  ln_cot                    60  out 0.018
  geglu kind 0               2  out 0.082
  geglu kind 1               2  out 0.052
  geglu kind 2               2  out 0.075
  temb                      24  out 0.001
  temb_proj                 24  out 0.001
  pool2x2_sum               13  out 0.095
  upsample2x                13  out 0.190
  copy                       4  out 0.250
  masked_axpby               7  out 0.158
  cot_seed                   7  out 0.250  out2 0.250
  ddim_step                  4  out 0.072  out2 0.108
  latent_sample              2  out 0.051
  lincomb                    6  out 0.050
  add                        2  out 0.250
(0.250 = 1 / MARGIN: one correctly rounded operation against MARGIN u.  All 36 adjoint identities held, the worst at 1e-3 of its
bound; every refusal was refused.  No kernel fault was found.)
(the bounds are worst-case chains; what they must exclude is in tests/test_token_oracle_host.py: every planted error there lands above 1)
"""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_oracle as to     # noqa: E402

CASE_KEYS = [c["id"] for c in to.CASES]
ADJ_KEYS = [a["id"] for a in to.ADJOINTS]
LIMIT_S = 20.0
NAN = float("nan")


def _run_case(eng, torch, c, state):
    op = c["op"]
    inp = to.inputs(c)
    D = torch.float64
    dev = lambda t: t.to(torch.float32).cuda().contiguous()
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device="cuda")
    pads = []                                                # (buffer [B][per + pad], per): the padding must stay NaN

    def pad_in(t, pad):                                      # [B][...] -> a buffer with batch stride per + pad
        B, per = t.shape[0], t[0].numel()
        buf = nan(B, per + pad)
        buf[:, :per] = dev(t).reshape(B, per)
        return buf, per + pad

    def pad_out(B, per, pad, fill=None):
        buf = nan(B, per + pad)
        if fill is not None:
            buf[:, :per] = dev(fill).reshape(B, per)
        pads.append((buf, per))
        return buf, per + pad

    t0 = time.time()
    tact = None
    outs = {}
    if op == "ln_fwd":
        B, C, T = c["B"], c["C"], c["T"]
        x, xbs = pad_in(inp["x"], 40)
        if c.get("inplace"):
            y, ybs = x, xbs
            pads.append((x, C * T))
        else:
            y, ybs = pad_out(B, C * T, 24)
        st, sbs = pad_out(B, 2 * T, 8)
        eng.debug_pointwise(op, B=B, C=C, T=T, eps=c["eps"], x=x, in_bs=xbs, gamma=dev(inp["gamma"]), beta=dev(inp["beta"]), out=y, out_bs=ybs,
                            out2=st, st_bs=sbs)
        outs = dict(y=y[:, :C * T], stats=st[:, :2 * T])
    elif op in ("ln_tan", "ln_cot"):
        B, C, T = c["B"], c["C"], c["T"]
        d, dbs = pad_in(inp["g"] if op == "ln_cot" else inp["d"], 40)
        y, ybs = pad_out(B, C * T, 24)
        kw = {}
        if op == "ln_cot" and c["base"]:
            kw["base"], kw["aux_bs"] = pad_in(inp["base"], 56)
        eng.debug_pointwise(op, B=B, C=C, T=T, x=d, in_bs=dbs, y=dev(inp["prim"]), stats=dev(inp["sprim"]), gamma=dev(inp["gamma"]), out=y,
                            out_bs=ybs, **kw)
        outs = dict(out=y[:, :C * T])
    elif op == "geglu":
        kind, n4, B = c["kind"], c["n4"], c["B"]
        a = {0: inp["f"], 1: inp["df"], 2: inp["g"]}[kind]
        x, xbs = pad_in(a, 12)
        wr = 2 * n4 if kind == 2 else n4
        y, ybs = pad_out(B, wr, 20)
        eng.debug_pointwise(op, kind=kind, B=B, count=n4, x=x, in_bs=xbs, y=dev(inp["f"][0]) if kind else None, out=y, out_bs=ybs)
        outs = dict(out=y[:, :wr])
    elif op == "temb":
        out = nan(c["tch"])
        eng.debug_pointwise(op, C=c["ch"], n=c["tch"], t=c["t"], freq=dev(inp["freq"]), w0=dev(inp["w0"]), b0=dev(inp["b0"]), w1=dev(inp["w1"]),
                            b1=dev(inp["b1"]), add=dev(inp["add"]) if c["add"] else None, add_in=dev(inp["add_in"]) if c["add_in"] else None,
                            act=c["act"], cos_first=c["cos_first"], t_dev=nan(1) if c["ptr"] else None, out=out)
        state["temb"][c["id"]] = out
        outs = dict(out=out)
    elif op == "temb_proj":
        x = state["temb"][c["after"]]                        # the fp32 output of the temb launch before it, taken as given
        tact = x.cpu().to(D)
        out = nan(c["cout"])
        eng.debug_pointwise(op, C=c["cout"], n=c["tch"], x=x, w0=dev(inp["pw"]), b0=dev(inp["pb"]) if c["bias"] else None, out=out)
        outs = dict(out=out)
    elif op in ("pool2x2_sum", "upsample2x"):
        B, C, H, W = c["B"], c["C"], c["H"], c["W"]
        pool = op == "pool2x2_sum"
        x, xbs = pad_in(inp["x"] if pool else inp["y"], 6)
        per = C * H * W * (1 if pool else 4)
        y, ybs = pad_out(B, per, 5 if pool else 10, (inp["small0"] if pool else inp["large0"]) if c["acc"] else None)
        eng.debug_pointwise(op, B=B, C=C, H=H, W=W, scale=c["scale"], accumulate=c["acc"], x=x, in_bs=xbs, out=y, out_bs=ybs)
        outs = dict(out=y[:, :per])
    elif op == "copy":
        B, n = c["B"], c["n"]
        x, xbs = pad_in(inp["x"], 8)
        y, ybs = pad_out(B, n, 12, inp["out0"] if c["acc"] else None)
        eng.debug_pointwise(op, B=B, count=n, accumulate=c["acc"], x=x, in_bs=xbs, out=y, out_bs=ybs)
        outs = dict(out=y[:, :n])
    elif op in ("masked_axpby", "cot_seed"):
        k, n = c["k"], c["n"]
        m8 = lambda m: None if m is None else m.to(torch.uint8).cuda()
        kw = dict(k=k, count=n, split=c["split"], cv=inp["cv"], ce=inp["ce"], mask=m8(inp["mask"]), mask2=m8(inp["mask2"]))
        out = nan(k, n)
        if op == "masked_axpby":
            eng.debug_pointwise(op, x=None if c["null"] else dev(inp["V"]), y=dev(inp["dE"]), out=out, **kw)
            outs = dict(out=out)
        else:
            out2 = None if c["null"] else nan(k, n)
            eng.debug_pointwise(op, x=dev(inp["U"]), out=out, out2=out2, **kw)
            outs = dict(out=out) if c["null"] else dict(out=out, out2=out2)
    elif op == "ddim_step":
        n = c["n"]
        out, out2 = nan(n), nan(n) if c["x0"] else None
        eng.debug_pointwise(op, count=n, x=dev(inp["x"]), y=dev(inp["e"]), base=dev(inp["noise"]) if c["noise"] else None, f=inp["f"], out=out,
                            out2=out2)
        outs = dict(out=out, out2=out2) if c["x0"] else dict(out=out)
    elif op == "latent_sample":
        out = nan(c["B"], c["n"])
        eng.debug_pointwise(op, B=c["B"], count=c["n"], scale=inp["scale"], x=dev(inp["mom"]), base=dev(inp["noise"]) if c["noise"] else None, out=out)
        outs = dict(out=out)
    elif op == "lincomb":
        src = [dev(s) for s in inp["src"]]
        out = src[0] if c["alias"] else nan(c["n"])          # alias: the first source IS the output
        eng.debug_pointwise(op, n=c["nsrc"], count=c["n"], src=src, f=inp["coef"], out=out)
        outs = dict(out=out)
    else:
        assert op == "add", op
        out = nan(c["n"])
        eng.debug_pointwise(op, count=c["n"], x=dev(inp["a"]), y=dev(inp["b"]), out=out)
        outs = dict(out=out)
    torch.cuda.synchronize()
    gpu_s = time.time() - t0
    host = {k: v.cpu() for k, v in outs.items()}
    stray = sum(int((~torch.isnan(buf[:, per:])).sum()) for buf, per in pads)
    refs, info = to.reference(c, inp, tact)
    r = to.check(host, refs, info)
    if c["id"] in state["adj_ids"]:
        state["adj"][c["id"]] = (host["out"].to(D).reshape(refs["out"][0].shape), refs["out"][1])
    return dict(id=c["id"], op=op, key=to.launcher_key(c), share=r["share"], shares=r["shares"], msg=r["msg"], unwritten=r["unwritten"],
                bits_bad=r["bits_bad"], zero_bad=r["zero_bad"], stray=stray, gpu_s=gpu_s, total_s=time.time() - t0)


def _run_adjoint(a, state):
    ca, cb = to.BY_ID[a["a"]], to.BY_ID[a["b"]]
    if a["a"] not in state["adj"] or a["b"] not in state["adj"]:
        return dict(id="adj-" + a["id"], ok=False, msg="a case of the pair did not run")
    (oa, ta), (ob, tb) = state["adj"][a["a"]], state["adj"][a["b"]]
    ia, ib = to.adjoint_io(ca, to.inputs(ca)), to.adjoint_io(cb, to.inputs(cb))
    diff, bound = to.adjoint(ia.reshape(ob.shape), oa, ta, ib.reshape(oa.shape), ob, tb)
    return dict(id="adj-" + a["id"], ok=diff <= bound, diff=diff, bound=bound, msg=f"|<A d, g> - <d, A^T g>| = {diff:.3e} against {bound:.3e}")


REFUSALS = ("ln: T not a multiple of 16", "ln: C < 1", "ln: statistics stride below 2 T", "ln: tangent output on its input",
            "ln: in place with unequal strides", "ln: cotangent output on its base", "geglu: in_bs below 2 n4", "geglu: out_bs below n4",
            "geglu: kind 2 out_bs below 2 n4", "geglu: kind 3", "copy: per_sample not a multiple of 4", "copy: stride not a multiple of 4",
            "pool2x2: odd batch stride", "pool2x2: W = 0", "upsample2x: H = 0", "temb: ch + temb_ch beyond the LDS", "lincomb: n = 0",
            "lincomb: n = 5", "masked_axpby: split > k", "masked_axpby: split < 0", "cot_seed: split > k", "masked_axpby: mask2 without mask",
            "cot_seed: mask2 without mask", "ln_fwd: null gamma", "geglu: null fprim", "temb: null w1", "temb_proj: null w", "pool2x2: null out",
            "copy: null x", "masked_axpby: null dE", "cot_seed: null U", "ddim_step: null eps", "latent_sample: null moments",
            "lincomb: null source", "add: null b", "ln_tan: null primal", "ln_cot: null statistics", "upsample2x: null x", "op out of range")


def _refusals(eng, torch):
    """what the kernels cannot take: each must raise before any launch -> {name: [refused, message]}"""
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    m = lambda n: torch.ones(n, dtype=torch.uint8, device="cuda")
    P = eng.debug_pointwise
    ln = lambda op="ln_fwd", **kw: (lambda: P(op, **dict(dict(B=2, C=8, T=16, eps=1e-5, x=z(2, 128), in_bs=128, gamma=z(8), beta=z(8), out=z(2, 128),
                                                              out_bs=128, out2=z(2, 32), st_bs=32), **kw)))
    lin = lambda op, **kw: ln(op, **dict(dict(beta=None, out2=None, y=z(128), stats=z(32)), **kw))
    buf = z(2, 128)
    geglu = lambda **kw: (lambda: P("geglu", **dict(dict(kind=0, B=2, count=16, x=z(2, 32), in_bs=32, y=z(32), out=z(2, 32), out_bs=32), **kw)))
    copy = lambda **kw: (lambda: P("copy", **dict(dict(B=2, count=8, x=z(2, 8), in_bs=8, out=z(2, 8), out_bs=8), **kw)))
    pool = lambda op="pool2x2_sum", **kw: (lambda: P(op, **dict(dict(B=2, C=1, H=2, W=2, x=z(2, 16), in_bs=16, out=z(2, 16), out_bs=16), **kw)))
    temb = lambda **kw: (lambda: P("temb", **dict(dict(C=4, n=8, t=1.0, freq=z(2), w0=z(8, 4), b0=z(8), w1=z(8, 8), b1=z(8), out=z(8)), **kw)))
    lc = lambda **kw: (lambda: P("lincomb", **dict(dict(n=2, count=8, src=[z(8), z(8)], f=[1.0, 1.0], out=z(8)), **kw)))
    ax = lambda op="masked_axpby", **kw: (lambda: P(op, **dict(dict(k=3, count=8, split=0, cv=1.0, ce=1.0, x=z(3, 8), y=z(3, 8), mask=m(8), mask2=m(8),
                                                                   out=z(3, 8)), **kw)))
    calls = dict(zip(REFUSALS, (
        ln(T=24), ln(C=0), ln(st_bs=31), lin("ln_tan", x=buf, out=buf), ln(x=buf, out=buf, out_bs=136), (lambda b=z(2, 128): lin("ln_cot", base=b, aux_bs=128, out=b)()),
        geglu(in_bs=31), geglu(out_bs=15), geglu(kind=2, x=z(2, 16), in_bs=16, out_bs=31), geglu(kind=3), copy(count=6), copy(in_bs=10),
        pool(in_bs=17), pool(W=0), pool("upsample2x", H=0), temb(C=8192, n=8193), lc(n=0), lc(n=5), ax(split=4), ax(split=-1), ax("cot_seed", split=4),
        ax(mask=None), ax("cot_seed", mask=None), ln(gamma=None), geglu(kind=1, y=None), temb(w1=None),
        (lambda: P("temb_proj", C=4, n=8, x=z(8), w0=None, out=z(4))), pool(out=None), copy(x=None), ax(y=None), ax("cot_seed", x=None),
        (lambda: P("ddim_step", count=8, x=z(8), y=None, out=z(8), f=[1.0, 0.5, 1.0, 0.5, 0.0])),
        (lambda: P("latent_sample", B=1, count=8, x=None, out=z(8))), lc(src=[z(8), None]),
        (lambda: P("add", count=8, x=z(8), y=None, out=z(8))), lin("ln_tan", y=None), lin("ln_cot", stats=None), pool("upsample2x", x=None),
        (lambda: P(15, count=8, x=z(8), y=z(8), out=z(8))))))
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
    import torch
    import loco_edit_amd      # noqa: F401
    import loco_edit_amd.hip as H
    from loco_edit_amd.config import CELEBA_DDPM, synth_params
    torch.set_num_threads(min(16, torch.get_num_threads()))
    eng = H.LocoEngine(CELEBA_DDPM, max_batch=2)
    eng.load_state_dict(synth_params(CELEBA_DDPM, 0))
    results = []
    state = dict(temb={}, adj={}, adj_ids={a[k] for a in to.ADJOINTS for k in ("a", "b")})

    def emit(r):
        print(json.dumps({k: v for k, v in r.items() if k != "msg"}), flush=True)
        results.append(r)
    for c in to.CASES:
        emit(_run_case(eng, torch, c, state))
    for a in to.ADJOINTS:
        emit(_run_adjoint(a, state))
    emit(dict(id="refusals", refusals=_refusals(eng, torch)))
    table = {}
    for r in results:
        if "key" in r:
            e = table.setdefault(r["key"], dict(cases=0, shares={}))
            e["cases"] += 1
            for k, v in r["shares"].items():
                e["shares"][k] = max(e["shares"].get(k, 0.0), v)
    for k, e in table.items():
        print(f"  {k:<22}{e['cases']:>5}  " + "  ".join(f"{n} {v:.3f}" for n, v in e["shares"].items()), flush=True)
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
    out = str(tmp_path_factory.mktemp("token_oracle") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    env["LOCO_HIP_LIB"] = _diag_lib()
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", out], env=env, capture_output=True, text=True, timeout=600)
    done = sum(1 for line in r.stdout.splitlines() if line.startswith("{"))
    total = len(CASE_KEYS) + len(ADJ_KEYS) + 1
    assert r.returncode == 0, f"the worker ended with {r.returncode} after {done} of {total} cases:\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    with open(out) as f:
        return {x["id"]: x for x in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_KEYS)
def test_launch_matches_float64(results, cid):
    r = results[cid]
    assert r["unwritten"] == 0, f"{r['unwritten']} entries were never written (NaN sentinel left); {r['msg']}"
    assert r["stray"] == 0, f"{r['stray']} entries of the padding between the samples were written"
    print(f"{cid}: worst share of tau " + ", ".join(f"{k} {v:.3f}" for k, v in r["shares"].items()))
    assert r["share"] <= 1.0, r["msg"]
    assert r["bits_bad"] == 0, f"{r['bits_bad']} entries of a launch that only moves data are not bit for bit"
    assert r["zero_bad"] == 0, f"{r['zero_bad']} entries outside the mask are not exact zeros"
    assert r["total_s"] < LIMIT_S, f"the case took {r['total_s']:.1f} s"


@pytest.mark.gpu
@pytest.mark.parametrize("aid", ADJ_KEYS)
def test_adjoint_identities_hold(results, aid):
    r = results["adj-" + aid]
    assert r["ok"], r["msg"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", REFUSALS)
def test_hook_refuses_what_the_launchers_cannot_take(results, name):
    refused, msg = results["refusals"]["refusals"][name]
    assert refused, msg
    assert "debug_pointwise" in msg, msg
