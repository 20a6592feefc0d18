"""CPU: the float64 conv reference of tests/conv_oracle.py against torch.autograd, its case table against the host-compiled
planner, and the check of tests/test_gpu_conv_oracle.py against planted errors.

  - reference() means what kernels.h says: modes 1 / 2 / 5 are the forward of GroupNorm -> activation -> conv built from
    torch.nn.functional, mode 3 is torch.func.jvp through norm + activation followed by the conv, mode 4 on the transposed
    operator composes to torch.func.vjp of the chain, the norm-cotangent term is the vjp of the norm it stands for, stride-2
    zero insertion + flipped weights is conv_transpose2d(stride=2), all in float64;
  - every row of the table reaches the kernel family it names under conv_plan.hip compiled with g++ (tests/c/conv_plan_cases.cpp
    prints the plan in the words loco_debug_conv uses), for every precision the row runs under;
  - no row has an output whose error scale A vanishes (A >= 1e-6 max A everywhere);
  - with emulated(bf16x3) standing in for a correct kernel, the check rejects one weight tap of one cout zeroed, two input
    columns (x = 31 / 32, or the last two of a narrower map) swapped, the last cout row shifted by one pixel, and m2 dropped in
    mode 3 -- on a tile-5 3x3 row, a split-K row and a GEMM row.  A tau under which one of these passes is too loose.
"""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import conv_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
D = torch.float64


def _close(a, b, tol=1e-11):
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= tol * max(scale, 1.0), (float((a - b).abs().max()), scale)


def _gn(x, G, gamma, beta):
    return F.group_norm(x, G, gamma, beta, eps=co.GN_EPS)


def _norm_ops(x0, G, gamma, beta):
    """sc, sh, mr of the GroupNorm (gamma, beta, G groups) over x0 [C][H][W], as the engine's statistics define them"""
    C = x0.shape[0]
    xg = x0.reshape(G, -1)
    mean, rstd = xg.mean(1), 1.0 / torch.sqrt(xg.var(1, unbiased=False) + co.GN_EPS)
    rs, mn = co._per_channel(rstd, C // G), co._per_channel(mean, C // G)
    return gamma * rs, beta - mn * rs * gamma, torch.stack([mean, rstd], 1)


@pytest.mark.parametrize("mode, act", [(1, F.silu), (5, lambda y: F.gelu(y)), (2, lambda y: y)])
def test_forward_modes_are_groupnorm_activation_conv(mode, act):
    g = torch.Generator().manual_seed(1)
    C, Co, H, G = 8, 5, 6, 2
    x = torch.randn(1, C, H, H, generator=g, dtype=D) + 2.0
    gamma, beta = torch.randn(C, generator=g, dtype=D), torch.randn(C, generator=g, dtype=D)
    w, b = torch.randn(Co, C, 3, 3, generator=g, dtype=D), torch.randn(Co, generator=g, dtype=D)
    sc, sh, _ = _norm_ops(x[0], G, gamma, beta)
    d = co.case(9, C, Co, H, B=1, mode=mode)
    got = co.reference(d, dict({"in": x, "weight": w, "bias": b, "sc": sc, "sh": sh}))
    _close(got, F.conv2d(act(_gn(x, G, gamma, beta)), w, b, padding=1))


def _lin_setup(B=2):
    g = torch.Generator().manual_seed(2)
    C, Co, H, G = 8, 6, 6, 2
    x = torch.randn(1, C, H, H, generator=g, dtype=D) * 0.7 + 1.5
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g, dtype=D), torch.randn(C, generator=g, dtype=D)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=D)
    sc, sh, mr = _norm_ops(x[0], G, gamma, beta)
    xh = (x[0] - co._per_channel(mr[:, 0], C // G).view(-1, 1, 1)) * co._per_channel(mr[:, 1], C // G).view(-1, 1, 1)
    return g, C, Co, H, G, x, gamma, beta, w, sc, sh, mr, xh


def test_mode3_is_the_jvp_of_norm_activation_followed_by_the_conv():
    g, C, Co, H, G, x, gamma, beta, w, sc, sh, mr, xh = _lin_setup()
    B = 2
    v = torch.randn(B, C, H, H, generator=g, dtype=D)
    f = lambda t: F.silu(_gn(t, G, gamma, beta))
    want = torch.cat([F.conv2d(torch.func.jvp(f, (x,), (v[b:b + 1],))[1], w, padding=1) for b in range(B)])
    m1 = v.reshape(B, G, -1).mean(2)
    m2 = (v * xh).reshape(B, G, -1).mean(2)
    d = co.case(9, C, Co, H, B=B, mode=3, cpg=C // G)
    ops = {"in": v, "weight": w, "prim": x[0], "sc": sc, "sh": sh, "mr": mr, "gamma": gamma, "tst": torch.stack([m1, m2], 2)}
    _close(co.reference(d, ops), want)


def test_mode4_on_the_transposed_operator_composes_to_the_vjp_of_the_chain():
    """The chain u -> conv_prev -> GroupNorm -> SiLU, cotangent g_a of the activation coming in: the engine hands the
    norm + activation cotangent rstd (gamma silu'(y) g_a - m1 - xhat m2) to conv_prev's dgrad as that launch's prologue (mode 4
    on the transposed operator), with m1, m2 the group means of z = gamma silu'(y) g_a and of xhat z.  The launch must equal
    torch.func.vjp of the whole chain."""
    g, C, Co, H, G, x, gamma, beta, w, sc, sh, mr, xh = _lin_setup()
    B = 2
    wprev = torch.randn(C, 4, 3, 3, generator=g, dtype=D)      # the module before the norm: 4 -> C channels
    u = torch.randn(1, 4, H, H, generator=g, dtype=D)
    ga = torch.randn(B, C, H, H, generator=g, dtype=D)
    chain = lambda t: F.silu(_gn(F.conv2d(t, wprev, padding=1) + (x - F.conv2d(u, wprev, padding=1)), G, gamma, beta))
    want = torch.cat([torch.func.vjp(chain, u)[1](ga[b:b + 1])[0] for b in range(B)])
    z = (gamma.view(-1, 1, 1) * co._dsilu(sc.view(-1, 1, 1) * x[0] + sh.view(-1, 1, 1))) * ga
    m1 = z.reshape(B, G, -1).mean(2)
    m2 = (z * xh).reshape(B, G, -1).mean(2)
    d = co.case(9, C, 4, H, B=B, mode=4, cpg=C // G, transposed=1, bias=False)
    ops = {"in": ga, "weight": wprev, "prim": x[0], "sc": sc, "sh": sh, "mr": mr, "gamma": gamma, "tst": torch.stack([m1, m2], 2)}
    _close(co.reference(d, ops), want)


def test_cot_term_is_the_vjp_of_the_norm_it_stands_for():
    """out = nin^T g_out + norm^T g_a: a 1x1 dgrad plus the cotangent of GroupNorm + SiLU over the OUTPUT tensor's primal"""
    g, C, Co, H, G, x, gamma, beta, w, sc, sh, mr, xh = _lin_setup()
    B = 2
    nin = torch.randn(5, C, 1, 1, generator=g, dtype=D)          # forward C -> 5; its dgrad maps 5 -> C
    gout = torch.randn(B, 5, H, H, generator=g, dtype=D)
    ga = torch.randn(B, C, H, H, generator=g, dtype=D)
    f = lambda t: F.silu(_gn(t, G, gamma, beta))
    want = torch.cat([F.conv_transpose2d(gout[b:b + 1], nin) + torch.func.vjp(f, x)[1](ga[b:b + 1])[0] for b in range(B)])
    z = (gamma.view(-1, 1, 1) * co._dsilu(sc.view(-1, 1, 1) * x[0] + sh.view(-1, 1, 1))) * ga
    m1 = co._per_channel(z.reshape(B, G, -1).mean(2), C // G)
    m2 = co._per_channel((z * xh).reshape(B, G, -1).mean(2), C // G)
    d = co.case(1, 5, C, H, B=B, transposed=1, bias=False, cot=True, cot_cpg=C // G)
    ops = {"in": gout, "weight": nin, "cot_d": ga, "cot_prim": x[0], "cot_sc": sc, "cot_sh": sh, "cot_mr": mr,
           "cot_tc": torch.stack([m1, m2], 2)}
    _close(co.reference(d, ops), want)
    assert float((co.magnitude(d, ops) - co.reference(d, ops).abs()).min()) >= -1e-12


def test_input_paths_are_the_torch_operators():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=D)
    w = torch.randn(6, 4, 3, 3, generator=g, dtype=D)
    # stride 2 with the zero row / column at the bottom / right (the DDPM Downsample)
    _close(co.reference(co.case(9, 4, 6, 8, B=2, stride=2, bias=False), {"in": x, "weight": w}),
           F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2))
    # its data gradient: zero insertion + flipped weights = conv_transpose2d(stride 2), cropped to the input's size
    gy = torch.randn(2, 6, 4, 4, generator=g, dtype=D)
    want = torch.func.vjp(lambda t: F.conv2d(F.pad(t, (0, 1, 0, 1)), w, stride=2), x)[1](gy)[0]
    _close(want, F.conv_transpose2d(gy, w, stride=2)[:, :, :8, :8])
    _close(co.reference(co.case(9, 6, 4, 4, B=2, zins=1, transposed=1, bias=False), {"in": gy, "weight": w}), want)
    # nearest x2 upsample ahead of the conv
    _close(co.reference(co.case(9, 4, 6, 8, B=2, upsample=1, bias=False), {"in": x, "weight": w}),
           F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1))
    # stride-1 dgrad, 1x1, epilogue terms, second operator
    gy = torch.randn(2, 6, 8, 8, generator=g, dtype=D)
    _close(co.reference(co.case(9, 6, 4, 8, B=2, transposed=1, bias=False), {"in": gy, "weight": w}), F.conv_transpose2d(gy, w, padding=1))
    b, b2, res, out0 = (torch.randn(*s, generator=g, dtype=D) for s in ((6,), (2, 6), (2, 6, 8, 8), (2, 6, 8, 8)))
    in2, w2, b2nd = (torch.randn(*s, generator=g, dtype=D) for s in ((2, 3, 8, 8), (6, 3, 1, 1), (6,)))
    d = co.case(9, 4, 6, 8, B=2, bias2=True, res=True, res_scale=0.5, accumulate=1, Cin2=3)
    ops = {"in": x, "weight": w, "bias": b, "bias2": b2, "res": res, "out0": out0, "in2": in2, "w2": w2, "bias2nd": b2nd}
    _close(co.reference(d, ops), out0 + F.conv2d(x, w, b, padding=1) + b2.view(2, 6, 1, 1) + 0.5 * res + F.conv2d(in2, w2, b2nd))
    for p in ("f32", "bf16x3", "f16"):      # the emulation is the reference up to the format
        lim = {"f32": 0.0, "bf16x3": 1e-4, "f16": 2e-3}[p]
        assert float(((co.emulated(d, ops, p) - co.reference(d, ops)).abs() / co.magnitude(d, ops)).max()) <= lim


def test_bf16x3_emulation_is_the_three_kept_products():
    g = torch.Generator().manual_seed(4)
    d = co.case(9, 5, 4, 6, B=1, bias=False)
    ops = {"in": torch.randn(1, 5, 6, 6, generator=g, dtype=D), "weight": torch.randn(4, 5, 3, 3, generator=g, dtype=D)}
    (ah, al), (wh, wl) = co._split(ops["in"]), co._split(ops["weight"])
    want = F.conv2d(ah, wh, padding=1) + F.conv2d(ah, wl, padding=1) + F.conv2d(al, wh, padding=1)
    _close(co.emulated(d, ops, "bf16x3"), want, 1e-13)


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
    keys = [(r["id"], p) for r in co.ROWS for p in r["precs"]]
    text = "".join(co.plan_line(r["case"], p) + "\n" for r in co.ROWS for p in r["precs"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOCO_")}
    r = subprocess.run([exe], input=text, env=env, capture_output=True, text=True, timeout=120, check=True)
    chunks = r.stdout.split("case ")[1:]
    assert len(chunks) == len(keys)
    return {k: co.parse_plan(c.split("\n", 1)[1]) for k, c in zip(keys, chunks)}


def test_every_row_reaches_the_family_it_names(plans):
    bad = []
    for r in co.ROWS:
        for p in r["precs"]:
            for msg in co.check_plan(plans[(r["id"], p)], r["expect"][p], r["case"]):
                bad.append(f"{r['family']} / {r['id']} / {p}: {msg}")
    assert not bad, "\n".join(bad)


def test_table_covers_every_family():
    fams = {r["family"] for r in co.ROWS}
    assert fams >= {"f32 tiles", "f32 split-K", "lowp tile 3", "lowp tile 5", "ragged", "lowp split-K", "stride 2", "upsample",
                    "zero-insert dgrad", "dgrad stride 1", "1x1 tiles", "GEMM tm=4 split", "GEMM tm=4", "GEMM tm=2", "GEMM declined",
                    "tap-pair", "pair declined", "kcat", "tail split", "cot epilogue"}
    assert len({r["id"] for r in co.ROWS}) == len(co.ROWS)


def test_no_output_has_a_vanishing_error_scale():
    """A >= 1e-6 max(A) on every output of every row: the componentwise check excludes nothing"""
    for r in co.ROWS:
        d, ops = r["case"], co.make_operands(r["case"])
        if r["probes"]:
            d, ops = co.sub_case(d, ops, r["probes"][:1])
        A = co.magnitude(d, ops)
        assert float(A.min()) >= 1e-6 * float(A.max()), r["id"]


# ---- the check must be able to fail -------------------------------------------------------------------------------------------

def _planted(d, ops, kind):
    """operands (or a transformation of the output) carrying one planted kernel error"""
    o = dict(ops)
    post = lambda out: out
    if kind == "tap":                  # one weight tap of one cout zeroed
        w = ops["weight"].clone()
        w[d["Cout"] // 2, :, w.shape[2] // 2, w.shape[3] // 2] = 0
        o["weight"] = w
    elif kind == "columns":            # two neighbouring input columns swapped (x = 31 / 32 where the map has them)
        x = ops["in"].clone()
        c = 31 if d["W"] > 32 else d["W"] - 2
        x[..., [c, c + 1]] = x[..., [c + 1, c]]
        o["in"] = x
    elif kind == "last_row":           # the last cout row shifted by one pixel
        def post(out):
            out = out.clone()
            out[:, -1] = torch.roll(out[:, -1], 1, dims=-1)
            return out
    elif kind == "m2":                 # m2 dropped from the tangent prologue
        t = ops["tst"].clone()
        t[:, :, 1] = 0
        o["tst"] = t
    return o, post


PLANT_ROWS = {
    "tile5": co.case(9, 48, 64, 16, B=2, mode=3),
    "splitk": co.case(9, 512, 128, 16, B=2, mode=3),
    "gemm": co.case(1, 320, 1280, 16, B=1, mode=0),
}


@pytest.mark.parametrize("row", list(PLANT_ROWS))
@pytest.mark.parametrize("kind", ["none", "tap", "columns", "last_row", "m2"])
def test_planted_errors_are_rejected(row, kind):
    d = PLANT_ROWS[row]
    if kind == "m2" and d["mode"] != 3:
        d = dict(d, mode=3, cpg=d["Cin"] // 8)      # (the GEMM kernel takes modes 0 and 2 only: the check itself is what is tested)
    ops = co.make_operands(d)
    ref, A = co.reference(d, ops), co.magnitude(d, ops)
    tau = co.tolerance(d, ops, "bf16x3", ref, A)["tau"]
    bad_ops, post = _planted(d, ops, kind)
    out = post(co.emulated(d, bad_ops, "bf16x3"))
    ok, msg = co.worst(out, ref, A, tau)
    if kind == "none":
        assert ok, msg
        assert not co.worst(torch.where(torch.arange(out.numel()).view(out.shape) == 5, float("nan"), out), ref, A, tau)[0]
    else:
        assert not ok, f"{kind} passes under tau = {tau:.3e}: {msg}"
