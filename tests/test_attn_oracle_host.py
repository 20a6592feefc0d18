"""CPU: the float64 attention oracle (tests/attn_oracle.py) is right and sharp enough -- no GPU.

  1. reference() equals autograd: torch.func.jvp and torch.autograd.grad through softmax(s q^T [K_text | k]) -> [V_text | v] P^T
     in float64, with and without text keys, and the cross-attention restatement likewise.
  2. The error scale A vanishes nowhere: no element of o, do, g_q, g_k, g_v has A < 1e-6 max A, on every row of the table.  (P is
     checked relative to itself, P (1 + |S - rowmax S|); its masked padding columns are exactly 0 and its smallest entries are
     e^-20 of the largest by construction, so the floor does not apply to it.)
  3. Planted faults are rejected: emulated() stands in for a correct kernel and passes; each fault of FAULTS, applied to it, must
     break |out - ref| <= tau A somewhere, on a flash row, a generic row and a cross-attention row (where the fault exists on
     that route).  A tau under which one passes is too loose.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as ao      # noqa: E402

ROW = {r["id"]: r for r in ao.ROWS}


def _fwd_fn(d, kt, vt):
    NH, CH, T, Lt, L = d["NH"], d["CH"], d["T"], d["Lt"], d["L"]
    s = 1.0 / math.sqrt(CH)

    def f(q, k, v):
        qh, kh, vh = (t.reshape(NH, CH, T) for t in (q, k, v))
        if d["kind"] == "cross" or Lt:
            kth, vth = kt.reshape(NH, CH, -1), vt.reshape(NH, CH, -1)
            kh = kth if d["kind"] == "cross" else torch.cat([kth, kh], -1)
            vh = vth if d["kind"] == "cross" else torch.cat([vth, vh], -1)
        S = s * torch.einsum("hci,hcj->hij", qh, kh)
        pad = torch.zeros(S.shape[-1], dtype=torch.bool)
        if d["kind"] == "cross":
            pad[L:] = True
        elif Lt:
            pad[L:Lt] = True
        P = torch.softmax(S.masked_fill(pad, -math.inf), -1)
        return torch.einsum("hcj,hij->hci", vh, P).reshape(NH * CH, T)
    return f


@pytest.mark.parametrize("d", [ao.case("self", 64, 2, 8, 2), ao.case("self", 64, 2, 8, 2, Lt=64, L=5), ao.case("cross", 64, 2, 8, 2, L=7)],
                         ids=["self", "self_text", "cross"])
def test_reference_equals_autograd(d):
    ops = ao.make_operands(d)
    # the exact P and o here: the identity with autograd is an identity of exact arithmetic
    f1 = ao.reference(dict(d, B=1), {k: (v[:1] if k in ("fq", "fk", "fv") else v) for k, v in ops.items()}, "fwd")
    ops = dict(ops, P=f1["P"][0], o=f1["o"][0])
    cross = d["kind"] == "cross"
    q = ops["q"]
    k, v = (q, q) if cross else (ops["k"], ops["v"])
    f = _fwd_fn(d, ops.get("kt"), ops.get("vt"))
    assert torch.allclose(f(q, k, v), ops["o"], rtol=1e-12, atol=1e-13)
    tan, cot = ao.reference(d, ops, "tan"), ao.reference(d, ops, "cot")
    z = torch.zeros_like(q)
    for b in range(d["B"]):
        t = (ops["dq"][b], z, z) if cross else (ops["dq"][b], ops["dk"][b], ops["dv"][b])
        _, jv = torch.func.jvp(f, (q, k, v), t)
        assert torch.allclose(jv, tan["out"][b], rtol=1e-10, atol=1e-12)
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        g = torch.autograd.grad(f(qq, kk, vv), (qq,) if cross else (qq, kk, vv), ops["go"][b])
        for name, gi in zip(("gq", "gk", "gv"), g):
            assert torch.allclose(gi, cot[name][b], rtol=1e-10, atol=1e-12), name


def _sub(row, pas):
    d = ao.case_of(row, pas)
    ops = ao.make_operands(d)
    pr = ao.probes_of(row, pas)
    return ao.sub_case(d, ops, pr[:1]) if pr else (d, ops)


@pytest.mark.parametrize("rid", [r["id"] for r in ao.ROWS if not r["refused"] and r["id"] != "gemm_bf16x3"])
def test_error_scale_vanishes_nowhere(rid):
    row = ROW[rid]
    for pas in row["passes"]:
        d, ops = _sub(row, pas)
        for name, A in ao.magnitude(d, ops, pas).items():
            if name == "P":
                continue
            assert float(A.min()) >= 1e-6 * float(A.max()), f"{rid} {pas} {name}: min A {float(A.min()):.3e} max A {float(A.max()):.3e}"


# fault -> the (row, pass, precision) cases it is planted on; a fault is listed for a route only where it exists there
# (drop_lohi needs a split product; pad_in_softmax and a second scale on the forward scores need the forward; ch64_79 an 80-channel head)
FLASH, FLASH_TXT, GENERIC, CROSS = "flash53_ch80", "flash_text_l5", "generic_text", "cross_lg4"
FAULTS = {
    "swap": [(FLASH, "tan", "bf16x3"), (FLASH, "cot", "bf16x3"), (GENERIC, "tan", "f32"), (CROSS, "tan", "f32")],
    "no_ro": [(FLASH, "tan", "bf16x3"), (FLASH, "cot", "bf16x3"), (GENERIC, "tan", "f32"), (GENERIC, "cot", "f32"), (CROSS, "tan", "f32"),
              (CROSS, "cot", "f32")],
    "skip_last": [(FLASH, "tan", "bf16x3"), (FLASH, "cot", "bf16x3"), (GENERIC, "tan", "f32")],
    "ch64_79": [(FLASH, "tan", "bf16x3"), (FLASH, "cot", "bf16x3")],
    "pad_in_softmax": [(GENERIC, "fwd", "f32"), (CROSS, "fwd", "f32")],
    "scale2_txt": [(FLASH_TXT, "tan", "bf16x3"), (FLASH_TXT, "cot", "bf16x3"), (GENERIC, "fwd", "f32"), (GENERIC, "tan", "f32"),
                   (CROSS, "fwd", "f32"), (CROSS, "tan", "f32")],
    "drop_lohi": [(FLASH, "tan", "bf16x3"), (FLASH, "cot", "bf16x3"), (FLASH_TXT, "tan", "bf16x3")],
}
_cache = {}


def _setup(rid, pas, prec):
    key = (rid, pas, prec)
    if key not in _cache:
        row = ROW[rid]
        d = ao.case_of(row, pas)
        ops = ao.make_operands(d)
        _, flags, flash = ao.route_of(d, pas, prec)
        ref, A = ao.reference(d, ops, pas), ao.magnitude(d, ops, pas)
        _cache[key] = (d, ops, flags, ref, A, ao.tolerance(d, ops, pas, flags, ref, A, flash))
    return _cache[key]


def _passes(d, out, ref, A, tol):
    return all(ao.worst(n, out[n], ref[n], A[n], tol[n]["tau"], d)[0] for n in ref)


def test_fault_rows_take_the_routes_they_stand_for():
    assert ROW[FLASH]["case"]["T"] <= 384 and ao.route_of(ROW[FLASH]["case"], "tan", "bf16x3")[2]
    assert ao.route_of(ROW[FLASH_TXT]["case"], "tan", "bf16x3")[2]
    assert not ao.route_of(ROW[GENERIC]["case"], "tan", "bf16x3")[2]
    assert ao.route_of(ROW[CROSS]["case"], "tan", "f32")[0][0]["kernel"] == "xattn_fused_lin"


@pytest.mark.parametrize("rid, pas, prec", sorted({c for cs in FAULTS.values() for c in cs}))
def test_emulated_kernel_passes(rid, pas, prec):
    d, ops, flags, ref, A, tol = _setup(rid, pas, prec)
    assert _passes(d, ao.emulated(d, ops, pas, flags), ref, A, tol)


@pytest.mark.parametrize("fault, rid, pas, prec", [(f, *c) for f, cs in FAULTS.items() for c in cs])
def test_planted_fault_is_rejected(fault, rid, pas, prec):
    d, ops, flags, ref, A, tol = _setup(rid, pas, prec)
    out = ao.emulated(d, ops, pas, flags, fault=fault)
    print({n: (t["tau"], float(((out[n] - ref[n]).abs() / A[n].clamp_min(1e-300)).max())) for n, t in tol.items()})
    assert not _passes(d, out, ref, A, tol), f"{fault} on {rid} {pas} {prec} stays within tau = { {n: t['tau'] for n, t in tol.items()} }"


def test_route_table_names_every_kernel_family():
    seen = set()
    for rid, pas, prec, ws in ao.keys():
        row = ROW[rid]
        if row["refused"]:
            continue
        lines, _, _ = ao.route_of(ao.case_of(row, pas), pas, "bf16x3" if prec == "f16" else prec, ws, row["rec"])
        seen |= {l["kernel"] for l in lines}
    assert seen == {"attn_split", "flash_dma_tan", "flash_dma_cotq", "flash_dma_cotk", "flash_tan", "flash_cotq", "flash_cotk", "gemm_rec",
                    "gemm_bf16x3", "gemm_f32", "softmax_rows", "softmax_jac", "xattn_fused_fwd", "xattn_fused_lin"}


def test_check_route_and_parse():
    text = "kernel=attn_split\nkernel=gemm_rec M=1024 N=1024 K=256 batch=8 heads=1 kcat=1\n"
    r = ao.parse_route(text)
    assert r[1]["M"] == 1024 and r[0] == dict(kernel="attn_split")
    assert not ao.check_route(r, [dict(kernel="attn_split"), dict(kernel="gemm_rec", M=1024, kcat=1)])
    assert ao.check_route(r, [dict(kernel="attn_split"), dict(kernel="gemm_rec", M=1024, kcat=0)])
    assert ao.check_route(r, [dict(kernel="gemm_rec")])
