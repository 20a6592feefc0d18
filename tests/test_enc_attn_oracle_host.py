"""CPU: the float64 oracle of the encoders' attention launches (tests/enc_attn_oracle.py) is right and sharp enough -- no GPU.

  1. reference() equals torch: the forward ops against torch.nn.functional.scaled_dot_product_attention in float64 with an additive
     mask built from the tables, the causal rule and lens; the cotangent (ops 5, 6) against autograd through that; sd_t2i / sd_i2t
     against the torch decoder statement the mask-head tests compare with (mask_segmentation.SamHead._attn, identity projections).
  2. emulated() -- the kernels' fixed-order chunked algorithms in float32 -- stays below tau A on EVERY row of the table: the cap is
     reachable, from the reference side alone.
  3. With each fault of FAULTS planted into it, at least one row of the table exceeds tau A.  A tau under which one passes is too loose.
  4. The table: the route of every row follows from its case; the chunk thresholds the cotangent kernels' comment states agree
     with the LDS formula; every row that runs fits 64 KiB and every LDS refusal exceeds it; the lens cover the edges.
"""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import enc_attn_oracle as eo      # noqa: E402

ROW = {r["id"]: r for r in eo.ROWS}
RUN = [r for r in eo.ROWS if not r["refused"]]
_cache = {}


def _setup(rid):
    if rid not in _cache:
        c = ROW[rid]["case"]
        ops = eo.make_operands(c)
        ref, A = eo.reference(c, ops), eo.magnitude(c, ops)
        _cache[rid] = (c, ops, ref, A, eo.tolerance(c, ops))
    return _cache[rid]


def _mask(c, ops):
    """the additive mask [G][H][Tq][Tk] of a forward op: tables, causal rule, lens"""
    op, G, H, nk = c["op"], c["groups"], c["heads"], c["nk"]
    i, j = torch.arange(nk).unsqueeze(1), torch.arange(nk).unsqueeze(0)
    M = torch.zeros(G, H, nk, nk, dtype=torch.float64)
    if op == 2:
        size = c["size"]
        relh, relw = ops["relh"].reshape(H, G, nk, size), ops["relw"].reshape(H, G, nk, size)
        for g in range(G):
            for key in range(nk):
                M[g, :, :, key] = relh[:, g, :, key // size] + relw[:, g, :, key % size]
    if op == 3:
        M = M.masked_fill(j > i, -math.inf)
    if op == 4:
        for h in range(H):
            for a in range(nk):
                for b in range(nk):
                    M[:, h, a, b] = ops["bias_tab"][h, b - a + nk - 1]
        for p, n in enumerate(c["lens"]):
            M[p, :, :, n:] = -math.inf
    return M


def _sdpa(c, q, k, v, M):
    """[G][H][hd][T] operands through torch's attention; T5 (op 4) has no scale"""
    t = lambda x: x.transpose(-1, -2)
    return t(F.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=M, scale=eo.scale_of(c)))


FWD = ["plain_17x16x2x3_spread", "plain_82x80x2x2_late", "bias_3x16x2x4_spread", "bias_10x80x2x1_late", "causal_7x16x2x3_spread",
       "causal_65x32x1x2_late", "t5_7x16x2x3_spread", "t5_65x32x1x2_late", "seg_37x8x2x2_spread"]


@pytest.mark.parametrize("rid", FWD)
def test_forward_reference_equals_torch_sdpa(rid):
    c, ops, ref, _, _ = _setup(rid)
    want = _sdpa(c, ops["q"], ops["k"], ops["v"], _mask(c, ops))
    assert torch.allclose(ref["out"], want, rtol=1e-11, atol=1e-12)


def test_kept_statistics_are_the_log_sum_exp():
    c, ops, ref, _, _ = _setup("keep_82x80x2x2_late")
    S = eo.scores(c, ops, torch.float64)
    assert torch.allclose(ref["lse"].squeeze(2), torch.logsumexp(S, -1), rtol=1e-12, atol=1e-12)
    assert torch.equal(ref["m"].squeeze(2), S.max(-1).values)
    assert torch.equal(ref["out"], eo.reference(ROW["plain_82x80x2x2_late"]["case"], ops)["out"])


@pytest.mark.parametrize("shape", [(17, 16, 2, 2), (82, 80, 2, 2)])
def test_cotangent_reference_equals_autograd(shape):
    T, hd, H, G = shape
    c5 = eo.case(5, T, hd, H, G)
    ops = eo.make_operands(c5)
    # the exact m, l, o here: the identity with autograd is one of exact arithmetic
    S = eo.scores(c5, ops, torch.float64)
    m = S.max(-1).values
    l = torch.exp(S - m.unsqueeze(-1)).sum(-1)
    o = torch.einsum("ghij,ghcj->ghci", torch.softmax(S, -1), ops["v"])
    ops = dict(ops, m=m.unsqueeze(2), l=l.unsqueeze(2), o=o)
    q, k, v = (ops[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    out = _sdpa(c5, q, k, v, None)
    assert torch.allclose(out, o, rtol=1e-11, atol=1e-12)
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), ops["go"])
    r5 = eo.reference(c5, ops)
    assert torch.allclose(r5["gq"], gq, rtol=1e-10, atol=1e-12)
    assert torch.allclose(r5["delta"], (ops["go"] * o).sum(2, keepdim=True), rtol=1e-12, atol=1e-13)
    r6 = eo.reference(dict(c5, op=6), dict(ops, delta=r5["delta"]))
    assert torch.allclose(r6["gk"], gk, rtol=1e-10, atol=1e-12)
    assert torch.allclose(r6["gv"], gv, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("rid", ["t2i_kbs_196x32x2x3x8_late", "t2i_36x16x2x2x7_spread", "i2t_qbs_36x48x16x2x2x7_spread", "i2t_64x64x8x2x3x1_spread"])
def test_decoder_attention_reference_equals_the_torch_decoder(rid):
    from loco_edit_amd import mask_segmentation as ms
    c, ops, ref, _, _ = _setup(rid)
    H, hd, G = c["heads"], c["hd"], c["groups"]
    Ci = H * hd
    head = ms.SamHead.__new__(ms.SamHead)
    head.cfg = SimpleNamespace(decoder=SimpleNamespace(num_attention_heads=H))
    head.p = {}
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        head.p[f"a.{n}.weight"], head.p[f"a.{n}.bias"] = torch.eye(Ci, dtype=torch.float64), torch.zeros(Ci, dtype=torch.float64)
    # logical [g][H][hd][T] -> the decoder's [B][T][Ci]
    tok = lambda x: x.expand(G, -1, -1, -1).permute(0, 3, 1, 2).reshape(G, x.shape[-1], Ci)
    want = head._attn("a", tok(ops["q"]), tok(ops["k"]), tok(ops["v"]))                 # [G][Tq][Ci]
    got = ref["out"].permute(0, 3, 1, 2).reshape(G, -1, Ci)
    # the decoder scales by hd ** -0.5 in float64, the launch receives the float32 scale: scores differ by 3e-8 relative
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


def _passes(c, out, ref, A, tol):
    return all(eo.worst(n, out[n].to(torch.float64), ref[n], A[n], tol[n]["tau"])[0] for n in ref)


@pytest.mark.parametrize("rid", [r["id"] for r in RUN])
def test_emulated_kernel_stays_under_tau(rid):
    c, ops, ref, A, tol = _setup(rid)
    out = eo.emulated(c, ops)
    for n in ref:
        ok, msg, measured = eo.worst(n, out[n].to(torch.float64), ref[n], A[n], tol[n]["tau"])
        print(f"{rid} {n}: max |emu - ref| / A = {measured:.3e}, tau = {tol[n]['tau']:.3e}")
        assert ok, msg
        assert float(A[n].min()) > 0, f"{n}: the error scale vanishes somewhere"


# fault -> the ops it exists on
FAULT_OPS = {"l_not_rescaled": (0, 1, 2, 8), "o_not_rescaled": (0, 1, 2, 8), "skip_last_chunk": (0, 1, 2, 8), "pad_p1": (0, 1, 2, 8),
             "rel_swapped": (2,), "bias_shift": (4,), "causal_strict": (3,), "len_inclusive": (4,), "drop_c64": (0, 1, 2, 5, 6),
             "no_delta": (5, 6), "dk_no_scale": (6,), "merge_no_factor": (8,)}


def test_every_fault_is_listed():
    assert set(FAULT_OPS) == set(eo.FAULTS)


@pytest.mark.parametrize("fault, op", [(f, op) for f, ops in FAULT_OPS.items() for op in ops])
def test_planted_fault_is_rejected(fault, op):
    caught = []
    for r in RUN:
        if r["case"]["op"] != op:
            continue
        c, ops, ref, A, tol = _setup(r["id"])
        if not _passes(c, eo.emulated(c, ops, fault), ref, A, tol):
            caught.append(r["id"])
    print(fault, op, caught)
    assert caught, f"{fault} passes every row of op {op}"


def test_late_profile_raises_the_maximum_in_every_chunk():
    # (rows without tables: the tables of op 2, of variance 1, ride on the ramp and may move a maximum by a chunk)
    for rid in ("plain_130x8x1x1_late", "t2i_400x32x1x1x5_late", "keep_82x80x2x2_late", "seg_130x64x1x2_late"):
        c, ops, _, _, _ = _setup(rid)
        S = eo.scores(c, ops, torch.float64)
        chunks = [S[..., k0:k0 + eo.KC].max(-1).values for k0 in range(0, S.shape[-1], eo.KC)]
        for a, b in zip(chunks, chunks[1:]):
            assert bool((b > a).all()), rid
        spread = (S.max(-1).values - S.min(-1).values)
        assert 20 < float(spread.min()) and float(spread.max()) < 45, (rid, float(spread.min()), float(spread.max()))


def test_spread_profile_has_score_variance_about_three():
    for rid in ("plain_82x80x2x2_spread", "t5_128x32x2x1_spread", "seg_130x64x1x2_spread"):
        c, ops, _, _, _ = _setup(rid)
        S = eo.scores(c, ops, torch.float64)
        S = S[torch.isfinite(S).all(-1)]
        assert 1.5 < float(S.var(-1).mean()) < 6.0, rid


def test_table_routes_and_thresholds():
    seen = set()
    for r in RUN:
        c = r["case"]
        (line,) = eo.expected_route(c)
        seen.add(tuple(sorted(line.items())))
        op, hd = c["op"], c["hd"]
        if op <= 2:
            assert eo.enc_attn_lds_bytes(hd, c["size"]) <= 65536, r["id"]
        elif op <= 4:
            assert eo.prompt_attn_lds_bytes(hd, c["nk"]) <= 65536 and c["nk"] <= 128, r["id"]
        elif op <= 6:
            tables = 1 if op == 5 else 2
            # the comment's thresholds (cot_chunk) against the formula the launcher branches on
            assert (eo.cot_lds_bytes(hd, 64, tables) <= 65536) == (eo.cot_chunk(c) == 64), r["id"]
            assert eo.cot_lds_bytes(hd, eo.cot_chunk(c), tables) <= 65536, r["id"]
        elif op == 8:
            assert eo.sd_t2i_lds_bytes(hd) <= 65536, r["id"]
    for hd in range(1, 129):
        for op in (5, 6):
            assert (eo.cot_lds_bytes(hd, 64, 1 if op == 5 else 2) <= 65536) == (eo.cot_chunk(dict(op=op, hd=hd)) == 64), (op, hd)
    chunks = {(dict(k)["kernel"], dict(k)["chunk"]) for k in seen if "chunk" in dict(k)}
    assert chunks == {("clipvis_attn_cot_q", 64), ("clipvis_attn_cot_q", 32), ("clipvis_attn_cot_kv", 64), ("clipvis_attn_cot_kv", 32)}
    assert {dict(k)["hd"] for k in seen if dict(k)["kernel"] == "seg_attn"} == {4, 8, 16, 32, 64}
    assert {dict(k)["kernel"] for k in seen} == {"enc_attn", "prompt_attn", "clipvis_attn_cot_q", "clipvis_attn_cot_kv", "seg_attn", "sd_t2i",
                                                "sd_i2t"}
    assert eo.enc_attn_lds_bytes(106, 0) <= 65536 < eo.enc_attn_lds_bytes(107, 0)      # 106: the widest head of ops 0 and 1
    assert eo.sd_t2i_lds_bytes(32) <= 65536 < eo.sd_t2i_lds_bytes(64)                  # 32: the widest head of op 8
    lds = {"refused_lds_enc": eo.enc_attn_lds_bytes(128, 0), "refused_lds_prompt": eo.prompt_attn_lds_bytes(64, 128),
           "refused_lds_t2i": eo.sd_t2i_lds_bytes(64)}
    assert all(v > 65536 for v in lds.values()), lds
    lens = [n for r in RUN if r["case"]["op"] == 4 for n in r["case"]["lens"]]
    Ls = [(n, r["case"]["nk"]) for r in RUN if r["case"]["op"] == 4 for n in r["case"]["lens"]]
    assert {1, 2, 63, 64, 65} <= set(lens) and any(n == L - 1 for n, L in Ls) and any(n == L for n, L in Ls)
    assert eo.parse_route("kernel=enc_attn bias=0 keep=1\n") == [dict(kernel="enc_attn", bias=0, keep=1)]
    assert len({r["id"] for r in eo.ROWS}) == len(eo.ROWS)
