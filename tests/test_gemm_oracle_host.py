"""CPU: the GEMM oracle (tests/gemm_oracle.py) against itself, before it judges a kernel.

  - every row of the table passes the oracle's own fault-free emulation of a kernel: float32 arithmetic in the kernels' order (K in
    chunks, the K split of the record GEMM as partial sums, the epilogue term by term), the split-bf16 form for ops 2 and 3;
  - each planted fault FAILS on at least one element, on the rows that can show it;
  - route_of (the launchers' predicates restated) gives the table's expected-route column for every row;
  - every row's operands fit their buffers, the output's addressed floats are distinct and lie between the guard bands.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as go      # noqa: E402

CASE = {c["id"]: c for c in go.CASES}
_CACHE = {}


def _oracle(cid):
    """operands, reference, magnitude and tolerance of a row: computed once, shared, never modified"""
    if cid not in _CACHE:
        case = CASE[cid]
        ops = go.make_operands(case)
        ref, A = go.reference(case, ops), go.magnitude(case, ops)
        _CACHE[cid] = (ops, ref, A, go.tolerance(case, ops, ref, A))
    return _CACHE[cid]


# fault -> the rows that can show it
PLANTED = [
    ("ktail64", "f64_70x45_k65"),                 # ONE k dropped: the smallest tail
    ("ktail64", "f64_70x45_k127"),
    ("ktail64", "small_ctx_kv"),                  # K = 200: the last 8
    ("ktail64", "fixed_inplace_none"),            # K = 72
    ("ktail16", "rec_ragged_tail"),               # K = 264: the zero-filled half record
    ("ktail16", "bf16x3_64"),                     # K = 40
    ("drop_lohi", "bf16x3_64"),
    ("drop_lohi", "bf16x3_128_full"),
    ("drop_lohi", "rec_min"),
    ("bias_n", "fixed_inplace_none"),
    ("r_nohead", "f64_grid320_heads"),
    ("r_nohead", "pipe_full_heads"),
    ("beta_twice", "fixed_inplace_none"),
    ("beta_twice", "fixed_inplace_gelu"),
    ("act_before_res", "fixed_inplace_quick_gelu"),
    ("act_before_res", "fixed_inplace_gelu"),
    ("ksplit_missing", "rec_ksplit3_uneven"),
    ("ksplit_missing", "rec_ksplit4"),
    ("seg2_stride", "small_ctx_kv_seg2"),
    ("seg2_stride", "pipe_full_a1_b0_seg2"),
    ("seg2_stride", "bf16x3_64_seg2"),
    ("seg2_stride", "rec_ksplit3_seg2"),
    ("pair_rowblock", "pair_grouped"),
]


def test_every_fault_is_planted_somewhere():
    assert {f for f, _ in PLANTED} == set(go.FAULTS)


@pytest.mark.parametrize("cid", list(CASE))
def test_fault_free_emulation_passes(cid):
    case = CASE[cid]
    ops, ref, A, tol = _oracle(cid)
    ok, msgs, meas = go.check(case, ops, go.kernel_emulation(case, ops), ref, A, tol)
    for i, (m, t) in enumerate(zip(meas, tol)):
        print(f"{cid} problem {i}: emulation max |out - ref| / A_out = {m:.3e}, tau = {t['tau']:.3e}")
        assert (t["format"] > 0) == (case["op"] in ("gemm_bf16x3", "gemm_rec"))
        assert m < 0.5 * t["tau"], "the fault-free emulation uses more than half of tau"
    assert ok, msgs


@pytest.mark.parametrize("fault, cid", PLANTED, ids=[f"{f}-{c}" for f, c in PLANTED])
def test_planted_fault_fails(fault, cid):
    case = CASE[cid]
    ops, ref, A, tol = _oracle(cid)
    ok, msgs, meas = go.check(case, ops, go.kernel_emulation(case, ops, fault), ref, A, tol)
    print(f"{fault} on {cid}: max |out - ref| / A_out = {max(meas):.3e} against tau = {[t['tau'] for t in tol]}")
    assert not ok, f"the oracle passes a kernel with the fault {fault!r}"


@pytest.mark.parametrize("cid", list(CASE))
def test_route_matches_table(cid):
    case = CASE[cid]
    route = go.route_of(case)
    print(f"{cid}: {go.route_summary(route)}")
    assert go.route_summary(route) == case["expect"]
    names = {"gemm_f32_64", "gemm_f32_small", "gemm_f32_small_pipe", "gemm_f32_pair", "gemm_f32_fixed", "gemm_bf16x3_64",
             "gemm_bf16x3_128", "gemm_rec", "rec_split", "gemm_rec_reduce"}
    assert {r["kernel"] for r in route} <= names


def test_table_reaches_every_kernel_and_layout():
    seen = {r["kernel"] for c in go.CASES for r in go.route_of(c)}
    assert seen >= {"gemm_f32_64", "gemm_f32_small", "gemm_f32_small_pipe", "gemm_f32_pair", "gemm_f32_fixed", "gemm_bf16x3_64",
                    "gemm_bf16x3_128", "gemm_rec", "rec_split", "gemm_rec_reduce"}
    pipe = {(r["akm"], r["bkm"], r["nseg"]) for c in go.CASES for r in go.route_of(c) if r["kernel"] == "gemm_f32_small_pipe"}
    assert pipe == {(a, b, s) for a in (0, 1) for b in (0, 1) for s in (1, 2)}
    rec = {(r["tm"], r["ksplit"]) for c in go.CASES for r in go.route_of(c) if r["kernel"] == "gemm_rec"}
    assert rec >= {(2, 1), (4, 1), (2, 4), (4, 4), (2, 3)}
    assert {r["kcontig"] for c in go.CASES for r in go.route_of(c) if r["kernel"] == "rec_split"} == {0, 1}
    # the grid of 320 workgroups is the first that is not small, and the pipelined kernel's thresholds are each crossed by a row
    assert not go.gemm_small_taken(CASE["f64_grid320_heads"]["probs"][0])
    assert go.gemm_small_taken(go.problem(128, 128, 128, batch=20, heads=4)) is False
    assert go.gemm_small_taken(go.problem(128, 128, 128, batch=79)) is True
    assert go.f32_variant(CASE["small_misaligned_base"]["probs"][0]) == "gemm_f32_small"
    assert go.f32_variant(dict(CASE["small_misaligned_base"]["probs"][0], offA=0)) == "gemm_f32_small_pipe"


@pytest.mark.parametrize("cid", list(CASE) + [r[0] for r in go.REFUSALS])
def test_operands_fit_their_buffers(cid):
    probs = CASE[cid]["probs"] if cid in CASE else next(r[3] for r in go.REFUSALS if r[0] == cid)
    case = dict(CASE[cid]) if cid in CASE else dict(id=cid, op="gemm", act="none", probs=probs)
    ops = go.make_operands(case)
    for p, o in zip(probs, ops):
        for name in go.operand_names(p):
            n = go.count_of(p, name)
            assert o[name].numel() == n
            if name in ("bias", "colbias"):
                assert n >= (p["M"] if name == "bias" else p["N"])
                continue
            idx = go._view(torch.arange(n), p, name)        # the float offsets the launch addresses
            assert 0 <= int(idx.min()) and int(idx.max()) < n
            assert int(idx.min()) == go.base_of(p, name)
        n = go.count_of(p, "C")
        idx = go._view(torch.arange(n), p, "C")
        assert int(idx.min()) == go.GUARD and int(idx.max()) == n - go.GUARD - 1
        assert idx.unique().numel() == idx.numel() == int(go.c_mask(p).sum()), "two output elements share a float"
        if p["R"] == "own":
            assert p["srb"] != p["scb"]
        if p["seg2"]:
            assert p["sab2"] != p["sab"] and p["sbb2"] != p["sbb"]


def test_lipschitz_constants():
    assert go.LIP["none"] == 1.0
    assert 1.09 < go.LIP["quick_gelu"] < 1.11 and 1.12 < go.LIP["gelu"] < 1.14
