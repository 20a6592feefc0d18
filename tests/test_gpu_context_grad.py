"""GPU tests of the prompt-state gradient, loco_pmp_vjp_context / LocoEngine.pmp_vjp(U, context_grad=True): G[p] =
U[p]^T d f / d tokens through every cross-attention stage of the cotangent pass (csrc/xattn_ctx.hip, the strided-GEMM route,
the projection back through the key / value weights).

Reference: float64 autograd of oracle/loco_oracle.unet_forward_adm with respect to `context` (tests/context_grad_oracle.py).
Error bars, by the project's yardstick rule: in the exact-fp32 mode rel-L2(G) <= 4 x the rel-L2 of the same restatement run
in fp32 on the host against its float64 run; in the split-bf16 mode <= 4 x max(that yardstick, the rel-L2 of the unchanged A
rows of the same call against float64) -- the surrounding convs set the error there, and A is code this gradient does not
touch.  Both numbers are printed per case."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loco_edit_amd  # noqa: E402,F401
import context_grad_oracle as cgo  # noqa: E402
from context_grad_oracle import AT_REF, T_REF, rel  # noqa: E402
from loco_edit_amd.config import TINY_DDPM, TINY_IF, synth_params  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine(r, prec="f32", max_batch=4):
    from loco_edit_amd.hip import LocoEngine
    eng = LocoEngine(r["cfg"], max_batch=max_batch, device=torch.device(DEV))
    eng.load_state_dict(r["params"])
    eng.set_precision(prec)
    eng.set_context(r["ctx"].to(DEV).contiguous())
    return eng


def _primal(eng, r, use_et=True):
    m = r["mask"]
    eng.pmp_primal(r["z"].to(DEV), T_REF, AT_REF, None if m is None else m.to(DEV), use_et=use_et)


# (case, use_et, generic): `generic` = LOCO_FUSE_XATTN=0, set before the engine is created
CASES = [("tiny_ldm", True, False), ("tiny_ldm", False, False), ("xattn", True, False), ("ldm77", True, False),
         ("wide", True, False), ("heads16", True, False), ("tiny_ldm", True, True), ("xattn", True, True)]


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name,use_et,generic", CASES)
def test_context_grad_vs_float64_autograd(name, use_et, generic, prec, monkeypatch):
    if generic:
        monkeypatch.setenv("LOCO_FUSE_XATTN", "0")
    r = cgo.reference(name, use_et=use_et)
    eng = _engine(r, prec)
    _primal(eng, r, use_et)
    A, G = eng.pmp_vjp(r["U"].to(DEV), context_grad=True)
    cfg = r["cfg"]
    assert tuple(G.shape) == (3, cfg.context_len, cfg.context_dim) and bool(torch.isfinite(G).all())
    eG, eA, yard = rel(G, r["G64"]), rel(A, r["A64"]), r["yardstick"]
    print(f"[{name} use_et={use_et} generic={generic} {prec}] G rel-L2 {eG:.3e}  fp32 host yardstick {yard:.3e}  A rel-L2 {eA:.3e}")
    bar = 4 * yard if prec == "f32" else 4 * max(yard, eA)
    assert eG <= bar


@pytest.mark.parametrize("streams", ["1", "2"])
@pytest.mark.parametrize("generic", [False, True])
def test_rows_do_not_depend_on_the_batch(generic, streams, monkeypatch):
    """Row p of G has the same bits for k = 1, at every position of k = 4 (= max_batch; with LOCO_STREAMS=2 the batched pass
    that writes A is cut into two lanes) and from call to call."""
    if generic:
        monkeypatch.setenv("LOCO_FUSE_XATTN", "0")
    monkeypatch.setenv("LOCO_STREAMS", streams)
    r = cgo.reference("tiny_ldm")
    eng = _engine(r, "bf16x3")
    _primal(eng, r)
    g = torch.Generator().manual_seed(5)
    U = torch.randn(4, r["cfg"].n, generator=g).to(DEV)
    A4, G4 = eng.pmp_vjp(U, context_grad=True)
    _, G4b = eng.pmp_vjp(U, context_grad=True)
    assert torch.equal(G4, G4b)
    # (not asserted: the batched pass plans its convolutions by k, so the rows of A need not keep their bits -- which is why the
    # rows of G come from single-probe passes)
    same = [bool(torch.equal(eng.pmp_vjp(U[p:p + 1].contiguous())[0], A4[p])) for p in range(4)]
    print(f"A rows with the same bits at k = 1 and k = 4 (generic={generic}, streams={streams}): {same}")
    for p in range(4):
        _, G1 = eng.pmp_vjp(U[p:p + 1].contiguous(), context_grad=True)
        assert torch.equal(G1[0], G4[p]), p
    for shift in (1, 2, 3):
        _, Gs = eng.pmp_vjp(torch.roll(U, shift, 0).contiguous(), context_grad=True)
        assert torch.equal(torch.roll(Gs, -shift, 0), G4), shift
    _, G6 = eng.pmp_vjp(torch.cat([U, U[:2]]).contiguous(), context_grad=True)      # k > max_batch: two passes
    assert torch.equal(G6[:4], G4) and torch.equal(G6[4:], G4[:2])


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", ["tiny_ldm", "xattn", "heads16"])
def test_the_rows_of_A_are_unchanged(name, prec):
    """A of the call with the flag is A of the call without it, to the bit; without A (the C entry point takes NULL) G keeps
    its bits."""
    from loco_edit_amd.hip import _ptr, _stream
    r = cgo.reference(name)
    eng = _engine(r, prec)
    _primal(eng, r)
    U = r["U"].to(DEV)
    A0 = eng.pmp_vjp(U)
    A1, G1 = eng.pmp_vjp(U, context_grad=True)
    assert torch.equal(A0, A1)
    assert torch.equal(eng.pmp_vjp(U), A0)
    G2 = torch.empty_like(G1)
    rc = eng.lib.loco_pmp_vjp_context(eng._ctx, _ptr(U), 3, None, _ptr(G2), _stream())
    assert rc == 0 and torch.equal(G2, G1)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name", ["tiny_ldm", "xattn", "heads16"])
def test_one_probe_shares_its_pass_with_the_gradient_and_keeps_A(name, generic, prec, monkeypatch):
    """k = 1, the optimiser's case, is the one path where A and G come out of the SAME cotangent pass: the stage's gradient
    work (workspace in the split-K scratch; on the strided-GEMM route behind the fused row kernel also the pass's score buffer)
    runs between the ops that produce A.  A must be what the call without the flag writes, to the bit -- before and after --
    and G what a call without A writes.  That A is also held to float64: in the f32 mode within 4 x the fp32 host restatement's
    own error; in the split-bf16 mode within tests/test_gpu_latent.py's bar for U^T J of these networks (5 x 2e-4), the bar the
    project already holds this unchanged code to."""
    from loco_edit_amd.hip import _ptr, _stream
    if generic:
        monkeypatch.setenv("LOCO_FUSE_XATTN", "0")
    r = cgo.reference(name)
    eng = _engine(r, prec)
    _primal(eng, r)
    U1 = r["U"][:1].to(DEV).contiguous()
    A0 = eng.pmp_vjp(U1)
    A1, G1 = eng.pmp_vjp(U1, context_grad=True)
    assert torch.equal(A1, A0) and torch.equal(eng.pmp_vjp(U1), A0)
    A2, G2 = eng.pmp_vjp(U1, context_grad=True)
    assert torch.equal(A2, A0) and torch.equal(G2, G1)
    G3 = torch.empty_like(G1)
    assert eng.lib.loco_pmp_vjp_context(eng._ctx, _ptr(U1), 1, None, _ptr(G3), _stream()) == 0 and torch.equal(G3, G1)
    eA, yard = rel(A1, r["A64"][:1]), r["yardstick_A1"]
    print(f"[{name} generic={generic} {prec}] k = 1 A of the flagged call: rel-L2 {eA:.3e}  fp32 host yardstick {yard:.3e}")
    assert eA <= (4 * yard if prec == "f32" else 5 * 2e-4)


def test_a_fork_differentiates_its_own_context():
    r = cgo.reference("tiny_ldm")
    r2 = cgo.reference("tiny_ldm", ctx_scale=0.5)          # same seed: the same z, U and mask, the states halved
    assert torch.equal(r["U"], r2["U"]) and torch.equal(r["z"], r2["z"]) and rel(r2["G64"], r["G64"]) > 1e-2
    eng = _engine(r)
    child = eng.fork()
    child.set_context(r2["ctx"].to(DEV).contiguous())
    _primal(eng, r); _primal(child, r2)
    _, Gc = child.pmp_vjp(r2["U"].to(DEV), context_grad=True)
    _, Gp = eng.pmp_vjp(r["U"].to(DEV), context_grad=True)
    print(f"fork: child {rel(Gc, r2['G64']):.3e} (yardstick {r2['yardstick']:.3e}), parent {rel(Gp, r['G64']):.3e} ({r['yardstick']:.3e})")
    assert rel(Gc, r2["G64"]) <= 4 * r2["yardstick"] and rel(Gp, r["G64"]) <= 4 * r["yardstick"]
    fresh = _engine(r2)                                     # an independent engine on the child's context: the same bits
    _primal(fresh, r2)
    assert torch.equal(fresh.pmp_vjp(r2["U"].to(DEV), context_grad=True)[1], Gc)


def test_refusals_leave_the_context_usable():
    from loco_edit_amd.hip import LocoEngine, _ptr, _stream
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(2)
    # no cross-attention stages at all
    eng = LocoEngine(TINY_DDPM, max_batch=2, device=dev)
    eng.load_state_dict(synth_params(TINY_DDPM, 0))
    x = torch.randn(1, 3, 32, 32, generator=g).to(DEV)
    eng.pmp_primal(x, 400.0, 0.5, None, use_et=True)
    U = torch.randn(2, TINY_DDPM.n, generator=g).to(DEV)
    A0 = eng.pmp_vjp(U)
    with pytest.raises(RuntimeError, match="context_dim"):
        eng.pmp_vjp(U, context_grad=True)
    assert torch.equal(eng.pmp_vjp(U), A0)
    # the DeepFloyd-IF blocks (added_kv)
    eng = LocoEngine(TINY_IF, max_batch=2, device=dev)
    eng.load_state_dict(synth_params(TINY_IF, 0))
    eng.set_context(torch.randn(TINY_IF.context_len, TINY_IF.context_dim, generator=g).to(DEV))
    x = torch.randn(1, 3, 32, 32, generator=g).to(DEV)
    eng.pmp_primal(x, 400.0, 0.5, None, use_et=True)
    U = torch.randn(2, eng.n_out, generator=g).to(DEV)
    A0 = eng.pmp_vjp(U)
    with pytest.raises(RuntimeError, match="added_kv"):
        eng.pmp_vjp(U, context_grad=True)
    assert torch.equal(eng.pmp_vjp(U), A0)
    # a stale primal, a tap's primal, no G
    r = cgo.reference("tiny_ldm")
    eng = _engine(r)
    U = r["U"].to(DEV)
    with pytest.raises(RuntimeError, match="primal"):
        eng.pmp_vjp(U, context_grad=True)                  # none yet
    _primal(eng, r)
    _, G0 = eng.pmp_vjp(U, context_grad=True)
    eng.set_context(r["ctx"].to(DEV).contiguous())
    with pytest.raises(RuntimeError, match="primal"):
        eng.pmp_vjp(U, context_grad=True)                  # set_context invalidated it
    eng.pmp_primal(r["z"].to(DEV), T_REF, AT_REF, None, use_et=True, tap="dec")
    with pytest.raises(RuntimeError, match="tap"):
        eng.pmp_vjp(U, context_grad=True)
    _primal(eng, r)
    assert eng.lib.loco_pmp_vjp_context(eng._ctx, _ptr(U), 3, None, None, _stream()) == -2
    assert b"G is NULL" in eng.lib.loco_last_error(eng._ctx)
    assert torch.equal(eng.pmp_vjp(U, context_grad=True)[1], G0)
