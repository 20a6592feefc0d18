"""Block Krylov solver, host side (no GPU): the float64 restatement of tests/krylov_ref.py against the float64 SVD of J,
the solver switch (``solver=`` / ``LOCO_SOLVER`` / ``--solver``, default ``power``), the refusal above 32 probes, and the
probe-sharded solve under gloo against the single-process solve."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_ref as kr      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTH, COS, S_RTOL = 2e-5, 0.9999, 1e-3       # the project's solver bounds (tests/test_gpu_solver_algebra.py)


def _svd(J):
    _, s64, vt64 = torch.linalg.svd(J.double(), full_matrices=False)
    return s64, vt64


def _orth_err(V):
    return (V @ V.T - torch.eye(V.shape[0], dtype=V.dtype)).abs().max().item()


@pytest.mark.parametrize("which", ["harmonic", "log"])
def test_restatement_converges_as_stated(which):
    """6 steps: span within the bounds; 8 steps: every row.  Power iteration at 12 iterations stays below 0.999 on the
    first operator (0.9966): the case shows what the solver is for."""
    J, V0 = kr.operator(which), kr.start_block(3071, 5)
    s64, vt64 = _svd(J)
    U, s, V, n, resid, _ = kr.krylov_reference(J, V0, 6)
    cos = kr.principal_cos(V, vt64[:5])
    s_rel = ((s.sqrt() - s64[:5]).abs() / s64[:5]).max().item()
    print(f"{which} 6 steps: span cos {cos:.8f} s_rel {s_rel:.2e} orth {_orth_err(V):.2e} max resid {resid.max():.2e}")
    assert n == 6 and cos >= COS and s_rel <= S_RTOL and _orth_err(V) < ORTH
    assert ((U - V @ J.double().T).norm() / U.norm()).item() <= 1e-5
    U, s, V, n, resid, _ = kr.krylov_reference(J, V0, 8)
    rows = (V * vt64[:5]).sum(dim=1).abs().min().item()
    print(f"{which} 8 steps ({n} run): per-row cos {rows:.8f}")
    assert rows >= COS
    if which == "harmonic":
        P = V0.double()
        for _ in range(12):
            P = torch.linalg.svd((P @ J.double().T) @ J.double(), full_matrices=False)[2]
        power = kr.principal_cos(P, vt64[:5])
        print(f"power iteration, 12 iterations: span cos {power:.4f}")
        assert power < 0.999


def test_restatement_residual_is_the_true_residual():
    """The free estimate sqrt(w^T G w) / theta_0 against ||J^T J y - theta y|| / theta_0 computed from the dense J."""
    J, V0 = kr.operator("harmonic"), kr.start_block(3071, 5)
    hist = []
    kr.krylov_reference(J, V0, 8, thr=0.0, history=hist)
    M = J.double().T @ J.double()
    worst = 0.0
    for h in hist:
        Y = h["Y"]
        theta = ((Y @ M) * Y).sum(dim=1)
        true = (Y @ M - theta[:, None] * Y).norm(dim=1) / h["theta"][0]
        big = true >= 1e-4
        if big.any():
            worst = max(worst, ((h["resid"][big] - true[big]).abs() / true[big]).max().item())
    print(f"residual estimate vs dense residual, worst relative difference {worst:.2e}")
    assert len(hist) == 8 and worst <= 1e-2


def test_restatement_ends_on_an_invariant_space():
    J, V0 = kr.operator("rank8"), kr.start_block(3071, 5)
    s64, vt64 = _svd(J)
    U, s, V, n, resid, reason = kr.krylov_reference(J, V0, 12)
    cos = kr.principal_cos(V, vt64[:5])
    print(f"rank 8: ended after {n} steps ({reason}), span cos {cos:.8f}")
    assert reason == "invariant" and n <= 6
    assert cos >= COS and ((s.sqrt() - s64[:5]).abs() / s64[:5]).max().item() <= S_RTOL
    norms = V.norm(dim=1)
    assert bool(((norms - 1).abs() <= ORTH).logical_or(norms == 0).all())


def test_restatement_undetermined_rows():
    """Rank 3 under 5 probes: three determined rows (s_i >= 1e-3 s_0); the others are no longer than a unit vector and
    orthogonal to the determined ones."""
    J, V0 = kr.operator("rank3"), kr.start_block(3071, 5)
    s64, vt64 = _svd(J)
    U, s, V, n, resid, reason = kr.krylov_reference(J, V0, 12)
    det = s >= 1e-3 * s[0]
    assert reason == "invariant" and n <= 6 and int(det.sum()) == 3
    assert (V[det] * vt64[:3]).sum(dim=1).abs().min().item() >= COS and _orth_err(V[det]) < ORTH
    assert ((s[det].sqrt() - s64[:3]).abs() / s64[:3]).max().item() <= S_RTOL
    assert V[~det].norm(dim=1).max().item() <= 1 + ORTH and (V[~det] @ V[det].T).abs().max().item() <= ORTH


# ---- the switch ---------------------------------------------------------------------------------------------------
class _DenseOp:
    def __init__(self, J):
        self.J, self.n_out = J, J.shape[0]

    def jvp(self, V):
        return V @ self.J.T

    def vjp(self, U):
        return U @ self.J

    def gather(self, U):
        return U


class _PowerAlgebra:
    def orthonormalize_(self, A):
        _, s, vh = torch.linalg.svd(A, full_matrices=False)
        A.copy_(vh)
        return s

    def convergence_rows(self, a, b, atol):
        return torch.tensor([0.0, 0.0])


class _BothAlgebra(kr.RefAlgebra, _PowerAlgebra):
    pass


def test_dispatcher_and_flag(monkeypatch):
    from loco_edit_amd import define_argparser, solver
    monkeypatch.delenv("LOCO_SOLVER", raising=False)
    assert solver.default_solver() == "power"
    J = kr.operator("log").double()
    V0 = kr.start_block(3071, 5).double()
    op, alg = _DenseOp(J), _BothAlgebra()
    ref = solver.subspace_iteration(op, alg, V0.clone(), 10, 3, 1e-3, verbose=False)
    info = {}
    got = solver.solve_basis(op, alg, V0.clone(), 10, 3, 1e-3, verbose=False, info=info)
    assert info == {"solver": "power"} and got[3] == 3
    assert all(torch.equal(a, b) for a, b in zip(ref[:3], got[:3]))          # default: the power loop, called as before
    info = {}
    U, s, V, n = solver.solve_basis(op, alg, V0.clone(), 10, 6, 1e-3, verbose=False, solver="krylov", info=info)
    Ur, sr, Vr, nr, rr, reason = kr.krylov_reference(J, V0, 6, store=torch.float64)
    assert n == nr and info["solver"] == "krylov" and info["reason"] == reason and info["rows"] == 30
    assert torch.allclose(V, Vr, atol=1e-12) and torch.allclose(U, Ur, atol=1e-12) and torch.allclose(s, sr, rtol=1e-12)
    assert torch.allclose(torch.tensor(info["residual"], dtype=torch.float64), rr, atol=1e-12)
    monkeypatch.setenv("LOCO_SOLVER", "krylov")
    assert solver.default_solver() == "krylov"
    assert solver.solve_basis(op, alg, V0.clone(), 10, 4, 1e-3, verbose=False)[3] == 4
    monkeypatch.setenv("LOCO_SOLVER", "lanczos")
    with pytest.raises(ValueError):
        solver.default_solver()
    with pytest.raises(ValueError):
        solver.solve_basis(op, alg, V0.clone(), solver="lanczos", verbose=False)
    # the command line: no flag leaves the environment alone, --solver sets the same switch
    monkeypatch.delenv("LOCO_SOLVER", raising=False)
    assert define_argparser.parse_args([]).solver is None and "LOCO_SOLVER" not in os.environ
    assert solver.default_solver() == "power"
    assert define_argparser.parse_args(["--solver", "krylov"]).solver == "krylov"
    assert os.environ["LOCO_SOLVER"] == "krylov" and solver.default_solver() == "krylov"
    monkeypatch.delenv("LOCO_SOLVER", raising=False)
    with pytest.raises(SystemExit):
        define_argparser.parse_args(["--solver", "lanczos"])


def test_more_than_32_probes_are_refused():
    from loco_edit_amd import solver
    J = torch.randn(40, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    V0 = torch.linalg.qr(torch.randn(64, 33, generator=torch.Generator().manual_seed(2), dtype=torch.float64))[0].T.contiguous()
    with pytest.raises(ValueError, match="32"):
        solver.krylov_iteration(_DenseOp(J), kr.RefAlgebra(), V0, max_iter=2, verbose=False)
    with pytest.raises(ValueError, match="32"):
        kr.krylov_reference(J, V0, 2)
    U, s, V, n = solver.krylov_iteration(_DenseOp(J), kr.RefAlgebra(), V0[:32].contiguous(), max_iter=4, verbose=False)
    assert n == 2 and V.shape == (32, 64)          # two blocks fill the 64 rows


def test_residual_file(tmp_path):
    import json
    from loco_edit_amd import solver
    base = str(tmp_path / "vT-modify.pt")
    assert solver.write_residuals(base, {"solver": "power"}) is None and solver.write_residuals(base, None) is None
    path = solver.write_residuals(base, {"solver": "krylov", "residual": [1e-5, 2e-5], "reason": "converged", "rows": 20})
    assert path == str(tmp_path / "vT-modify_residual.json")
    assert json.load(open(path)) == {"solver": "krylov", "residual": [1e-5, 2e-5], "reason": "converged", "rows": 20}


# ---- sharded solve under gloo -------------------------------------------------------------------------------------
def _run(rank, world, port, k, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import krylov_ref
    import loco_edit_amd  # noqa: F401
    from loco_edit_amd.dist import ProbeSharder
    from loco_edit_amd.solver import krylov_iteration
    if world > 1:                     # (the single-process leg runs inside pytest: leave its thread count alone)
        torch.set_num_threads(1)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(3)
    J = torch.randn(112, 48, generator=g, dtype=torch.float64) / 48 ** 0.5     # rectangular: rows of J V wider than the probes
    V0 = torch.linalg.qr(torch.randn(48, k, generator=g, dtype=torch.float64))[0].T.contiguous()
    info = {}
    U, s, V, n = krylov_iteration(_DenseOp(J), krylov_ref.RefAlgebra(), V0, max_iter=4, convergence_threshold=1e-9,
                                  sharder=ProbeSharder("world"), verbose=False, info=info)
    if rank == 0:
        q.put((U.tolist(), s.tolist(), V.tolist(), n, info["residual"]))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("k,port", [(5, 29591), (1, 29593)], ids=["5-probes-uneven-shards", "more-ranks-than-probes"])
def test_sharded_equals_single(k, port):
    ctx = mp.get_context("spawn")
    q1 = ctx.Queue()
    _run(0, 1, 0, k, q1)
    one = q1.get()
    q2 = ctx.Queue()
    procs = [ctx.Process(target=_run, args=(r, 2, port, k, q2)) for r in range(2)]
    for p in procs:
        p.start()
    two = q2.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert one[3] == two[3] == 4
    for a, b in zip(one[:3] + one[4:], two[:3] + two[4:]):
        a, b = torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)
        assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-12
    assert torch.tensor(two[0]).shape == (k, 112)
