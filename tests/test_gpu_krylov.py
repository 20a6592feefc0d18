"""Block Krylov solver on the device (csrc/solver.hip: loco_krylov_extend / _ritz / _left, solver.krylov_iteration)
against the float64 SVD of the fp32-rounded J or the float64 restatement of tests/krylov_ref.py.

Bounds are the project's solver bounds (tests/test_gpu_solver_algebra.py): max |V V^T - I| < 2e-5, |cos| >= 0.9999,
s to rtol 1e-3.  A convergence threshold of -1 switches the aligned stop test off (no element passes it), so that a case
runs the number of steps it states.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_ref as kr      # noqa: E402
import loco_oracle as orc    # noqa: E402
from loco_edit_amd.config import TINY_DDPM, UNetConfig, synth_params      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE = UNetConfig(resolution=128, ch=32, ch_mult=(1, 1, 2, 2), num_res_blocks=1, attn_resolutions=(16,))   # n = 49152
ORTH, COS, S_RTOL = 2e-5, 0.9999, 1e-3
N = 3071             # partial Gram blocks (256 columns) and sign segments (4096) throughout
NO_STOP = -1.0


@pytest.fixture(scope="module")
def engines():
    from loco_edit_amd.hip import LocoEngine, library_path
    assert os.path.exists(library_path())
    cache = {}

    def get(n):
        cfg = TINY_DDPM if n <= TINY_DDPM.n else WIDE
        assert n <= cfg.n
        if cfg not in cache:
            e = LocoEngine(cfg, max_batch=8 if cfg is TINY_DDPM else 1, device=torch.device(DEV))
            e.load_state_dict(synth_params(cfg, 0))
            cache[cfg] = e
        return cache[cfg]
    return get


class DenseOp:
    """jvp = V J^T, vjp = U J for a dense J [n_out, n]."""

    def __init__(self, J):
        self.J, self.n_out = J, J.shape[0]

    def jvp(self, V):
        return V @ self.J.T

    def vjp(self, U):
        return U @ self.J

    def gather(self, U):
        return U


@functools.lru_cache(maxsize=None)
def _case(which, n=N):
    """-> (J fp32, s64, vt64): the operator and the float64 SVD of the rounded matrix (computed once, never modified)."""
    if which == "harmonic" and n != N:
        J = kr.with_spectrum(1.0 / (1.0 + 0.1 * torch.arange(96, dtype=torch.float64)), n, 3)
    else:
        J = kr.operator(which, n=n)
    _, s64, vt64 = torch.linalg.svd(J.double(), full_matrices=False)
    return J, s64, vt64


def _orth_err(V):
    return (V @ V.T - torch.eye(V.shape[0], dtype=V.dtype)).abs().max().item()


def _solve(eng, J, V0, steps, thr=NO_STOP):
    from loco_edit_amd import solver
    info = {}
    U, s, V, n = solver.krylov_iteration(DenseOp(J.to(DEV)), eng, V0.to(DEV).clone(), max_iter=steps, convergence_threshold=thr,
                                         verbose=False, info=info)
    return U.cpu().double(), s.cpu().double(), V.cpu().double(), n, info


def _top_k_bounds(tag, s, V, s64, vt64, k, rows=False):
    cos = kr.principal_cos(V, vt64[:k])
    row_cos = (V * vt64[:k]).sum(dim=1).abs().min().item()
    s_rel = ((s.sqrt() - s64[:k]).abs() / s64[:k]).max().item()
    orth = _orth_err(V)
    print(f"{tag}: span cos {cos:.8f} row cos {row_cos:.8f} s_rel {s_rel:.2e} orth {orth:.2e}")
    assert torch.isfinite(V).all() and torch.isfinite(s).all()
    assert cos >= COS and s_rel <= S_RTOL and orth < ORTH, tag
    if rows:
        assert row_cos >= COS, tag


# ---------------------------------------------------------------------------------------------------------------------
# 1. convergence
@pytest.mark.parametrize("which", ["harmonic", "log"])
def test_convergence_in_six_and_eight_steps(which, engines):
    from loco_edit_amd import solver
    J, s64, vt64 = _case(which)
    eng, V0 = engines(N), kr.start_block(N, 5)
    U, s, V, n, info = _solve(eng, J, V0, 6)
    assert n == 6 and info["rows"] == 30
    _top_k_bounds(f"krylov {which} 6 steps", s, V, s64, vt64, 5)
    U, s, V, n, info = _solve(eng, J, V0, 8)
    assert n == 8
    _top_k_bounds(f"krylov {which} 8 steps", s, V, s64, vt64, 5, rows=True)
    if which == "harmonic":      # what the solver is for: the power loop at twice the passes is not there yet (0.9966 in float64)
        _, _, Vp, n_it = solver.subspace_iteration(DenseOp(J.to(DEV)), eng, V0.to(DEV).clone(), min_iter=12, max_iter=12,
                                                   verbose=False)
        power = kr.principal_cos(Vp.cpu(), vt64[:5])
        print(f"power iteration, 12 iterations: span cos {power:.6f}")
        assert n_it == 12 and power < 0.999


# ---------------------------------------------------------------------------------------------------------------------
# 2. the residual estimate is the residual; U = J V
def _residual_identity(tag, eng, J, V0, steps):
    """Drive the per-solve state step by step; at every step compare the estimate with ||J^T J y - theta y|| / theta_0 from
    the dense J in float64 wherever the latter is >= 1e-4.  -> the state after the last step."""
    from loco_edit_amd import solver
    from loco_edit_amd.dist import ProbeSharder
    Jd = J.to(DEV)
    M = J.double().T @ J.double()
    k = V0.shape[0]
    st = solver.KrylovState(eng, V0.to(DEV).clone(), J.shape[0], (0, k))
    worst, compared = 0.0, 0
    for j in range(steps):
        blk = st.block()
        U = blk @ Jd.T
        done = st.advance(U, U @ Jd, NO_STOP, last=(j == steps - 1))
        Y = st.Y[(st.steps - 1) % 2].cpu().double()
        MY = Y @ M
        theta = (MY * Y).sum(dim=1) / (Y * Y).sum(dim=1).clamp_min(1e-300)
        true = (MY - theta[:, None] * Y).norm(dim=1) / theta.max()
        est = st.resid.cpu().double()
        big = true >= 1e-4
        if big.any():
            compared += int(big.sum())
            worst = max(worst, ((est[big] - true[big]).abs() / true[big]).max().item())
        assert _orth_err(Y) < ORTH, f"{tag} step {j}"
        if done:
            break
    print(f"{tag}: {st.steps} steps, {compared} residuals >= 1e-4 compared, worst relative difference {worst:.2e}")
    assert compared > 0 and worst <= 1e-2, tag
    Uf, s, V, _ = st.finish(ProbeSharder(None))
    Uf, s, V = Uf.cpu().double(), s.cpu().double(), V.cpu().double()
    u_rel = ((Uf - V @ J.double().T).norm() / Uf.norm()).item()
    s_rel = ((s - (V @ J.double().T).pow(2).sum(dim=1)).abs() / s).max().item()
    print(f"{tag}: |U - J V| / |U| {u_rel:.2e}  s against ||J v||^2 {s_rel:.2e}")
    assert u_rel <= 1e-5 and s_rel <= 2e-5, tag      # s is quadratic in U: twice its bound
    return st


def test_residual_estimate_and_left_rows(engines):
    J, _, _ = _case("harmonic")
    st = _residual_identity("residual k=5", engines(N), J, kr.start_block(N, 5), 8)
    assert st.steps == 8


# ---------------------------------------------------------------------------------------------------------------------
# 3. an invariant Krylov space ends the solve
def test_invariance_exit_on_exact_rank(engines):
    J, s64, vt64 = _case("rank8")
    U, s, V, n, info = _solve(engines(N), J, kr.start_block(N, 5), 12, thr=1e-3)
    print(f"rank 8: ended after {n} steps ({info['reason']}), residuals {info['residual']}")
    assert n <= 6 and info["reason"] == "invariant"
    _top_k_bounds("krylov rank 8", s, V, s64, vt64, 5, rows=True)
    norms = V.norm(dim=1)
    assert bool(((norms - 1).abs() <= ORTH).logical_or(norms == 0).all())


def test_undetermined_rows_on_rank_three(engines):
    """More probes than directions: rows with s_i >= 1e-3 s_0 are determined, the others are no longer than a unit vector
    and orthogonal to the determined ones (the contract of loco_orthonormalize's undetermined rows)."""
    J, s64, vt64 = _case("rank3")
    U, s, V, n, info = _solve(engines(N), J, kr.start_block(N, 5), 12, thr=1e-3)
    det = s >= 1e-3 * s[0]
    cos = (V[det] * vt64[:3]).sum(dim=1).abs().min().item()
    norm, cross = V[~det].norm(dim=1).max().item(), (V[~det] @ V[det].T).abs().max().item()
    print(f"rank 3: {n} steps ({info['reason']}), determined {int(det.sum())}, row cos {cos:.8f}, other rows: norm {norm:.7f} "
          f"|<row, determined>| {cross:.2e}")
    assert info["reason"] == "invariant" and n <= 6 and int(det.sum()) == 3
    assert cos >= COS and _orth_err(V[det]) < ORTH and ((s[det].sqrt() - s64[:3]).abs() / s64[:3]).max().item() <= S_RTOL
    assert norm <= 1 + ORTH and cross <= ORTH and torch.isfinite(V).all() and torch.isfinite(U).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. limits
def test_sixteen_probes_fill_the_64_rows(engines):
    J, _, _ = _case("harmonic")
    st = _residual_identity("residual k=16", engines(N), J, kr.start_block(N, 16), 10)
    assert st.steps == 4 and st.m_ritz == 64 and st.reason == "full"


def test_one_probe(engines):
    J, s64, vt64 = _case("harmonic")
    eng, V0 = engines(N), kr.start_block(N, 1)
    U, s, V, n, info = _solve(eng, J, V0, 16)
    cos = (V * vt64[:1]).sum().abs().item()
    print(f"k = 1, 16 steps: |cos| {cos:.8f} residual {info['residual']}")
    assert n == 16 and cos >= COS and abs(V.norm().item() - 1) <= ORTH
    U, s, V, n, info = _solve(eng, J, V0, 100)
    cos = (V * vt64[:1]).sum().abs().item()
    print(f"k = 1, to 64 rows: {n} steps ({info['reason']}), |cos| {cos:.8f}")
    assert n == 64 and info["rows"] == 64 and info["reason"] == "full"
    assert cos >= COS and abs(V.norm().item() - 1) <= ORTH and abs(s.sqrt().item() - s64[0].item()) <= S_RTOL * s64[0].item()


def test_more_than_32_probes_raise(engines):
    from loco_edit_amd import solver
    J, _, _ = _case("harmonic")
    with pytest.raises(ValueError, match="32"):
        solver.krylov_iteration(DenseOp(J.to(DEV)), engines(N), kr.start_block(N, 33).to(DEV), max_iter=2, verbose=False)
    eng = engines(N)       # and the ABI itself refuses sizes it cannot hold, with an error string
    A, Q, stat = torch.zeros(33, N, device=DEV), torch.zeros(64, N, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match="k <= 32"):
        eng.krylov_extend(A, Q, 33, None, stat)
    with pytest.raises(RuntimeError, match="multiple of k"):
        eng.krylov_extend(A[:5], Q, 7, None, stat)
    with pytest.raises(RuntimeError, match="has not been called"):
        eng.krylov_ritz(Q, 60, torch.zeros(5, N, device=DEV), None, 1e-3, torch.zeros(5, device=DEV), stat, slot=1)


@functools.lru_cache(maxsize=None)
def _tall_case():
    """J 4000 x 3071 of rank 96 (rows of J V wider than the probes) and the float64 restatement's 6 steps on it."""
    g = torch.Generator().manual_seed(11)
    sigma = 1.0 / (1.0 + 0.1 * torch.arange(96, dtype=torch.float64))
    J = ((kr.orth_cols(4000, 96, g) * sigma) @ kr.orth_cols(N, 96, g).T).float().contiguous()
    V0 = kr.start_block(N, 5)
    return J, V0, kr.krylov_reference(J, V0, 6, thr=NO_STOP)


def test_left_rows_wider_than_the_probes(engines):
    J, V0, (Ur, sr, Vr, nr, rr, _) = _tall_case()
    U, s, V, n, info = _solve(engines(N), J, V0, 6)
    cos = kr.principal_cos(V, Vr)
    s_rel = ((s - sr).abs() / sr).max().item()
    u_rel = ((U - V @ J.double().T).norm() / U.norm()).item()
    print(f"n_out 4000: span cos against the restatement {cos:.8f} s_rel {s_rel:.2e} |U - J V| / |U| {u_rel:.2e}")
    assert n == nr == 6 and U.shape == (5, 4000)
    assert cos >= COS and s_rel <= S_RTOL and _orth_err(V) < ORTH and u_rel <= 1e-5


def test_wide_rows_loop_the_capped_grids(engines):
    n = WIDE.n
    J, s64, vt64 = _case("harmonic", n)
    U, s, V, steps, info = _solve(engines(n), J, kr.start_block(n, 5), 8)
    assert steps == 8
    _top_k_bounds(f"krylov n = {n}, 8 steps", s, V, s64, vt64, 5, rows=True)
    u_rel = ((U - V @ J.double().T).norm() / U.norm()).item()
    assert u_rel <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 5. on the engine's own Jacobian
def _tiny_problem(golden):
    g = golden("tiny")
    sch = orc.Scheduler()
    sch.set_timesteps(100)
    res = TINY_DDPM.resolution
    mask = torch.zeros(3, res, res, dtype=torch.bool)
    mask[:, 10:12, 14:16] = True                       # 2 x 2 pixels x 3 channels: L = 12
    v0 = torch.randn(TINY_DDPM.n, 5, generator=torch.Generator().manual_seed(21))
    v0b = torch.randn(TINY_DDPM.n, 5, generator=torch.Generator().manual_seed(22))
    return g["x"].to(DEV), float(g["t"]), float(sch.alpha_at(g["t"])), mask, v0.to(DEV), v0b.to(DEV)


def test_on_the_engine_jacobian(engines, golden):
    from loco_edit_amd import solver
    eng = engines(N)
    prec = eng.get_precision()
    eng.set_precision("f32")
    try:
        x, t, at, mask, v0, v0b = _tiny_problem(golden)
        n = TINY_DDPM.n
        # dense masked J [12, n] from the VJPs of the 12 unit cotangents
        eng.pmp_primal(x, t, at, mask.to(DEV))
        pos = mask.reshape(-1).nonzero()[:, 0]
        E = torch.zeros(12, n)
        E[torch.arange(12), pos] = 1.0
        J = eng.pmp_vjp(E.to(DEV)).cpu().double()
        _, s64, vt64 = torch.linalg.svd(J, full_matrices=False)
        info = {}
        u, s, vT, n_it = solver.local_basis(eng, x, t, at, 5, mask=mask.to(DEV), max_iter=50, convergence_threshold=1e-3, v0=v0,
                                            verbose=False, solver="krylov", info=info)
        V = vT.cpu().double()
        cos = kr.principal_cos(V, vt64[:5])
        s_rel = ((s.cpu().double() - s64[:5]).abs() / s64[:5]).max().item()
        print(f"engine J: {n_it} steps ({info['reason']}), span cos {cos:.8f} s_rel {s_rel:.2e} residuals {info['residual']} "
              f"sigma {s64[:6].tolist()}")
        assert n_it <= 6 and u.shape == (12, 5)
        assert cos >= COS and s_rel <= S_RTOL and _orth_err(V) < ORTH
        assert max(info["residual"]) <= 1e-4
        # the pair of solves in one batch per pass equals the two solves run alone (3 steps each)
        kw = dict(max_iter=3, convergence_threshold=NO_STOP, verbose=False, solver="krylov")
        alone_a = solver.local_basis(eng, x, t, at, 5, mask=mask.to(DEV), v0=v0, **kw)
        alone_b = solver.local_basis(eng, x, t, at, 5, mask=(~mask).to(DEV), v0=v0b, **kw)
        infos = []
        pair = solver.local_basis_pair(eng, x, t, at, 5, mask.to(DEV), 5, (~mask).to(DEV), v0_a=v0, v0_b=v0b, info=infos, **kw)
        for name, one, two in (("modify", alone_a, pair[0]), ("null", alone_b, pair[1])):
            cos = kr.principal_cos(one[2].cpu(), two[2].cpu())
            s_rel = ((one[1] - two[1]).abs() / one[1]).max().item()
            print(f"pair [{name}]: span cos {cos:.8f} s_rel {s_rel:.2e} steps {one[3]} / {two[3]}")
            assert one[3] == two[3] == 3 and one[0].shape == two[0].shape
            assert cos >= COS and s_rel <= S_RTOL
        assert len(infos) == 2 and all(len(i["residual"]) == 5 for i in infos)
    finally:
        eng.set_precision(prec)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the default path is the power loop, bit for bit
def test_default_path_is_unchanged(engines, golden, monkeypatch):
    from loco_edit_amd import solver
    monkeypatch.delenv("LOCO_SOLVER", raising=False)
    eng = engines(N)
    x, t, at, mask, v0, _ = _tiny_problem(golden)
    u, s, vT, n_it = solver.local_basis(eng, x, t, at, 5, mask=mask.to(DEV), min_iter=3, max_iter=3, v0=v0, verbose=False)
    V = v0.T.contiguous()
    eng.qr_rows_(V)
    op = solver.JacobianOperator(eng, x, t, at, mask.to(DEV), False)
    U2, s2, V2, n2 = solver.subspace_iteration(op, eng, V, 3, 3, 1e-3, sharder=None, verbose=False, stop_rule=None)
    assert n_it == n2 == 3
    assert torch.equal(u, op.gather(U2).T.contiguous()) and torch.equal(s, s2.sqrt()) and torch.equal(vT, V2)
