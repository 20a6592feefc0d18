"""PMP-Jacobian low-rank subspace solver: block power iteration on J^T J with
J = d x0_hat[mask] / d x_t (reference ``local_encoder_decoder_pullback_xt``,
``src/modules/edit.py:2406-2504``).

The reference pays (3k+1) denoiser passes per iteration (jacfwd recomputes the
primal k times, k sequential backward sweeps) plus three host round trips; here
the primal is evaluated once per solve, each iteration is one batched tangent
pass + one batched cotangent pass + an on-device Gram/eig re-orthonormalisation,
and at most one 2-float readback.

``LOCO_SOLVER=krylov`` / ``solver="krylov"`` selects the block Krylov solver (``krylov_iteration``) instead: the same
two passes per step, Rayleigh-Ritz over every stored block, a residual per returned direction.

Multi-GPU: probes are sharded over ranks (``ProbeSharder``), each
rank runs JVP+VJP on its rows, one all-gather of the A shards per iteration,
the k x k algebra is replicated.
"""
from __future__ import annotations

import os
import time
from typing import Optional, Tuple

import torch

from .dist import ProbeSharder


def default_stop_rule() -> str:
    """How the stop test of edit.py:2489-2492 is applied (``LOCO_STOP_RULE``, default ``reference``).

    The reference tests ``torch.allclose(v_prev, v, atol)`` on the right singular vectors LAPACK returns.  Measured on
    the reference itself (``oracle/make_golden.py --only converge`` -> ``tests/golden/converge.pt``): with ONE probe the
    sign LAPACK picks is stable and the loop stops when the vector has converged; with k >= 2 probes the left factor of
    the nearly diagonal k x k problem comes back as a reflection (first row ~ -e_0, others vary), so at least one row of
    ``v`` is the NEGATIVE of its predecessor in every iteration, the test never holds, and the reference runs ``max_iter``
    iterations (38 - 40 of 40 random near-diagonal problems for every k in 2..64 on the LAPACK build of this image; the
    test asserts >= 38 -- on a LAPACK that does not flip, the reference would stop early and this rule would not).

    ``reference``: what the reference does -- a single probe stops on the test (rows compared up to sign, which for one
    probe is the reference's own comparison); k >= 2 runs ``max_iter`` iterations, the test is still evaluated where the
    reference evaluates it (every iteration after ``min_iter``) and reported, but does not end the loop.
    ``aligned``: the test the reference intends -- every row allclose to +-its predecessor -- ends the loop for any k
    (fewer iterations than the reference on spectra that converge; same subspace).
    """
    rule = os.environ.get("LOCO_STOP_RULE", "reference")
    if rule not in ("reference", "aligned"):
        raise ValueError(f"LOCO_STOP_RULE must be 'reference' or 'aligned', got {rule!r}")
    return rule


def _converged(algebra, V_prev, V, thr):
    """[distance, flag] of the stop test, rows compared up to sign (``loco_convergence_rows``); test doubles that only
    provide the flat comparison (fixed signs) are used as they are."""
    fn = getattr(algebra, "convergence_rows", None) or algebra.convergence
    return fn(V_prev, V, thr).tolist()


class JacobianOperator:
    """J and J^T products on the HIP engine for a fixed (x, t, mask).

    ``tap``: None -- J = d x0_hat[mask] / d x_t; ``"enc"`` -- J = d h / d x_t (rows of J V have the bottleneck's width n_h, no
    mask); ``"dec"`` -- J = mask . c . d eps / d h with x_t and the skips fixed (rows of V and J^T U have the width n_h)."""

    def __init__(self, engine, x: torch.Tensor, t, at: float, mask: Optional[torch.Tensor], noise: bool = False,
                 tap: Optional[str] = None):
        self.engine = engine
        self.tap = tap
        self.n = engine.n_h if tap == "dec" else engine.n
        self.n_out = engine.n_h if tap == "enc" else engine.n_out      # width of the rows of J V (= n for the pixel-space denoisers)
        self.masked = mask is not None
        if tap is None:
            engine.pmp_primal(x.contiguous(), float(t), at, mask, use_et=noise)
        else:
            engine.pmp_primal(x.contiguous(), float(t), at, mask, use_et=noise, tap=tap)

    def check_mask(self):
        """The gather list is built on the device and its length L is read back lazily (no host sync at the start
        of a solve): the empty-mask error is raised when L is first needed, at the end of the solve."""
        if self.masked and self.engine.mask_count() == 0:
            # the reference would run the power iteration on a 0-row Jacobian and return NaN directions
            raise ValueError("empty mask: J = d x0_hat[mask] / d x_t has no rows")

    def jvp(self, V: torch.Tensor) -> torch.Tensor:   # [k,n] -> dense masked [k,n]
        return self.engine.pmp_jvp(V)

    def vjp(self, U: torch.Tensor) -> torch.Tensor:   # dense [k,n] -> [k,n]
        return self.engine.pmp_vjp(U)

    def gather(self, U: torch.Tensor) -> torch.Tensor:  # dense [k,n] -> [k,L]
        return self.engine.mask_gather(U)


def _n_out(op, V: torch.Tensor) -> int:
    """Row width of J V for the operator ``op`` (the decoded image for the latent operator, else the input width)."""
    return int(getattr(op, "n_out", V.shape[1]))


def subspace_iteration(op, algebra, V0: torch.Tensor, min_iter: int = 10, max_iter: int = 100,
                       convergence_threshold: float = 1e-3, sharder: Optional[ProbeSharder] = None,
                       verbose: bool = True, stop_rule: Optional[str] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """Core loop of edit.py:2443-2494 on orthonormal rows ``V0`` [k, n].

    ``op`` provides jvp/vjp/gather, ``algebra`` provides orthonormalize_/convergence
    (the HIP engine in production; tests substitute CPU doubles to exercise the
    sharding logic under gloo).  Returns (U_dense [k,n], s [k], V [k,n], n_iter)
    where U = J V_prev of the last iteration (edit.py:2457 -- the reference
    returns u one iteration behind vT) and s are the singular values of A.
    ``stop_rule``: see ``default_stop_rule``.
    """
    sharder = sharder or ProbeSharder(None)
    k = V0.shape[0]
    may_stop = (stop_rule or default_stop_rule()) == "aligned" or k == 1
    if verbose and not may_stop and max_iter > min_iter + 1:
        print(f'power method : {k} probes run all {max_iter} iterations under LOCO_STOP_RULE=reference (the reference\'s allclose '
              f'never holds for k >= 2); LOCO_STOP_RULE=aligned stops on the intended test')
    V = V0
    n_done = 0
    U = None
    s = None
    for i in range(max_iter):
        V_prev = V
        lo, hi = sharder.rows(k)
        if hi > lo:
            U_loc = op.jvp(V[lo:hi].contiguous())      # u_i = J v_i            (edit.py:2451-2455)
            A_loc = op.vjp(U_loc)                       # a_i = J^T u_i          (edit.py:2460-2480)
        else:                                           # more ranks than probes: this rank only joins the gathers
            A_loc = V[0:0].contiguous()                 # rows of J^T U have the input width ...
            U_loc = V.new_empty(0, _n_out(op, V))       # ... rows of J V the OUTPUT width (latent operator: n_out != n)
        A = sharder.all_gather_rows(A_loc, k)           # the one collective per iteration
        U = U_loc
        V = A
        s = algebra.orthonormalize_(V)                  # _, s, v = svd(v_)      (edit.py:2482)
        n_done = i + 1
        need_flag = i > min_iter
        if verbose or need_flag:
            dist_close = _converged(algebra, V_prev, V, convergence_threshold)   # edit.py:2489-2492
            if verbose:
                print(f'power method : {i}-th step convergence : ', dist_close[0])
            if need_flag and may_stop and dist_close[1] > 0.5:
                if verbose:
                    print('reach convergence threshold : ', dist_close[0])
                break
    U = sharder.all_gather_rows(U, k)
    return U, s, V, n_done


# ---------------------------------------------------------------------------------------------------------------------
# block Krylov solver (opt-in)
KRYLOV_ROWS = 64          # rows of Q the eigensolver takes
KRYLOV_MAX_PROBES = 32    # two blocks must fit


def default_solver() -> str:
    """``LOCO_SOLVER``: ``power`` (default; ``subspace_iteration``) or ``krylov`` (``krylov_iteration``)."""
    name = os.environ.get("LOCO_SOLVER", "power")
    if name not in ("power", "krylov"):
        raise ValueError(f"LOCO_SOLVER must be 'power' or 'krylov', got {name!r}")
    return name


def _pick_solver(solver: Optional[str]) -> str:
    name = solver or default_solver()
    if name not in ("power", "krylov"):
        raise ValueError(f"solver must be 'power' or 'krylov', got {name!r}")
    return name


class KrylovState:
    """What one block Krylov solve keeps between steps: ``Q`` [cap, n] (orthonormal rows, blocks of k, block 0 = V0),
    the rows ``J Q`` this rank computed, two buffers for the Ritz vectors of this step and the previous one, the
    residuals and the four floats read back per step.  Allocated once per solve; ``slot`` names the context's own
    small state (T, Ritz pairs, G), so that two solves can be in flight."""

    def __init__(self, algebra, V0: torch.Tensor, n_out: int, local_rows: Tuple[int, int], slot: int = 0):
        k, n = V0.shape
        if k > KRYLOV_MAX_PROBES:
            raise ValueError(f"the block Krylov solver keeps at least two blocks in {KRYLOV_ROWS} rows: {k} probes > "
                             f"{KRYLOV_MAX_PROBES}; use solver='power' for this probe count")
        self.algebra, self.k, self.n, self.n_out, self.slot = algebra, k, n, n_out, slot
        self.cap = (KRYLOV_ROWS // k) * k
        self.lo, self.hi = local_rows
        self.Q = V0.new_zeros(self.cap, n)
        self.Q[:k] = V0
        self.Uloc = V0.new_zeros(self.cap // k, self.hi - self.lo, n_out)      # block b: rows lo..hi of J Q_b
        self.Y = [V0.new_empty(k, n), V0.new_empty(k, n)]
        self.resid = V0.new_zeros(k)
        self.stat = V0.new_zeros(4)
        self.m = k              # rows of Q in use, the current block last
        self.steps = 0
        self.m_ritz = 0         # rows the last Ritz vectors were computed over
        self.reason = None      # why the solve ended: invariant | converged | full | max_iter
        self.dist = -1.0
        self.max_resid = float("nan")

    def block(self) -> torch.Tensor:
        return self.Q[self.m - self.k:self.m]

    def advance(self, U_loc: torch.Tensor, A: torch.Tensor, thr: float, last: bool) -> bool:
        """Take this step's J Q_j rows (this rank's) and A = J^T J Q_j (all rows; overwritten).  True: the solve ends."""
        k, m = self.k, self.m
        self.Uloc[m // k - 1].copy_(U_loc)
        room = m + k <= self.cap and not last
        nxt = self.Q[m:m + k] if room else None
        self.algebra.krylov_extend(A, self.Q, m, nxt, self.stat, self.slot)
        Y, Yprev = self.Y[self.steps % 2], (self.Y[(self.steps + 1) % 2] if self.steps >= 1 else None)
        self.algebra.krylov_ritz(self.Q, m, Y, Yprev, thr, self.resid, self.stat, self.slot)
        self.dist, flag, self.max_resid, all_zero = self.stat.tolist()         # the one readback of the step
        self.steps += 1
        self.m_ritz = m
        if room and all_zero > 0.5:
            self.reason = "invariant"
        elif Yprev is not None and flag > 0.5:
            self.reason = "converged"
        elif not room:
            self.reason = "max_iter" if last else "full"
        else:
            self.m = m + k
        return self.reason is not None

    def finish(self, sharder: ProbeSharder):
        """-> (U [k, n_out] = J V, s [k] = ||U_i||^2, V [k, n], resid [k])."""
        k, nb = self.k, self.m_ritz // self.k
        if sharder.active:      # the stored rows are gathered once, here: [rows, blocks * n_out] keeps all_gather_rows' layout
            loc = self.Uloc[:nb].permute(1, 0, 2).reshape(self.hi - self.lo, nb * self.n_out)
            Ustore = sharder.all_gather_rows(loc, k).view(k, nb, self.n_out).permute(1, 0, 2).reshape(nb * k, self.n_out)
            Ustore = Ustore.contiguous()
        else:
            Ustore = self.Uloc.view(self.cap, self.n_out)
        UY = self.Q.new_empty(k, self.n_out)
        s = self.Q.new_empty(k)
        self.algebra.krylov_left(Ustore, self.m_ritz, UY, s, self.slot)
        return UY, s, self.Y[(self.steps - 1) % 2], self.resid


def krylov_iteration(op, algebra, V0: torch.Tensor, max_iter: int = 100, convergence_threshold: float = 1e-3,
                     sharder: Optional[ProbeSharder] = None, verbose: bool = True, info: Optional[dict] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """Block Krylov counterpart of ``subspace_iteration`` on orthonormal rows ``V0`` [k, n], k <= 32 (DESIGN.md "Block
    Krylov solver").  Every step pays the same one batched J V and one batched J^T U; the blocks of all steps are kept
    (at most 64 rows) and the returned rows are the top-k Ritz vectors of J^T J over their span.  After j steps that span
    is V0, (J^T J) V0 ... (J^T J)^(j-1) V0: the newest block A_j enters T and the residual, and the basis one step later.

    ``algebra`` provides krylov_extend / krylov_ritz / krylov_left (the HIP engine; tests substitute a float64 double).
    Returns (U [k, n_out], s [k], V [k, n], n_steps) with ``subspace_iteration``'s conventions -- callers take
    ``s.sqrt()`` and ``op.gather(U)`` -- except that U = J V of the RETURNED V (the power loop returns it one iteration
    behind) and s_i = ||U_i||^2.  ``info`` (a dict) receives ``residual`` (list of k floats: ||J^T J v_i - theta_i v_i||
    / theta_0 as estimated from the last residual block), ``reason`` and ``rows``.

    The solve ends when the next block is entirely below 1e-6 of the largest Ritz value (the space is invariant: the
    result is exact), when every row is allclose(``convergence_threshold``) to +-its predecessor (tested from the second
    step on; a negative threshold switches this exit off), when another block would not fit in 64 rows, or after
    ``max_iter`` steps.  The reference's ``min_iter`` is not consulted: the drivers pass 10, which would forbid the early
    stop this solver exists for."""
    sharder = sharder or ProbeSharder(None)
    k = V0.shape[0]
    st = KrylovState(algebra, V0, _n_out(op, V0), sharder.rows(k))
    lo, hi = st.lo, st.hi
    for j in range(max_iter):
        blk = st.block()
        if hi > lo:
            U_loc = op.jvp(blk[lo:hi].contiguous())
            A_loc = op.vjp(U_loc)
        else:                                           # more ranks than probes: this rank only joins the gathers
            A_loc = blk[0:0].contiguous()
            U_loc = blk.new_empty(0, st.n_out)
        A = sharder.all_gather_rows(A_loc, k)           # the one collective per step
        done = st.advance(U_loc, A, convergence_threshold, last=(j == max_iter - 1))
        if verbose:
            print(f'block krylov : {j}-th step ({st.m_ritz} rows) convergence : {st.dist}  residual : {st.max_resid}')
        if done:
            break
    if verbose:
        print(f'block krylov : ended after {st.steps} steps ({st.reason})')
    U, s, V, resid = st.finish(sharder)
    if info is not None:
        info.update(residual=[float(r) for r in resid.tolist()], reason=st.reason, rows=st.m_ritz, solver="krylov")
    return U, s, V, st.steps


def solve_basis(op, algebra, V0: torch.Tensor, min_iter: int = 10, max_iter: int = 100, convergence_threshold: float = 1e-3,
                sharder: Optional[ProbeSharder] = None, verbose: bool = True, stop_rule: Optional[str] = None,
                solver: Optional[str] = None, info: Optional[dict] = None):
    """The solver picked by ``solver`` (default ``LOCO_SOLVER``, default ``power``) -> (U, s, V, n_iter).  ``power`` is
    ``subspace_iteration`` called exactly as before; ``krylov`` ignores ``min_iter`` and ``stop_rule`` and fills ``info``."""
    if _pick_solver(solver) == "krylov":
        return krylov_iteration(op, algebra, V0, max_iter, convergence_threshold, sharder=sharder, verbose=verbose, info=info)
    if info is not None:
        info.update(solver="power")
    return subspace_iteration(op, algebra, V0, min_iter, max_iter, convergence_threshold, sharder=sharder, verbose=verbose,
                              stop_rule=stop_rule)


def write_residuals(basis_path: str, info: Optional[dict]):
    """``<basis name>_residual.json`` next to a basis file, for a solve that produced residuals (the Krylov solver)."""
    if not info or "residual" not in info:
        return None
    import json
    path = os.path.splitext(basis_path)[0] + "_residual.json"
    with open(path, "w") as f:
        json.dump({k: info[k] for k in ("solver", "residual", "reason", "rows") if k in info}, f)
    return path


# local_basis targets -> the engine's tap
H_TARGETS = {"x0": None, "h_enc": "enc", "h_dec": "dec"}


def local_basis(engine, x, t, at, pca_rank: int, mask=None, noise=False, min_iter=10, max_iter=100,
                convergence_threshold=1e-3, v0: Optional[torch.Tensor] = None,
                sharder: Optional[ProbeSharder] = None, verbose=True, stop_rule: Optional[str] = None,
                solver: Optional[str] = None, info: Optional[dict] = None, target: str = "x0"):
    """Top-``pca_rank`` right singular subspace of J (edit.py:2406-2504).

    ``target``: ``"x0"`` -- J = d x0_hat[mask] / d x_t (``noise``: d eps instead); ``"h_enc"`` -- J = d h / d x_t, the
    reference's ``local_encoder_pullback_xt`` (models/ddpm/diffusion.py:484-556; no mask; ``u`` is [n_h, k]); ``"h_dec"`` --
    J = mask . d eps / d h with ``noise`` (``local_decoder_pullback_xt``, :558-632) or mask . d x0_hat / d h without
    (``local_x0_decoder_pullback_xt``, :634-707); ``vT`` is [k, n_h] and ``u`` [L, k] (n_out without a mask).  The h-space
    targets run the power iteration only: ``solver="krylov"`` is refused for them.

    ``v0``: optional [n, k] Gaussian matrix standing in for the ``torch.randn``
    draw of edit.py:2435 (parity tests inject it).  Returns (u [L,k], s [k],
    vT [k,n], n_iter) with the reference's conventions: ``s`` is the square
    root of the singular values of A = U^T J (edit.py:2500).  ``solver``: ``power`` | ``krylov`` (``solve_basis``);
    ``info`` receives the Krylov solver's residuals.
    """
    if target not in H_TARGETS:
        raise ValueError(f"target must be one of {sorted(H_TARGETS)}, got {target!r}")
    tap = H_TARGETS[target]
    if tap is not None and _pick_solver(solver) == "krylov":
        raise ValueError("the block Krylov solver is not wired to the h-space operators (its stores are sized for x_t -> x0); "
                         "use solver='power' for target 'h_enc' / 'h_dec'")
    if tap == "enc" and mask is not None:
        raise ValueError("target 'h_enc' takes no mask: h has no pixel positions to select")
    n = engine.n_h if tap == "dec" else engine.n
    dev = x.device
    time_s = time.time()
    if v0 is None:
        v0 = torch.randn(n, pca_rank, device=dev, dtype=torch.float32)      # edit.py:2435
    if tuple(v0.shape) != (n, pca_rank) and tap is not None:
        raise ValueError(f"v0 must be [{n}, {pca_rank}] for target {target!r}, got {tuple(v0.shape)}")
    V = v0.to(device=dev, dtype=torch.float32).T.contiguous()               # rows = probes
    engine.qr_rows_(V)                                                       # edit.py:2436 (thin QR)
    op = JacobianOperator(engine, x, t, at, mask, noise) if tap is None else JacobianOperator(engine, x, t, at, mask, noise, tap=tap)
    U, s, V, n_iter = solve_basis(op, engine, V, min_iter, max_iter, convergence_threshold, sharder=sharder,
                                  verbose=verbose, stop_rule=stop_rule, solver=solver, info=info)
    op.check_mask()
    u = op.gather(U).T.contiguous()                                          # [L, k]  (edit.py:2500-2502)
    if verbose:
        torch.cuda.synchronize()
        print('power method runtime ==' if _pick_solver(solver) == "power" else 'block krylov runtime ==', time.time() - time_s)
    return u, s.sqrt(), V, n_iter


def local_basis_pair(engine, x, t, at, rank_a: int, mask_a, rank_b: int, mask_b, noise=False, min_iter=10, max_iter=100,
                     convergence_threshold=1e-3, v0_a: Optional[torch.Tensor] = None, v0_b: Optional[torch.Tensor] = None,
                     sharder: Optional[ProbeSharder] = None, verbose=True, stop_rule: Optional[str] = None,
                     solver: Optional[str] = None, info: Optional[list] = None):
    """The two solves of ``run_edit_null_space_projection`` -- modify space on ``mask_a``, null space on ``mask_b`` (its
    complement), same ``x``, ``t`` (edit.py:2290-2310) -- with their probes in ONE batch per pass.

    The rows of J V and J^T U are independent, so each solve's iterates are exactly what ``local_basis`` computes for it
    alone (same V0 draws in the same order, own re-orthonormalisation, own convergence test and iteration count); what
    changes is that a pass carries rank_a + rank_b probes, which fills the deep levels of the network better (5 + 5
    probes: 14 % less time per probe than 5).  ``loco_pmp_set_second_mask`` tells the engine from which row of a call the
    second mask applies; once one solve has converged the other continues alone.  Returns
    ``((u_a, s_a, vT_a, n_iter_a), (u_b, s_b, vT_b, n_iter_b))`` with ``local_basis``'s conventions.

    ``solver``: ``power`` | ``krylov`` (default ``LOCO_SOLVER``).  With ``krylov`` each solve keeps its own basis, context
    slot and exits (``_krylov_pair``); ``info`` (a list) receives one dict per solve (``krylov_iteration``'s ``info``)."""
    sharder = sharder or ProbeSharder(None)
    if _pick_solver(solver) == "krylov":
        return _krylov_pair(engine, x, t, at, rank_a, mask_a, rank_b, mask_b, noise, max_iter, convergence_threshold,
                            v0_a, v0_b, sharder, verbose, info)
    n, dev = engine.n, x.device
    rule = stop_rule or default_stop_rule()
    may_stop = [rule == "aligned" or rank_a == 1, rule == "aligned" or rank_b == 1]
    time_s = time.time()
    if v0_a is None:
        v0_a = torch.randn(n, rank_a, device=dev, dtype=torch.float32)          # edit.py:2435, first solve
    if v0_b is None:
        v0_b = torch.randn(n, rank_b, device=dev, dtype=torch.float32)          # edit.py:2435, second solve
    V = [v0_a.to(device=dev, dtype=torch.float32).T.contiguous(), v0_b.to(device=dev, dtype=torch.float32).T.contiguous()]
    for v in V:
        engine.qr_rows_(v)
    op = JacobianOperator(engine, x, t, at, mask_a, noise)
    ranks = (rank_a, rank_b)
    m8_b = mask_b.to(device=dev, dtype=torch.uint8).contiguous().view(-1)
    mask_state = None
    active = [True, True]
    U_last = [None, None]
    s_last = [None, None]
    n_iter = [0, 0]
    for i in range(max_iter):
        if not any(active):
            break
        idx = [j for j in (0, 1) if active[j]]
        Vin = torch.cat([V[j] for j in idx]) if len(idx) == 2 else V[idx[0]]
        k = Vin.shape[0]
        lo, hi = sharder.rows(k)
        state = (tuple(idx), lo, hi)
        if state != mask_state:                                  # only when the set of running solves changes
            if len(idx) == 2:
                engine.pmp_set_second_mask(m8_b, min(max(rank_a - lo, 0), hi - lo))   # local row where the second mask starts
            elif idx[0] == 1:
                engine.pmp_set_second_mask(m8_b, 0)              # only the null-space solve is still running
            else:
                engine.pmp_set_second_mask(None)
            mask_state = state
        if hi > lo:
            U_loc = op.jvp(Vin[lo:hi].contiguous())
            A_loc = op.vjp(U_loc)
        else:
            A_loc = Vin[0:0].contiguous()
            U_loc = Vin.new_empty(0, _n_out(op, Vin))
        A = sharder.all_gather_rows(A_loc, k)
        off = 0
        for j in idx:
            Vj_prev = V[j]
            Vj = A[off:off + ranks[j]].contiguous()
            s_last[j] = engine.orthonormalize_(Vj)
            V[j] = Vj
            n_iter[j] = i + 1
            need_flag = i > min_iter
            conv = False
            if verbose or need_flag:
                dist_close = _converged(engine, Vj_prev, Vj, convergence_threshold)
                if verbose:
                    print(f'power method [{"modify" if j == 0 else "null"}] : {i}-th step convergence : ', dist_close[0])
                conv = need_flag and may_stop[j] and dist_close[1] > 0.5
            if conv or i == max_iter - 1:
                # this solve ends here: keep its U = J V_prev of this iteration (edit.py:2457 convention)
                U_all = sharder.all_gather_rows(U_loc, k)
                U_last[j] = U_all[off:off + ranks[j]].contiguous()
                active[j] = False
            off += ranks[j]
    engine.pmp_set_second_mask(None)
    out = []
    for j, m in ((0, mask_a), (1, mask_b)):
        mflat = m.to(dev).reshape(-1)
        if not bool(mflat.any()):
            raise ValueError("empty mask: J = d x0_hat[mask] / d x_t has no rows")
        u = U_last[j][:, mflat].T.contiguous()                                   # [L, k]
        out.append((u, s_last[j].sqrt(), V[j], n_iter[j]))
    if verbose:
        torch.cuda.synchronize()
        print('power method runtime (both solves) ==', time.time() - time_s)
    return out[0], out[1]


def _krylov_pair(engine, x, t, at, rank_a, mask_a, rank_b, mask_b, noise, max_iter, convergence_threshold, v0_a, v0_b,
                 sharder, verbose, info):
    """``local_basis_pair`` with the block Krylov solver: the current blocks of both solves share one batch per pass, each
    solve has its own ``KrylovState`` (context slot 0 and 1) and ends by its own exits; once one has ended the other
    continues alone.  With probes sharded over ranks the two solves run one after the other instead (each sharded as
    ``krylov_iteration`` shards it): a rank's rows of a joint batch are not a contiguous share of either solve."""
    n, dev = engine.n, x.device
    time_s = time.time()
    if v0_a is None:
        v0_a = torch.randn(n, rank_a, device=dev, dtype=torch.float32)          # edit.py:2435, first solve
    if v0_b is None:
        v0_b = torch.randn(n, rank_b, device=dev, dtype=torch.float32)          # edit.py:2435, second solve
    infos = [{}, {}]
    if sharder.active:
        out = [local_basis(engine, x, t, at, r, mask=m, noise=noise, max_iter=max_iter, convergence_threshold=convergence_threshold,
                           v0=v0, sharder=sharder, verbose=verbose, solver="krylov", info=infos[j])
               for j, (r, m, v0) in enumerate(((rank_a, mask_a, v0_a), (rank_b, mask_b, v0_b)))]
        if info is not None:
            info.extend(infos)
        return out[0], out[1]
    ranks = (rank_a, rank_b)
    states = []
    for j, v0 in enumerate((v0_a, v0_b)):
        V = v0.to(device=dev, dtype=torch.float32).T.contiguous()
        engine.qr_rows_(V)
        states.append(KrylovState(engine, V, engine.n_out, (0, ranks[j]), slot=j))
    op = JacobianOperator(engine, x, t, at, mask_a, noise)
    m8_b = mask_b.to(device=dev, dtype=torch.uint8).contiguous().view(-1)
    mask_state = None
    active = [True, True]
    names = ("modify", "null")
    for i in range(max_iter):
        idx = [j for j in (0, 1) if active[j]]
        if not idx:
            break
        Vin = torch.cat([states[j].block() for j in idx]) if len(idx) == 2 else states[idx[0]].block()
        if tuple(idx) != mask_state:                             # only when the set of running solves changes
            if len(idx) == 2:
                engine.pmp_set_second_mask(m8_b, rank_a)
            elif idx[0] == 1:
                engine.pmp_set_second_mask(m8_b, 0)              # only the null-space solve is still running
            else:
                engine.pmp_set_second_mask(None)
            mask_state = tuple(idx)
        U = op.jvp(Vin)
        A = op.vjp(U)
        off = 0
        for j in idx:
            st = states[j]
            done = st.advance(U[off:off + ranks[j]], A[off:off + ranks[j]], convergence_threshold, last=(i == max_iter - 1))
            if verbose:
                print(f'block krylov [{names[j]}] : {i}-th step ({st.m_ritz} rows) convergence : {st.dist}  residual : {st.max_resid}')
            if done:
                active[j] = False
            off += ranks[j]
    engine.pmp_set_second_mask(None)
    out = []
    for j, m in ((0, mask_a), (1, mask_b)):
        mflat = m.to(dev).reshape(-1)
        if not bool(mflat.any()):
            raise ValueError("empty mask: J = d x0_hat[mask] / d x_t has no rows")
        st = states[j]
        U, s, V, resid = st.finish(sharder)
        infos[j].update(residual=[float(r) for r in resid.tolist()], reason=st.reason, rows=st.m_ritz, solver="krylov")
        out.append((U[:, mflat].T.contiguous(), s.sqrt(), V, st.steps))
    if info is not None:
        info.extend(infos)
    if verbose:
        torch.cuda.synchronize()
        print('block krylov runtime (both solves) ==', time.time() - time_s)
    return out[0], out[1]
