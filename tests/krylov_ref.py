"""Float64 torch restatement of the block Krylov solver (DESIGN.md "Block Krylov solver"), step for step, written from
the algorithm's statement and not from the HIP kernels.  It serves two purposes:

* ``krylov_reference``: the whole solve on a dense J, the reference of the host tests (checked there against the float64
  SVD of J) and of the GPU tests that compare per-step quantities;
* ``RefAlgebra``: the three primitives ``solver.krylov_iteration`` asks of its algebra (krylov_extend / krylov_ritz /
  krylov_left), as a CPU double for the sharding tests under gloo.

``store`` is the dtype the rows of Q, J Q and Y are rounded to when they are written (float32 reproduces the fp32 rows
with double accumulation of the device code; float64 is the exact-arithmetic algorithm).
"""
import math

import torch

ROWS = 64            # rows the eigensolver takes
DROP = 1e-6          # singular value of a residual direction, relative to theta_0, below which the row becomes zero
REORTHO = 1e-7       # eigenvalue ratio of the block's Gram below which the rotated rows take one Cholesky pass


def _rt(x, store):
    return x.to(store).double()


def _sign_fix(Y):
    """Entry of largest magnitude of every row positive (a zero row keeps sign +1)."""
    peak = Y.gather(1, Y.abs().argmax(dim=1, keepdim=True))[:, 0]
    sg = torch.where(peak < 0, -torch.ones_like(peak), torch.ones_like(peak))
    return Y * sg[:, None], sg


def _eigh_desc(T):
    w, v = torch.linalg.eigh(T)
    return w.flip(0), v.flip(1).T.contiguous()        # rows = eigenvectors, descending eigenvalue


def _rows_test(a, b, atol):
    """The aligned convergence test (loco_convergence_rows): per row the closer orientation."""
    a, b = a.double(), b.double()
    tol = atol + 1e-5 * b.abs()
    dp, dm = ((a - b) ** 2).sum(dim=1), ((a + b) ** 2).sum(dim=1)
    okp, okm = ((a - b).abs() <= tol).all(dim=1), ((a + b).abs() <= tol).all(dim=1)
    minus = dm < dp
    return math.sqrt(float(torch.where(minus, dm, dp).sum())), float(bool(torch.where(minus, okm, okp).all()))


class KrylovAlgebra64:
    """The context's side of one solve: T, the Ritz pairs, G and the signs, in float64."""

    def __init__(self, store=torch.float32):
        self.store = store
        self.T = torch.zeros(ROWS, ROWS, dtype=torch.float64)
        self.theta = self.W = self.G = self.sign = None

    def extend(self, A, Q, m, want_next=True):
        """A [k, n] float64 = J^T J Q[m-k:m].  -> (next block [k, n] or None, all_zero)."""
        k = A.shape[0]
        Qm = Q[:m].double()
        C = A @ Qm.T                                        # step 2: k x m
        self.T[m - k:m, :m] = C
        self.T[:m, m - k:m] = C.T
        D = C[:, m - k:m]
        self.T[m - k:m, m - k:m] = 0.5 * (D + D.T)
        R = _rt(A - C @ Qm, self.store)                     # step 3: two passes of block Gram-Schmidt
        R = _rt(R - (R @ Qm.T) @ Qm, self.store)
        self.G = R @ R.T
        self.theta, self.W = _eigh_desc(self.T[:m, :m])     # step 4
        if not want_next:
            return None, False
        lam, P = _eigh_desc(self.G)                         # step 6
        keep = (lam > 0) & (lam.clamp_min(0).sqrt() >= DROP * self.theta[0])
        scale = torch.where(keep, 1.0 / lam.clamp_min(1e-300).sqrt(), torch.zeros_like(lam))
        N = _rt((P * scale[:, None]) @ R, self.store)
        if bool(keep.any()) and lam[keep].min() < REORTHO * lam[0]:
            # graded block: one Cholesky pass in the order of descending singular value, as loco_orthonormalize does
            N = N.clone()
            for i in range(k):
                if not keep[i]:
                    continue
                v = N[i] - (N[:i] @ N[i]) @ N[:i]
                nv = v.norm()
                N[i] = v / nv if nv * nv >= 0.25 else 0.0
            N = _rt(N, self.store)
        N = _rt(N - (N @ Qm.T) @ Qm, self.store)            # one more projection against Q
        return N, not bool(keep.any())

    def ritz(self, Q, m, k):
        """-> (Y [k, n] signed, resid [k])."""
        Y, self.sign = _sign_fix(_rt(self.W[:k] @ Q[:m].double(), self.store))
        w = self.W[:k, m - k:m]
        q = ((w @ self.G) * w).sum(dim=1).clamp_min(0)
        resid = q.sqrt() / self.theta[0] if self.theta[0] > 0 else torch.zeros(k, dtype=torch.float64)
        return Y, resid

    def left(self, Ustore, m, k):
        UY = _rt((self.W[:k] @ Ustore[:m].double()) * self.sign[:, None], self.store)
        return UY, (UY * UY).sum(dim=1)


def krylov_reference(J, V0, max_iter, thr=1e-3, store=torch.float32, history=None):
    """The whole solve on a dense J [n_out, n] (float64).  -> (U [k, n_out], s [k], V [k, n], n_steps, resid [k], reason).
    ``history`` (a list) receives per step a dict with Y, resid, theta, m."""
    J = J.double()
    k, n = V0.shape
    if k > ROWS // 2:
        raise ValueError("k > 32: two blocks do not fit in 64 rows")
    cap = (ROWS // k) * k
    alg = KrylovAlgebra64(store)
    Q = torch.zeros(cap, n, dtype=torch.float64)
    Q[:k] = _rt(V0.double(), store)
    Ustore = torch.zeros(cap, J.shape[0], dtype=torch.float64)
    m, steps, reason, Yprev, Y, resid = k, 0, None, None, None, None
    for j in range(max_iter):
        U = _rt(Q[m - k:m] @ J.T, store)
        Ustore[m - k:m] = U
        A = _rt(U @ J, store)
        room = m + k <= cap and j != max_iter - 1
        nxt, all_zero = alg.extend(A, Q, m, want_next=room)
        Y, resid = alg.ritz(Q, m, k)
        steps += 1
        if history is not None:
            history.append(dict(Y=Y.clone(), resid=resid.clone(), theta=alg.theta[:k].clone(), m=m))
        conv = Yprev is not None and _rows_test(Yprev, Y, thr)[1] > 0.5
        Yprev = Y
        if room and all_zero:
            reason = "invariant"
        elif conv:
            reason = "converged"
        elif not room:
            reason = "max_iter" if j == max_iter - 1 else "full"
        if reason:
            break
        Q[m:m + k] = nxt
        m += k
    UY, s = alg.left(Ustore, m, k)
    return UY, s, Y, steps, resid, reason


class RefAlgebra:
    """CPU double of the engine's Krylov primitives for ``solver.krylov_iteration`` (tensors of any float dtype; the
    arithmetic is float64, rows are stored in the tensors' own dtype)."""

    def __init__(self):
        self.slots = {}

    def krylov_extend(self, A, Q, m, nxt, stat, slot=0):
        if m == A.shape[0]:
            self.slots[slot] = KrylovAlgebra64(store=Q.dtype)
        N, all_zero = self.slots[slot].extend(A.double(), Q, m, want_next=nxt is not None)
        if nxt is not None:
            nxt.copy_(N.to(nxt.dtype))
        stat[3] = 1.0 if all_zero else 0.0

    def krylov_ritz(self, Q, m, Y, Yprev, atol, resid, stat, slot=0):
        k = Y.shape[0]
        y, r = self.slots[slot].ritz(Q, m, k)
        Y.copy_(y.to(Y.dtype))
        resid.copy_(r.to(resid.dtype))
        stat[2] = float(r.max())
        stat[0], stat[1] = _rows_test(Yprev, Y, atol) if Yprev is not None else (-1.0, 0.0)

    def krylov_left(self, Ustore, m, UY, s, slot=0):
        u, sq = self.slots[slot].left(Ustore, m, UY.shape[0])
        UY.copy_(u.to(UY.dtype))
        s.copy_(sq.to(s.dtype))


# ---- operators of the issue's convergence cases -----------------------------------------------------------------------
def orth_cols(rows, cols, g):
    return torch.linalg.qr(torch.randn(rows, cols, generator=g, dtype=torch.float64))[0]


def with_spectrum(sigma, n, seed):
    """(U diag(sigma)) W^T in float64 rounded to fp32, the formula of tests/test_gpu_solver_algebra.py::_with_spectrum."""
    g = torch.Generator().manual_seed(seed)
    sigma = torch.as_tensor(sigma, dtype=torch.float64)
    k = sigma.numel()
    return ((orth_cols(k, k, g) * sigma) @ orth_cols(n, k, g).T).float().contiguous()


def operator(which, rows=96, n=3071):
    """``harmonic``: sigma_i = 1 / (1 + 0.1 i); ``log``: 3 logspace(0, -3); ``rank8`` / ``rank3``: Gaussian rows x r times r x n
    (exact rank r)."""
    if which == "harmonic":
        return with_spectrum(1.0 / (1.0 + 0.1 * torch.arange(rows, dtype=torch.float64)), n, 3)
    if which == "log":
        return with_spectrum(3.0 * torch.logspace(0, -3, rows, dtype=torch.float64), n, 3)
    if which in ("rank8", "rank3"):
        g, r = torch.Generator().manual_seed(5), int(which[4:])
        return (torch.randn(rows, r, generator=g, dtype=torch.float64) @ torch.randn(r, n, generator=g, dtype=torch.float64)).float()
    raise ValueError(which)


def start_block(n, k, seed=7):
    """QR of randn(n, k) under Generator().manual_seed(seed), transposed: orthonormal rows [k, n].  Drawn and factored in
    float64 (the draw under which power iteration scores 0.9966 at 12 iterations on ``harmonic``), rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.linalg.qr(torch.randn(n, k, generator=g, dtype=torch.float64))[0].T.float().contiguous()


def principal_cos(Va, Vb):
    """Smallest principal cosine between the row spans of Va and Vb."""
    qa = torch.linalg.qr(Va.double().T)[0]
    qb = torch.linalg.qr(Vb.double().T)[0]
    return torch.linalg.svdvals(qa.T @ qb).min().item()
