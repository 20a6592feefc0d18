"""Torch restatement of the device PCA (csrc/pca.hip, include/loco_hip.h loco_pca_fit): the same algorithm on the same
``omega``, in whatever dtype the sample matrix arrives in (float64: the truth the tests compare with; float32: the yardstick
for what fp32 arithmetic in another summation order may cost).

    Hc = H - mean(H)                      (center)
    Q  = orth(Hc omega)
    niter times:  Z = orth(Hc^T Q),  Q = orth(Hc Z)
    B  = Hc^T Q;  B^T B = E diag(lambda) E^T, lambda descending
    s  = sqrt(lambda),  V = B E / s,  each column of V flipped so that its entry of largest magnitude is positive

orth is CholeskyQR2: twice  G = Y^T Y,  G = L L^T,  Y <- Y L^-T.  A pivot of the first factor below ``PIVOT_FLOOR`` of its
column's squared norm raises ``RankError`` with the numerical rank.  ``s`` are the singular values of Hc (no 1 / sqrt(N - 1)),
as ``torch.pca_lowrank`` returns them.
"""
import torch

PIVOT_FLOOR = 2.0 ** -30


class RankError(RuntimeError):
    pass


def center_rows(H):
    """(Hc, mean): the mean is taken in float64 whatever the dtype, the difference is rounded once."""
    mean = H.double().mean(dim=0)
    return (H.double() - mean).to(H.dtype), mean.to(H.dtype)


def cholesky_qr2(Y, what="Y"):
    q = Y.shape[1]
    for rep in range(2):
        G = Y.T @ Y
        L = torch.zeros_like(G)
        for j in range(q):                      # the factorisation written out: the pivots are the rank test
            d = G[j, j] - (L[j, :j] ** 2).sum()
            if rep == 0 and not bool(d >= PIVOT_FLOOR * G[j, j]):
                raise RankError(f"numerical rank {j} is below q = {q} ({what})")
            L[j, j] = d.sqrt()
            L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        Y = torch.linalg.solve_triangular(L, Y.T, upper=False).T          # Y L^-T
    return Y


def sign_fix(V):
    """Each column: the entry of largest magnitude (the first on a tie) becomes positive."""
    idx = V.abs().argmax(dim=0)
    sgn = torch.where(V[idx, torch.arange(V.shape[1])] < 0, -1.0, 1.0).to(V.dtype)
    return V * sgn


def pca_lowrank_oracle(H, q, niter, omega, center=True):
    """(s [q], V [D, q], mean [D]) in H's dtype; ``omega [D, q]`` is cast to it."""
    N, D = H.shape
    if q > min(N - 1 if center else N, D):
        raise ValueError(f"q = {q} exceeds min({'N - 1' if center else 'N'}, D)")
    omega = omega.to(H.dtype)
    if tuple(omega.shape) != (D, q):
        raise ValueError(f"omega must be [{D}, {q}]")
    Hc, mean = center_rows(H) if center else (H, torch.zeros(D, dtype=H.dtype))
    Q = cholesky_qr2(Hc @ omega, "Hc omega")
    for _ in range(niter):
        Z = cholesky_qr2(Hc.T @ Q, "Hc^T Q")
        Q = cholesky_qr2(Hc @ Z, "Hc Z")
    B = Hc.T @ Q
    lam, E = torch.linalg.eigh(B.T @ B)
    lam, E = lam.flip(0), E.flip(1)
    if not bool((lam > PIVOT_FLOOR * lam[0]).all()):
        raise RankError(f"numerical rank {int((lam > PIVOT_FLOOR * lam[0]).sum())} is below q = {q} (B^T B)")
    s = lam.sqrt()
    return s, sign_fix((B @ E) / s), mean


def graded_matrix(N, D, q_spec, base, ratio, offset, seed):
    """[N, D] float32 with centred singular values base * ratio^i (i < q_spec) on random orthonormal factors, plus
    ``offset`` on every column: the spectrum the bars of tests/test_pca_host.py are stated for."""
    g = torch.Generator().manual_seed(seed)
    U = torch.linalg.qr(torch.randn(N, q_spec, generator=g, dtype=torch.float64))[0]
    U = torch.linalg.qr(U - U.mean(dim=0))[0]                 # columns orthogonal to the ones vector: centring leaves them alone
    W = torch.linalg.qr(torch.randn(D, q_spec, generator=g, dtype=torch.float64))[0]
    s = base * ratio ** torch.arange(q_spec, dtype=torch.float64)
    return ((U * s) @ W.T + offset).float()


def cos_columns(A, B):
    """|cos| between matching columns."""
    A, B = A.double(), B.double()
    return ((A * B).sum(dim=0) / (A.norm(dim=0) * B.norm(dim=0))).abs()
