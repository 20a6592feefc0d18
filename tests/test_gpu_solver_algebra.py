"""The solver's dense algebra (csrc/solver.hip: loco_orthonormalize, loco_qr_rows, loco_convergence_rows,
loco_convergence, loco_null_project) against float64 LAPACK on graded, clustered and rank-deficient spectra, at row
lengths that leave partial blocks in every kernel (Gram chunks of 256 columns, sign segments of 4096 elements, the
64-segment cap of the row-wise convergence test) and on a context wide enough (n = 49152) for the capped loops to loop.

Every input is built in float64 with prescribed singular values, (U diag(sigma)) W^T with U, W from QR of Gaussian draws
under fixed seeds, and rounded to fp32; every reference is float64 torch.linalg.svd / qr (or a float64 restatement of the
formula) of THE ROUNDED matrix on the CPU.  A row is *determined* when its float64 s_i >= 1e-6 s_0; include/loco_hip.h
states what loco_orthonormalize returns for the others.

Worst values of one run on an MI355X next to the bound each is held to (each test prints its own figures, -s shows them):

    part                                   figure                              worst measured   bound
    -------------------------------------  ----------------------------------  ---------------  -----------
    1 orthonormalize, graded / clustered   max |V V^T - I|                     6.2e-08          < 2e-5
                                           |s - s64| / s64                     5.6e-08          <= 1e-4
                                           1 - |cos| (clusters: principal)     3.1e-08          < 1e-3
    2 undetermined rows                    determined rows: max |V V^T - I|    4.3e-09          < 2e-5
                                           determined rows: |s - s64| / s64    4.3e-08          <= 1e-4
                                           determined rows: 1 - |cos|          2.2e-09          < 1e-3
                                           |s - s64| / s64_0, every row        3.5e-08          <= 1e-6
                                           other rows: largest norm            1.0000000        <= 1 + 2e-5
                                           other rows: |<row, determined>|     1.1e-09          <= 2e-5
    3 sign convention                      1 - signed cos                      4.2e-09          < 1e-3
    4 qr_rows                              max |Q Q^T - I|                     5.6e-08          < 2e-5
                                           1 - |cos|                           2.6e-08          < 1e-4
    5 convergence_rows                     distance, rel. to float64           3.6e-08          <= 1e-5
      convergence (flat)                   distance, rel. to float64           1.2e-08          <= 1e-5
    6 null_project                         rel-L2                              6.4e-08          < 1e-5
                                           | ||row|| - 1 |                     5.8e-08          <= 1e-6
                                           |<row, Vn>|                         1.9e-08          <= 1e-6
    7 subspace_iteration, 12 iterations    max |V V^T - I|                     4.9e-08          < 2e-5
                                           |s - s64| / s64                     7.1e-08          <= 1e-3
                                           1 - |cos|                           1.0e-09          < 1e-4
                                           rank 8 of 16: s[8:] / s[0]          0 (zero rows)    <= 1e-6

Before the eigenvalue floor and the gated Cholesky pass of loco_orthonormalize the same run gave, at the same bounds:
max |V V^T - I| = 2.1e-5 (k = 16, 1e6, n = 3071) and 3.7e-5 (k = 2, 1e6, n = 4097); undetermined rows of norm 1.0076
with |<row, determined>| = 1.9e-4 (condition 1e8), 1.098 (rank 5 of 8) and 1.479 (rank 8 of 16); and in the rank-8 loop a
row of norm 1.003 with |<row, determined>| = 0.17.  (k = 64, 1e6, n = 4097 held there: 7.2e-6.)
"""
import functools
import math

import pytest
import torch

from loco_edit_amd.config import TINY_DDPM, UNetConfig, synth_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# TINY's widths at 128 x 128: n = 49152 > 16384, so conv_rows_partial_kernel loops under its 64-segment cap, the Gram has
# 192 > 64 column blocks and the grid-stride loops of the row kernels (<= 1024 blocks of 256) are still one pass
WIDE = UNetConfig(resolution=128, ch=32, ch_mult=(1, 1, 2, 2), num_res_blocks=1, attn_resolutions=(16,))

ORTH = 2e-5          # max |V V^T - I|, the bound of test_gpu_parity.test_solver_algebra_kernels
S_RTOL = 1e-4        # singular values against float64
COS = 0.999          # |cos| of a row against the float64 right singular vector
UNDET = 1e-6         # s_i < UNDET * s_0: the row is not determined by fp32 data


@pytest.fixture(scope="module")
def engines():
    import os
    from loco_edit_amd.hip import LocoEngine, library_path
    assert os.path.exists(library_path())
    cache = {}

    def get(n):
        """The engine whose context is wide enough for rows of n elements (the ABI takes any n up to the context's)."""
        cfg = TINY_DDPM if n <= TINY_DDPM.n else WIDE
        assert n <= cfg.n
        if cfg not in cache:
            e = LocoEngine(cfg, max_batch=1, device=torch.device(DEV))
            e.load_state_dict(synth_params(cfg, 0))
            cache[cfg] = e
        return cache[cfg]
    return get


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references (computed once per case and shared; never modified)
def _orth_cols(rows, cols, g):
    return torch.linalg.qr(torch.randn(rows, cols, generator=g, dtype=torch.float64))[0]


def _with_spectrum(sigma, n, seed):
    """(U diag(sigma)) W^T in float64, rounded to fp32: [k, n] with singular values sigma (up to the rounding)."""
    g = torch.Generator().manual_seed(seed)
    sigma = torch.as_tensor(sigma, dtype=torch.float64)
    k = sigma.numel()
    return ((_orth_cols(k, k, g) * sigma) @ _orth_cols(n, k, g).T).float().contiguous()


def _graded(k, cond, scale=3.0):
    return scale * torch.logspace(0, -math.log10(cond), k, dtype=torch.float64) if k > 1 else torch.tensor([scale], dtype=torch.float64)


CLUSTERED = [4, 4 * (1 - 1e-6), 4 * (1 - 2e-6), 1, 1, 1 - 1e-7, .3, .1]
CLUSTERS = [[0, 1, 2], [3, 4, 5], [6], [7]]


@functools.lru_cache(maxsize=None)
def _svd_case(kind, k, n, cond, seed):
    """-> (A fp32 [k, n], s64 [k], vt64 [k, n]) with s64, vt64 = float64 SVD of the fp32 matrix."""
    g = torch.Generator().manual_seed(seed)
    if kind == "graded":
        A = _with_spectrum(_graded(k, cond), n, seed)
    elif kind == "clustered":
        A = _with_spectrum(CLUSTERED, n, seed)
    elif kind == "rank":          # exact rank `cond`: Gaussian k x r times Gaussian r x n
        A = (torch.randn(k, cond, generator=g, dtype=torch.float64) @ torch.randn(cond, n, generator=g, dtype=torch.float64)).float()
    elif kind == "zero":
        A = torch.zeros(k, n)
    elif kind == "lastcol":       # the top right singular vector peaks at the very last element
        A64 = _with_spectrum(_graded(k, cond), n, seed).double()
        A64[:, -1] *= 200.0
        A = A64.float()
    else:
        raise ValueError(kind)
    A = A.contiguous()
    _, s64, vt64 = torch.linalg.svd(A.double(), full_matrices=False)
    return A, s64, vt64


def _run_orth(engines, A):
    V = A.to(DEV).clone()
    s = engines(A.shape[1]).orthonormalize_(V)
    return V.cpu().double(), s.cpu().double()


def _orth_err(V):
    return (V @ V.T - torch.eye(V.shape[0], dtype=V.dtype)).abs().max().item() if V.shape[0] else 0.0


def _principal_cos(Va, Vb):
    """Smallest principal cosine between the row spans of Va and Vb (both orthonormalised in float64 first)."""
    qa = torch.linalg.qr(Va.T)[0]
    qb = torch.linalg.qr(Vb.T)[0]
    return torch.linalg.svdvals(qa.T @ qb).min().item()


# ---------------------------------------------------------------------------------------------------------------------
# 1. loco_orthonormalize on graded spectra and odd lengths
ORTH_CASES = [
    # (kind, k, n, condition number, seed)
    ("graded", 1, 1, 1, 11),                 # n = k = 1
    ("graded", 2, 2, 1e3, 12),               # n = k, a full matrix
    ("graded", 5, 255, 1e5, 13),             # one partial Gram chunk
    ("graded", 5, 257, 1e3, 14),             # one full chunk + one column
    ("graded", 16, 3071, 1e6, 15),
    ("graded", 16, 3072, 1e5, 16),
    ("graded", 33, 3071, 1e5, 17),           # odd k: one player idle in the round-robin
    ("graded", 63, 257, 1e3, 18),
    ("graded", 64, 64, 1e3, 19),             # n = k = 64, a full matrix
    ("graded", 64, 4097, 1e6, 20),           # wide engine: one-element tail of the sign segments
    ("graded", 64, 49152, 1e4, 21),          # 192 Gram blocks
    ("graded", 1, 49152, 1, 22),
    ("graded", 2, 4097, 1e6, 23),
    ("clustered", 8, 3071, 0, 24),
]


@pytest.mark.parametrize("kind,k,n,cond,seed", ORTH_CASES, ids=[f"{c[0]}-k{c[1]}-n{c[2]}-c{c[3]:g}" for c in ORTH_CASES])
def test_orthonormalize_graded_spectra(kind, k, n, cond, seed, engines):
    A, s64, vt64 = _svd_case(kind, k, n, cond, seed)
    V, s = _run_orth(engines, A)
    orth = _orth_err(V)
    s_rel = ((s - s64).abs() / s64).max().item()
    if kind == "clustered":      # rows inside a cluster are defined up to a rotation: compare the cluster's span
        cos = min(_principal_cos(V[c], vt64[c]) for c in CLUSTERS)
    else:
        cos = (V * vt64).sum(dim=1).abs().min().item()
    print(f"orthonormalize {kind} k={k} n={n} cond={cond:g}: orth {orth:.2e} s_rel {s_rel:.2e} 1-cos {1 - cos:.2e}")
    assert torch.isfinite(V).all() and torch.isfinite(s).all()
    assert orth < ORTH
    assert s_rel <= S_RTOL
    assert cos > COS


# ---------------------------------------------------------------------------------------------------------------------
# 2. beyond fp32 resolution and rank deficiency
def _check_contract(tag, V, s, s64, vt64, cos_min=COS, s_rtol=S_RTOL, ref_rows=None):
    """The contract of loco_orthonormalize (include/loco_hip.h) against the float64 (s64, vt64)."""
    assert torch.isfinite(V).all() and torch.isfinite(s).all(), tag
    det = s64 >= UNDET * s64[0] if s64[0] > 0 else torch.zeros_like(s64, dtype=torch.bool)
    D, R = V[det], V[~det]
    ref = vt64 if ref_rows is None else ref_rows
    orth = _orth_err(D)
    s_rel = ((s[det] - s64[det]).abs() / s64[det]).max().item() if det.any() else 0.0
    cos = (D * ref[det]).sum(dim=1).abs().min().item() if det.any() else 1.0
    s_abs = ((s - s64).abs().max() / s64[0]).item() if s64[0] > 0 else s.abs().max().item()
    norm = R.norm(dim=1).max().item() if R.shape[0] else 0.0
    cross = (R @ D.T).abs().max().item() if R.shape[0] and D.shape[0] else 0.0
    print(f"{tag}: {int(det.sum())} determined of {len(s64)}: orth {orth:.2e} s_rel {s_rel:.2e} 1-cos {1 - cos:.2e} "
          f"|s-s64|/s0 {s_abs:.2e} other rows: max norm {norm:.7f} max |<row, determined>| {cross:.2e}")
    assert orth < ORTH, tag
    assert s_rel <= s_rtol, tag
    assert cos > cos_min, tag
    assert s_abs <= 1e-6, tag                       # fp32 resolution with a 4x margin (fp32 LAPACK: <= 2.5e-7)
    assert norm <= 1 + ORTH, tag                    # unit or zero, never longer
    assert cross <= ORTH, tag
    return det


DEFICIENT_CASES = [
    ("graded", 16, 3071, 1e8, 31),      # (a) the last rows lie below fp32 resolution
    ("rank", 8, 3071, 5, 32),           # (b) exact rank 5
    ("rank", 16, 4097, 8, 33),          # (c) rank 8, wide engine
    ("zero", 5, 257, 0, 34),            # (d) A = 0
]


@pytest.mark.parametrize("kind,k,n,cond,seed", DEFICIENT_CASES, ids=["cond1e8", "rank5of8", "rank8of16", "zero"])
def test_orthonormalize_undetermined_rows(kind, k, n, cond, seed, engines):
    A, s64, vt64 = _svd_case(kind, k, n, cond, seed)
    V, s = _run_orth(engines, A)
    det = _check_contract(f"orthonormalize {kind} k={k} n={n} ({cond:g})", V, s, s64, vt64)
    expect = {"graded": 12, "zero": 0}.get(kind, cond)      # 3 * 10^(-8 i / 15) >= 3e-6 for i <= 11
    assert int(det.sum()) == expect


# ---------------------------------------------------------------------------------------------------------------------
# 3. sign convention: the entry of largest magnitude of every non-zero row is positive
SIGN_CASES = [
    ("graded", 5, 3071, 1e3, 41),
    ("graded", 16, 257, 1e3, 42),
    ("lastcol", 3, 4097, 1e3, 43),      # row 0 peaks at element 4096: the one-element tail segment decides its sign
    ("rank", 8, 3071, 5, 32),           # zero rows stay zero
]


@pytest.mark.parametrize("kind,k,n,cond,seed", SIGN_CASES, ids=[f"{c[0]}-k{c[1]}-n{c[2]}" for c in SIGN_CASES])
def test_orthonormalize_sign_convention(kind, k, n, cond, seed, engines):
    A, s64, vt64 = _svd_case(kind, k, n, cond, seed)
    det = s64 >= UNDET * s64[0]
    ref = vt64[det]
    top2 = ref.abs().topk(2, dim=1).values
    gap = ((top2[:, 0] - top2[:, 1]) / top2[:, 0]).min().item()
    assert gap > 1e-3, "seed leaves a row whose two largest magnitudes are within 1e-3: the sign is not defined by the data"
    peak = ref.abs().argmax(dim=1)
    ref = ref * ref.gather(1, peak[:, None]).sign()
    if kind == "lastcol":
        assert peak[0].item() == n - 1
    V, _ = _run_orth(engines, A)
    nz = V.abs().amax(dim=1) > 0
    assert bool(nz[det].all())
    at_peak = V.gather(1, V.abs().argmax(dim=1)[:, None])[:, 0]
    cos = (V[det] * ref).sum(dim=1).min().item()
    print(f"sign {kind} k={k} n={n}: top-2 gap {gap:.2e} signed 1-cos {1 - cos:.2e} non-zero rows {int(nz.sum())}")
    assert bool((at_peak[nz] > 0).all())
    assert (V[det].abs().argmax(dim=1) == peak).all()
    assert cos > COS


# ---------------------------------------------------------------------------------------------------------------------
# 4. loco_qr_rows against float64 QR of the transpose
QR_CASES = [
    # (condition number or 0 for Gaussian rows, k, n, seed)
    (0, 1, 1, 51), (0, 5, 5, 52), (0, 64, 64, 53), (0, 5, 257, 54), (0, 64, 3071, 55), (0, 64, 49152, 56), (0, 1, 49152, 57),
    (1e3, 5, 3071, 58), (1e3, 64, 257, 59), (1e5, 5, 257, 60), (1e5, 64, 3071, 61), (1e5, 64, 49152, 62),
]


@functools.lru_cache(maxsize=None)
def _qr_case(cond, k, n, seed):
    if cond:
        A = _with_spectrum(_graded(k, cond), n, seed)
    else:
        A = torch.randn(k, n, generator=torch.Generator().manual_seed(seed))
    return A, torch.linalg.qr(A.double().T)[0].T


@pytest.mark.parametrize("cond,k,n,seed", QR_CASES, ids=[f"c{c[0]:g}-k{c[1]}-n{c[2]}" for c in QR_CASES])
def test_qr_rows(cond, k, n, seed, engines):
    A, q64 = _qr_case(cond, k, n, seed)
    Q = A.to(DEV).clone()
    engines(n).qr_rows_(Q)
    Q = Q.cpu().double()
    orth = _orth_err(Q)
    cos = (Q * q64).sum(dim=1).abs().min().item()
    print(f"qr_rows cond={cond:g} k={k} n={n}: orth {orth:.2e} 1-cos {1 - cos:.2e}")
    assert torch.isfinite(Q).all()
    assert orth < ORTH
    assert cos > 0.9999


# ---------------------------------------------------------------------------------------------------------------------
# 5. loco_convergence_rows / loco_convergence against a float64 restatement
ATOL = 1e-3
ATOL32 = float(torch.tensor(ATOL, dtype=torch.float32))      # what the kernel receives


def _rows_restated(a, b):
    """Per row the orientation with the smaller distance; flag = every row allclose(atol, rtol 1e-5) in that orientation;
    distance = sqrt(sum_rows min(||a - b||^2, ||a + b||^2)).  Ties take the first orientation (a - b), like min()."""
    a, b = a.double(), b.double()
    tol = ATOL32 + 1e-5 * b.abs()
    dp, dm = ((a - b) ** 2).sum(dim=1), ((a + b) ** 2).sum(dim=1)
    okp, okm = ((a - b).abs() <= tol).all(dim=1), ((a + b).abs() <= tol).all(dim=1)
    minus = dm < dp
    return math.sqrt(float(torch.where(minus, dm, dp).sum())), float(bool(torch.where(minus, okm, okp).all()))


def _flat_restated(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm()), float(bool(((a - b).abs() <= ATOL32 + 1e-5 * b.abs()).all()))


@functools.lru_cache(maxsize=None)
def _conv_pair(k, n, seed):
    """a [k, n] Gaussian; sg [k, 1] random signs; b = sg * a + noise of at most half the threshold (fp32)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(k, n, generator=g)
    sg = (torch.randint(0, 2, (k, 1), generator=g) * 2 - 1).float()
    b = sg * a + 0.5 * ATOL * (2 * torch.rand(k, n, generator=g) - 1)
    return a, sg, b


CONV_ROWS_CASES = [(1, 1, 71), (1, 255, 72), (5, 257, 73), (5, 16385, 74), (64, 255, 75), (64, 1, 76), (1, 49152, 77),
                   (64, 49152, 78)]


@pytest.mark.parametrize("k,n,seed", CONV_ROWS_CASES, ids=[f"k{c[0]}-n{c[1]}" for c in CONV_ROWS_CASES])
def test_convergence_rows_vs_float64(k, n, seed, engines):
    eng = engines(n)
    a, sg, b = _conv_pair(k, n, seed)

    def both(a_, b_):
        got = eng.convergence_rows(a_.to(DEV), b_.to(DEV), ATOL).tolist()
        return got, _rows_restated(a_, b_)

    got, (dist, flag) = both(a, b)
    rel = abs(got[0] - dist) / dist
    print(f"convergence_rows k={k} n={n}: distance rel err {rel:.2e} (float64 {dist:.6e})")
    assert flag == 1.0 and got[1] == 1.0
    assert rel <= 1e-5
    # one element, the last of the last row, at 1.5x the threshold
    b1 = b.clone()
    b1[-1, -1] = sg[-1, 0] * a[-1, -1] + 1.5 * (ATOL + 1e-5 * a[-1, -1].abs())
    got, (dist, flag) = both(a, b1)
    assert flag == 0.0 and got[1] == 0.0
    assert abs(got[0] - dist) / dist <= 1e-5
    # that element NaN
    b2 = b.clone()
    b2[-1, -1] = float("nan")
    assert eng.convergence_rows(a.to(DEV), b2.to(DEV), ATOL).tolist()[1] == 0.0
    # a row equally close in both orientations (b row = 0): far from it, then inside the tolerance
    b3 = b.clone()
    b3[0] = 0.0
    got, (dist, flag) = both(a, b3)
    assert flag == 0.0 and got[1] == flag and abs(got[0] - dist) / dist <= 1e-5
    a4 = a.clone()
    a4[0] = 0.4 * ATOL * (2 * (a[0] > 0).float() - 1)
    got, (dist, flag) = both(a4, b3)
    assert flag == 1.0 and got[1] == flag and abs(got[0] - dist) / dist <= 1e-5


@pytest.mark.parametrize("count", [1, 257, 64 * 49152])
def test_convergence_flat_vs_float64(count, engines):
    eng = engines(min(count, WIDE.n))
    g = torch.Generator().manual_seed(80 + count % 7)
    a = torch.randn(count, generator=g)
    b = a + 0.5 * ATOL * (2 * torch.rand(count, generator=g) - 1)
    got = eng.convergence(a.to(DEV), b.to(DEV), ATOL).tolist()
    dist, flag = _flat_restated(a, b)
    rel = abs(got[0] - dist) / dist
    print(f"convergence count={count}: distance rel err {rel:.2e}")
    assert flag == 1.0 and got[1] == 1.0 and rel <= 1e-5
    b1 = b.clone()
    b1[-1] = a[-1] + 1.5 * (ATOL + 1e-5 * a[-1].abs())
    got = eng.convergence(a.to(DEV), b1.to(DEV), ATOL).tolist()
    dist, flag = _flat_restated(a, b1)
    assert flag == 0.0 and got[1] == 0.0 and abs(got[0] - dist) / dist <= 1e-5
    b1[-1] = float("nan")
    assert eng.convergence(a.to(DEV), b1.to(DEV), ATOL).tolist()[1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 6. loco_null_project against float64 normalize(Vm - (Vm Vn^T) Vn)
NULL_CASES = [(1, 5, 257, 91), (5, 5, 3071, 92), (5, 64, 49152, 93), (64, 64, 3071, 94), (64, 64, 257, 95),
              (1, 5, 49152, 96), (3, 0, 257, 97)]


def _exact_orthonormal_rows(k0, n, g):
    """k0 rows of length n that are orthonormal EXACTLY, in fp32 as in float64: rows 1..k0 of the Sylvester Hadamard matrix
    of order m = the largest power of 4 <= n, entries +-2^-p = +-1/sqrt(m), on m columns drawn at random."""
    m = 4 ** int(math.log(n, 4) + 1e-9)
    r, c = torch.arange(1, k0 + 1)[:, None], torch.arange(m)[None, :]
    bits = r & c
    par = torch.zeros_like(bits)
    while bool(bits.any()):
        par ^= bits & 1
        bits = bits >> 1
    V = torch.zeros(k0, n, dtype=torch.float64)
    V[:, torch.randperm(n, generator=g)[:m]] = (1.0 - 2.0 * par.double()) / math.sqrt(m)
    return V


@functools.lru_cache(maxsize=None)
def _null_case(k, k0, n, seed, cancel):
    """Gaussian case: Vn = orthonormal rows from float64 QR rounded to fp32, Vm = Gaussian rows.
    Cancellation case: unit rows Vm with 1 - 1e-6 of their energy inside span(Vn), so that what the projection keeps has
    amplitude 1e-3.  The formula's own departure from span(Vn)'s complement is |Vn Vn^T - I| / 1e-3 there, which for
    QR rows rounded to fp32 is 3e-7 ... 9e-6 in float64 already; so that the 1e-6 bound measures the kernel, this case
    takes rows that are orthonormal exactly (_exact_orthonormal_rows)."""
    g = torch.Generator().manual_seed(seed)
    if cancel:
        Vn64 = _exact_orthonormal_rows(k0, n, g)
        inside = torch.nn.functional.normalize(torch.randn(k, k0, generator=g, dtype=torch.float64), dim=1) @ Vn64
        out = torch.randn(k, n, generator=g, dtype=torch.float64)
        out = torch.nn.functional.normalize(out - (out @ Vn64.T) @ Vn64, dim=1)
        Vm = (math.sqrt(1 - 1e-6) * inside + 1e-3 * out).float()
    else:
        Vn64 = _orth_cols(n, k0, g).T if k0 else None
        Vm = torch.randn(k, n, generator=g)
    Vn = Vn64.float().contiguous() if k0 else None
    assert not cancel or torch.equal(Vn.double(), Vn64)
    ref = Vm.double()
    if k0:
        ref = ref - (ref @ Vn.double().T) @ Vn.double()
    return Vm.contiguous(), Vn, torch.nn.functional.normalize(ref, dim=1)


def _check_null(tag, k, k0, n, seed, cancel, engines):
    Vm, Vn, ref = _null_case(k, k0, n, seed, cancel)
    out = engines(n).null_project(Vm.to(DEV), Vn.to(DEV) if k0 else None).cpu().double()
    rel = ((out - ref).norm() / ref.norm()).item()
    unit = (out.norm(dim=1) - 1).abs().max().item()
    perp = (out @ Vn.double().T).abs().max().item() if k0 else 0.0
    perp_ref = (ref @ Vn.double().T).abs().max().item() if k0 else 0.0
    print(f"null_project {tag} k={k} k0={k0} n={n}: rel-L2 {rel:.2e} |norm-1| {unit:.2e} |<row, Vn>| {perp:.2e} "
          f"(float64 reference itself: {perp_ref:.2e})")
    assert torch.isfinite(out).all()
    assert rel < 1e-5
    assert unit <= 1e-6
    assert perp <= 1e-6


@pytest.mark.parametrize("k,k0,n,seed", NULL_CASES, ids=[f"k{c[0]}-k0_{c[1]}-n{c[2]}" for c in NULL_CASES])
def test_null_project_vs_float64(k, k0, n, seed, engines):
    _check_null("gaussian", k, k0, n, seed, False, engines)


@pytest.mark.parametrize("k,k0,n,seed", [c for c in NULL_CASES if c[1]], ids=[f"k{c[0]}-k0_{c[1]}-n{c[2]}" for c in NULL_CASES if c[1]])
def test_null_project_under_cancellation(k, k0, n, seed, engines):
    _check_null("cancel", k, k0, n, seed + 100, True, engines)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the loop on a low-rank operator
class LapackAlgebra:                      # the double of tests/test_host_logic.py: raw LAPACK rows in float64
    def orthonormalize_(self, A):
        _, s, vh = torch.linalg.svd(A, full_matrices=False)
        A.copy_(vh)
        return s

    def convergence_rows(self, a, b, atol):
        sg = (a * b).sum(dim=1, keepdim=True).sign()
        return torch.tensor([torch.dist(a, b * sg).item(), float(torch.allclose(a, b * sg, atol=atol))])

    convergence = None


class DenseOp:
    """jvp = V J^T, vjp = U J for a dense J [m, n]."""

    def __init__(self, J):
        self.J = J
        self.n_out = J.shape[0]

    def jvp(self, V):
        return V @ self.J.T

    def vjp(self, U):
        return U @ self.J

    def gather(self, U):
        return U


LOOP_M, LOOP_N = 96, 3071


@functools.lru_cache(maxsize=None)
def _loop_case(which):
    """-> (J fp32 [96, 3071], V0 fp32 [k, n] orthonormal, s64, V64 of the same 12 iterations in float64 on the CPU)."""
    from loco_edit_amd import solver
    g = torch.Generator().manual_seed(7 if which == "graded" else 8)
    if which == "graded":        # A = V J^T J has the spectrum 1 ... 2.5e-3 on the five rows kept
        sigma = torch.cat([torch.tensor([1, .5, .25, .1, .05], dtype=torch.float64),
                           1e-3 * torch.rand(LOOP_M - 5, generator=g, dtype=torch.float64)])
        k = 5
    else:                        # exact rank 8 under 16 probes: more probes than directions in every iteration
        sigma = torch.cat([torch.logspace(0, -2, 8, dtype=torch.float64), torch.zeros(LOOP_M - 8, dtype=torch.float64)])
        k = 16
    J = ((_orth_cols(LOOP_M, LOOP_M, g) * sigma) @ _orth_cols(LOOP_N, LOOP_M, g).T).float().contiguous()
    V0 = _orth_cols(LOOP_N, k, g).T.float().contiguous()
    _, s64, V64, n_it = solver.subspace_iteration(DenseOp(J.double()), LapackAlgebra(), V0.double().clone(), min_iter=12,
                                                  max_iter=12, verbose=False)
    assert n_it == 12
    return J, V0, s64, V64


@pytest.mark.parametrize("which", ["graded", "rank8of16"])
def test_subspace_iteration_on_a_low_rank_operator(which, engines):
    from loco_edit_amd import solver
    J, V0, s64, V64 = _loop_case(which)
    eng = engines(LOOP_N)
    _, s, V, n_it = solver.subspace_iteration(DenseOp(J.to(DEV)), eng, V0.to(DEV).clone(), min_iter=12, max_iter=12,
                                              verbose=False)
    assert n_it == 12
    V, s = V.cpu().double(), s.cpu().double()
    # the project's solver bounds on the determined rows: |cos| >= 0.9999 and s to rtol 1e-3
    det = _check_contract(f"subspace_iteration {which}", V, s, s64, V64, cos_min=0.9999, s_rtol=1e-3)
    if which == "rank8of16":
        assert int(det.sum()) == 8
        assert bool((s[8:] <= 1e-6 * s[0]).all())
        assert V[8:].norm(dim=1).max().item() <= 1 + ORTH
    else:
        assert int(det.sum()) == 5
