// Randomized, centred low-rank PCA of a sample matrix that stays on the device (include/loco_hip.h loco_pca_*): the global
// and local h-space PCA baselines (hspace_pca.py).  The handle owns the sample store H [n_max][d] (fp32), its centred copy
// Hc and every workspace; rows arrive with loco_pca_add_rows, loco_pca_fit returns (s [q], V [d][q], mean [d]).
//
// Algorithm (torch.pca_lowrank's family; restated in float64 by tests/pca_oracle.py), Omega [d][q] from the caller:
//     Q = orth(Hc Omega);   niter times:  Z = orth(Hc^T Q),  Q = orth(Hc Z);   B = Hc^T Q;
//     B^T B = E diag(lambda) E^T (lambda descending):  s = sqrt(lambda),  V = B E / s,
// and every column of V is flipped so that its entry of largest magnitude is positive (the rule solver.hip's sign_cand /
// sign_apply apply to basis rows; ties: the first such entry).  s are the singular values of Hc, no 1 / sqrt(N - 1).
//
// Arithmetic:
//   - centring: column means in double (each thread one column over one row part, parts joined in order), Hc = fp32(H - mu)
//     formed in double and rounded once.  The rank-one form H W - 1 (mu^T W) is not used anywhere.
//   - orth = CholeskyQR2.  The Gram Y^T Y (q x q) is summed in double from the fp32 operand (a product of two fp32 values is
//     exact in double): the long dimension L is cut into parts at positions that depend on L alone (pca_seg), each part's
//     q x q sum is one block-local chain per element, and the parts are added in order by a second kernel -- no atomics.  The
//     q x q Cholesky, the inverse of its factor and the final eigendecomposition run in double on the host (one read-back of
//     q x q doubles each); the factor is applied on the device as a product Y R^-1.
//   - pivots: a column whose pivot -- what is left of its squared norm after the columns before it -- is below
//     PCA_PIVOT_FLOOR of that squared norm has no direction of its own.  This is solver.hip's drop_below convention
//     (kernels.h launch_cholesky) on columns scaled to unit norm; there it zeroes a row, here it is an error that names the
//     numerical rank and q, and no output is written.
//   - the two large products Hc W and Hc^T Q read Hc with swapped strides (no transpose is stored).  Where the 64 x 64
//     output grid fills the chip they are launch_gemm (exact fp32 MFMA); where it does not -- a few hundred rows against a
//     contraction of 32 768 -- pca_gemm_kernel: 64 x 64 tiles of fp32 FMAs over a part of the contraction, the parts' tiles
//     added in order in double (pca_join_kernel).  Part boundaries depend on the shape alone.
//   - determinism: nothing above depends on how the rows were appended or on a previous call; no atomics anywhere.
#include "encoder_common.h"

#include <cmath>
#include <cstdio>

// pivot floor relative to the column's own squared norm: an fp32 product over a contraction of up to 32 768 terms carries a
// relative error of about sqrt(K) 2^-24 = 1e-5, so an independent part below 2^-15 of the column (2^-30 of its square) is
// not distinguishable from the rounding of the product that made the column
constexpr double PCA_PIVOT_FLOOR = 0x1p-30;
constexpr int PCA_Q_LIMIT = 512;
constexpr int PCA_MAX_PARTS = 64;                 // parts of a Gram / of the column sums
constexpr long PCA_SPLIT_WS = 2048L * 4096;       // floats of split-contraction partial tiles (see pca_split_plan)
constexpr int PCA_FILL_TILES = 256;               // 64 x 64 output tiles from which launch_gemm takes a product (one per CU)

struct loco_pca : loco::EncoderBase {
    long n_max = 0, d = 0, n = 0;
    int q_max = 0;
    int route = 0;                 // 0: by grid size, 1: launch_gemm always, 2: the split-contraction kernel always
    bool centred_valid = false;    // Hc / mean hold the centring of the current n rows
    int centred_mode = -1;
    float *H = nullptr, *Hc = nullptr, *Y0 = nullptr, *Y1 = nullptr, *Z0 = nullptr, *Z1 = nullptr, *small = nullptr, *split = nullptr,
          *meanf = nullptr;
    double *mean = nullptr, *colpart = nullptr, *G = nullptr, *gpart = nullptr;
    std::string routes;            // the routes of the last products, for the profile
};

namespace loco {
namespace {

std::string g_pca_create_err;

// length of a part of a long dimension L: a multiple of 256, at most PCA_MAX_PARTS parts.  A function of L alone.
inline long pca_seg(long L) {
    long seg = (L + PCA_MAX_PARTS - 1) / PCA_MAX_PARTS;
    seg = (seg + 255) / 256 * 256;
    return seg < 256 ? 256 : seg;
}
inline int pca_parts(long L) { return (int)((L + pca_seg(L) - 1) / pca_seg(L)); }

// part[p][c] = sum over rows r of part p of H[r][c], in double, rows in order.  grid (ceil(d / 256), parts)
__global__ __launch_bounds__(256) void pca_colsum_kernel(const float* H, long n, long d, long seg, double* part) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const long r0 = (long)blockIdx.y * seg, r1 = r0 + seg < n ? r0 + seg : n;
    double s = 0.0;
    for (long r = r0; r < r1; ++r) s += (double)H[r * d + c];
    part[(long)blockIdx.y * d + c] = s;
}
// mean[c] = (sum over parts in order) / n (center) or 0
__global__ __launch_bounds__(256) void pca_mean_kernel(const double* part, int parts, long n, long d, int center, double* mean,
                                                       float* meanf) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    if (center) {
        for (int p = 0; p < parts; ++p) s += part[(long)p * d + c];
        s /= (double)n;
    }
    mean[c] = s;
    meanf[c] = (float)s;
}
// Hc = fp32(double(H) - mean): one rounding
__global__ __launch_bounds__(256) void pca_centre_kernel(const float* H, const double* mean, long n, long d, float* Hc) {
    const long total = n * d;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        Hc[e] = (float)((double)H[e] - mean[e % d]);
}

// part[p][i][j] = sum over the rows l of part p of Y[l][i] Y[l][j] in double (Y [L][q] row-major, fp32).
// grid (ceil(q / 16), ceil(q / 16), parts), 256 threads: thread (ti, tj) owns one element of a 16 x 16 tile.
__global__ __launch_bounds__(256) void pca_gram_kernel(const float* Y, long L, int q, long seg, double* part) {
    __shared__ float Ai[64][17], Aj[64][17];
    const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const long l0 = (long)blockIdx.z * seg, l1 = l0 + seg < L ? l0 + seg : L;
    double acc = 0.0;
    for (long lb = l0; lb < l1; lb += 64) {
        for (int e = threadIdx.x; e < 64 * 16; e += 256) {
            const int r = e >> 4, c = e & 15;
            const long l = lb + r;
            Ai[r][c] = (l < l1 && i0 + c < q) ? Y[l * q + i0 + c] : 0.f;
            Aj[r][c] = (l < l1 && j0 + c < q) ? Y[l * q + j0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < 64; ++r) acc = fma((double)Ai[r][ti], (double)Aj[r][tj], acc);
        __syncthreads();
    }
    if (i0 + ti < q && j0 + tj < q) part[((long)blockIdx.z * q + i0 + ti) * q + j0 + tj] = acc;
}
// G[e] = sum over parts in order
__global__ __launch_bounds__(256) void pca_gram_join_kernel(const double* part, int parts, long qq, double* G) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= qq) return;
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += part[(long)p * qq + e];
    G[e] = s;
}

// C[m][n] (+ part offset) = sum over k of part z of A(m, k) B[k][n]: A with strides (sam, sak), B [K][N] row-major, C [M][N]
// row-major.  64 x 64 tile per block, 4 x 4 per thread, fp32 FMAs in k order.  AKM: sam == 1 (the m index is the fast one of A).
// grid (ceil(N / 64), ceil(M / 64), parts); out = C when parts == 1, else the partial tiles [parts][M][N]
template <bool AKM>
__global__ __launch_bounds__(256) void pca_gemm_kernel(const float* A, long sam, long sak, const float* B, int M, int N, int K, int klen,
                                                       float* out) {
    __shared__ float As[16][64 + 4], Bs[16][64 + 4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int k0 = blockIdx.z * klen, k1 = k0 + klen < K ? k0 + klen : K;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kb = k0; kb < k1; kb += 16) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int e = threadIdx.x + it * 256;
            int am, ak;
            if (AKM) { am = e & 63; ak = e >> 6; } else { ak = e & 15; am = e >> 4; }
            const int m = m0 + am, k = kb + ak;
            As[ak][am] = (m < M && k < k1) ? A[(long)m * sam + (long)k * sak] : 0.f;
            const int bn = e & 63, bk = e >> 6;
            const int n = n0 + bn, kk = kb + bk;
            Bs[bk][bn] = (n < N && kk < k1) ? B[(long)kk * N + n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[k][ty * 4 + i]; b[i] = Bs[k][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
    float* o = out + (long)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
            if (m < M && n < N) o[(long)m * N + n] = acc[i][j];
        }
}
// C[e] = fp32(sum over parts, in order, in double)
__global__ __launch_bounds__(256) void pca_join_kernel(const float* part, int parts, long mn, float* C) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= mn) return;
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += (double)part[(long)p * mn + e];
    C[e] = (float)s;
}

// per column j of V [d][q]: the entry of largest magnitude (the first one on a tie) becomes positive.  grid (q)
__global__ __launch_bounds__(256) void pca_sign_kernel(float* V, long d, int q) {
    __shared__ float bv[256];
    __shared__ long bi[256];
    const int j = blockIdx.x;
    float v = 0.f; long at = d;
    for (long r = threadIdx.x; r < d; r += 256) {
        const float x = V[r * q + j];
        if (fabsf(x) > fabsf(v)) { v = x; at = r; }          // r ascending: the first of equal magnitudes stays
    }
    bv[threadIdx.x] = v; bi[threadIdx.x] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float a = fabsf(bv[threadIdx.x]), b = fabsf(bv[threadIdx.x + s]);
            if (b > a || (b == a && bi[threadIdx.x + s] < bi[threadIdx.x])) { bv[threadIdx.x] = bv[threadIdx.x + s]; bi[threadIdx.x] = bi[threadIdx.x + s]; }
        }
        __syncthreads();
    }
    if (bv[0] < 0.f)
        for (long r = threadIdx.x; r < d; r += 256) V[r * q + j] = -V[r * q + j];
}

struct SplitPlan { int parts, klen; };
// parts of the contraction for an M x N product over K: enough parts for about 1024 blocks, each a multiple of 32 long and at
// least 256; one part (no partial tiles) from 1024 tiles up.  parts * M * N <= PCA_SPLIT_WS for every shape.
inline SplitPlan pca_split_plan(int M, int N, int K) {
    const long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
    long want = tiles >= 1024 ? 1 : (1024 + tiles - 1) / tiles;
    const long most = (K + 255) / 256;
    if (want > most) want = most;
    if (want < 1) want = 1;
    int klen = (int)((K + want - 1) / want);
    klen = (klen + 31) / 32 * 32;
    return {(K + klen - 1) / klen, klen};
}

// C [M][N] = A(m, k) B [K][N]; A(m, k) = A[m * sam + k * sak].  Returns the route's name.
const char* pca_product(loco_pca* p, const float* A, long sam, long sak, const float* B, float* Cm, int M, int N, int K, hipStream_t st) {
    const long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
    const bool gemm = p->route == 1 || (p->route == 0 && tiles >= PCA_FILL_TILES);
    if (gemm) {
        GemmArgs g; std::memset(&g, 0, sizeof(g));
        g.A = A; g.sam = sam; g.sak = sak;
        g.Bm = B; g.sbk = N; g.sbn = 1;
        g.C = Cm; g.scm = N; g.scn = 1;
        g.M = M; g.N = N; g.K = K; g.batch = 1; g.alpha = 1.f;
        launch_gemm(g, st);
        return "gemm";
    }
    const SplitPlan sp = pca_split_plan(M, N, K);
    float* out = sp.parts == 1 ? Cm : p->split;
    dim3 grid((N + 63) / 64, (M + 63) / 64, sp.parts);
    if (sam == 1) hipLaunchKernelGGL(pca_gemm_kernel<true>, grid, dim3(256), 0, st, A, sam, sak, B, M, N, K, sp.klen, out);
    else hipLaunchKernelGGL(pca_gemm_kernel<false>, grid, dim3(256), 0, st, A, sam, sak, B, M, N, K, sp.klen, out);
    if (sp.parts > 1) hipLaunchKernelGGL(pca_join_kernel, dim3(blocks256((long)M * N)), dim3(256), 0, st, p->split, sp.parts, (long)M * N, Cm);
    return sp.parts > 1 ? "split" : "tile";
}

void pca_gram(loco_pca* p, const float* Y, long L, int q, double* G, hipStream_t st) {
    const long seg = pca_seg(L);
    const int parts = pca_parts(L);
    const int t = (q + 15) / 16;
    hipLaunchKernelGGL(pca_gram_kernel, dim3(t, t, parts), dim3(256), 0, st, Y, L, q, seg, p->gpart);
    hipLaunchKernelGGL(pca_gram_join_kernel, dim3(blocks256((long)q * q)), dim3(256), 0, st, p->gpart, parts, (long)q * q, G);
}

bool pca_ok(loco_pca* p, hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    p->err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

// mean, Hc of the current rows (center == 0: mean = 0, Hc = H)
int pca_centre(loco_pca* p, int center, hipStream_t st) {
    center = center ? 1 : 0;
    if (p->centred_valid && p->centred_mode == center) return 0;
    const long seg = pca_seg(p->n);
    const int parts = pca_parts(p->n);
    const unsigned cb = blocks256(p->d);
    if (center) hipLaunchKernelGGL(pca_colsum_kernel, dim3(cb, parts), dim3(256), 0, st, p->H, p->n, p->d, seg, p->colpart);
    hipLaunchKernelGGL(pca_mean_kernel, dim3(cb), dim3(256), 0, st, p->colpart, parts, p->n, p->d, center, p->mean, p->meanf);
    const long total = p->n * p->d;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(pca_centre_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, st, p->H, p->mean, p->n, p->d, p->Hc);
    if (!pca_ok(p, hipGetLastError(), "loco_pca: centring launch")) return -1;
    p->centred_valid = true;
    p->centred_mode = center;
    return 0;
}

// Y [L][q] -> orthonormal columns (CholeskyQR2), result in *Y (the two buffers swap).  -1 with the message on a rank failure.
int pca_orth(loco_pca* p, float** Y, float** other, long L, int q, const char* what, hipStream_t st) {
    std::vector<double> G((size_t)q * q), Rinv((size_t)q * q);
    std::vector<float> Rf((size_t)q * q);
    for (int rep = 0; rep < 2; ++rep) {
        pca_gram(p, *Y, L, q, p->G, st);
        if (!pca_ok(p, hipMemcpyAsync(G.data(), p->G, G.size() * sizeof(double), hipMemcpyDeviceToHost, st), "loco_pca: Gram read-back") ||
            !pca_ok(p, hipStreamSynchronize(st), "loco_pca: Gram read-back"))
            return -1;
        // lower Cholesky in place (G = L L^T), pivots against the floor
        for (int j = 0; j < q; ++j) {
            const double gjj = G[(size_t)j * q + j];
            double dj = gjj;
            for (int k = 0; k < j; ++k) dj -= G[(size_t)j * q + k] * G[(size_t)j * q + k];
            if (!(gjj > 0.0) || !(dj >= PCA_PIVOT_FLOOR * gjj) || !std::isfinite(dj)) {
                char m[256];
                std::snprintf(m, sizeof(m), "loco_pca_fit: numerical rank %d is below q = %d (%s: the pivot of column %d is %.3g of its squared norm, "
                              "floor %.3g)", j, q, what, j, gjj > 0.0 ? dj / gjj : 0.0, PCA_PIVOT_FLOOR);
                p->err = m;
                return -1;
            }
            const double ljj = std::sqrt(dj);
            G[(size_t)j * q + j] = ljj;
            for (int i = j + 1; i < q; ++i) {
                double v = G[(size_t)i * q + j];
                for (int k = 0; k < j; ++k) v -= G[(size_t)i * q + k] * G[(size_t)j * q + k];
                G[(size_t)i * q + j] = v / ljj;
            }
        }
        // R = L^T (upper); Rinv = R^-1 (upper) = (L^-1)^T.  X = L^-1 by forward substitution, column by column.
        std::fill(Rinv.begin(), Rinv.end(), 0.0);
        for (int c = 0; c < q; ++c) {
            for (int i = c; i < q; ++i) {
                double v = i == c ? 1.0 : 0.0;
                for (int k = c; k < i; ++k) v -= G[(size_t)i * q + k] * Rinv[(size_t)c * q + k];      // Rinv[c][k] holds X[k][c]
                Rinv[(size_t)c * q + i] = v / G[(size_t)i * q + i];
            }
        }
        for (size_t e = 0; e < Rf.size(); ++e) Rf[e] = (float)Rinv[e];
        if (!pca_ok(p, hipMemcpyAsync(p->small, Rf.data(), Rf.size() * sizeof(float), hipMemcpyHostToDevice, st), "loco_pca: factor upload") ||
            !pca_ok(p, hipStreamSynchronize(st), "loco_pca: factor upload"))
            return -1;
        pca_product(p, *Y, q, 1, p->small, *other, (int)L, q, q, st);          // Y R^-1
        std::swap(*Y, *other);
    }
    return pca_ok(p, hipGetLastError(), "loco_pca: orthonormalisation launch") ? 0 : -1;
}

// symmetric eigendecomposition of A [q][q] (double, row-major) by cyclic Jacobi: w descending, eigenvectors the columns of E.
// A rotation of the pair (a, b) rotates rows a and b (contiguous), sets their 2 x 2 block from the closed form and mirrors
// the two rows into columns a and b (A stays symmetric); the eigenvectors are kept as rows until the end.
void pca_eig(std::vector<double>& A, int q, std::vector<double>& w, std::vector<double>& E) {
    std::vector<double> Et((size_t)q * q, 0.0);
    for (int i = 0; i < q; ++i) Et[(size_t)i * q + i] = 1.0;
    double scale = 0.0;
    for (int i = 0; i < q; ++i) scale += A[(size_t)i * q + i] * A[(size_t)i * q + i];
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < q; ++i)
            for (int j = i + 1; j < q; ++j) off += A[(size_t)i * q + j] * A[(size_t)i * q + j];
        if (off <= 1e-31 * scale) break;
        for (int a = 0; a < q - 1; ++a)
            for (int b = a + 1; b < q; ++b) {
                const double apq = A[(size_t)a * q + b];
                const double app = A[(size_t)a * q + a], aqq = A[(size_t)b * q + b];
                if (std::fabs(apq) <= 1e-20 * (std::fabs(app) + std::fabs(aqq))) continue;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                double *Ra = &A[(size_t)a * q], *Rb = &A[(size_t)b * q];
                for (int k = 0; k < q; ++k) {
                    const double x = Ra[k], y = Rb[k];
                    Ra[k] = c * x - s * y; Rb[k] = s * x + c * y;
                }
                Ra[a] = app - t * apq; Rb[b] = aqq + t * apq; Ra[b] = 0.0; Rb[a] = 0.0;
                for (int k = 0; k < q; ++k)
                    if (k != a && k != b) { A[(size_t)k * q + a] = Ra[k]; A[(size_t)k * q + b] = Rb[k]; }
                double *Ea = &Et[(size_t)a * q], *Eb = &Et[(size_t)b * q];
                for (int k = 0; k < q; ++k) {
                    const double x = Ea[k], y = Eb[k];
                    Ea[k] = c * x - s * y; Eb[k] = s * x + c * y;
                }
            }
    }
    std::vector<int> order(q);
    for (int i = 0; i < q; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A[(size_t)x * q + x] > A[(size_t)y * q + y]; });
    w.resize(q);
    E.assign((size_t)q * q, 0.0);
    for (int j = 0; j < q; ++j) {
        w[j] = A[(size_t)order[j] * q + order[j]];
        for (int k = 0; k < q; ++k) E[(size_t)k * q + j] = Et[(size_t)order[j] * q + k];
    }
}

std::string pca_bytes(long rows, long d) { return std::to_string((long long)rows * d * 4) + " bytes"; }

int pca_check_q(loco_pca* p, const char* fn, int q) {
    if (q < 1 || q > PCA_Q_LIMIT || q > p->q_max)
        return p->fail(std::string(fn) + ": q = " + std::to_string(q) + " is outside [1, " + std::to_string(std::min(p->q_max, PCA_Q_LIMIT)) +
                       "] (q_max of the handle " + std::to_string(p->q_max) + ", the unit's limit " + std::to_string(PCA_Q_LIMIT) + ")");
    return 0;
}

}  // namespace
}  // namespace loco

using namespace loco;

extern "C" {

int loco_pca_create(int32_t device, int64_t n_max, int64_t d, int32_t q_max, loco_pca** out) {
    struct Cfg { int64_t n_max, d; int32_t q_max; } cfg{n_max, d, q_max};
    return encoder_create<loco_pca>("loco_pca_create", g_pca_create_err, &cfg, device, out,
        [](const Cfg& c) -> std::string {
            if (c.n_max < 2 || c.d < 1) return "need n_max >= 2 rows and d >= 1 columns";
            if (c.n_max > 0x7fffffffL || c.d > 0x7fffffffL) return "n_max and d must fit 31 bits";
            if (c.q_max < 1 || c.q_max > PCA_Q_LIMIT) return "q_max = " + std::to_string(c.q_max) + " is outside [1, " + std::to_string(PCA_Q_LIMIT) + "]";
            return "";
        },
        [&](loco_pca& p) {
            p.n_max = n_max; p.d = d; p.q_max = q_max; p.n = 0;
            const size_t nd = (size_t)n_max * d, nq = (size_t)n_max * q_max, dq = (size_t)d * q_max, qq = (size_t)q_max * q_max;
            return p.alloc({EncoderBase::buf(&p.H, nd), EncoderBase::buf(&p.Hc, nd), EncoderBase::buf(&p.Y0, nq), EncoderBase::buf(&p.Y1, nq),
                            EncoderBase::buf(&p.Z0, dq), EncoderBase::buf(&p.Z1, dq), EncoderBase::buf(&p.small, qq),
                            EncoderBase::buf(&p.split, (size_t)PCA_SPLIT_WS), EncoderBase::buf(&p.meanf, (size_t)d),
                            EncoderBase::buf(&p.mean, (size_t)d), EncoderBase::buf(&p.colpart, (size_t)PCA_MAX_PARTS * d),
                            EncoderBase::buf(&p.G, qq), EncoderBase::buf(&p.gpart, (size_t)PCA_MAX_PARTS * qq)});
        });
}

int loco_pca_reset(loco_pca* p) {
    if (!p) return -2;
    p->n = 0; p->centred_valid = false;
    return 0;
}

int64_t loco_pca_rows(loco_pca* p) { return p ? p->n : -1; }

int loco_pca_add_rows(loco_pca* p, const float* rows_dev, int64_t b, int64_t d, void* stream) {
    if (!p) return -2;
    if (!rows_dev || b < 1) return p->fail("loco_pca_add_rows: need b >= 1 rows");
    if (d != p->d) return p->fail("loco_pca_add_rows: rows of width " + std::to_string(d) + " (" + pca_bytes(1, d) + " each), the store was created for width " +
                                  std::to_string(p->d) + " (" + pca_bytes(1, p->d) + " each)");
    if (p->n + b > p->n_max)
        return p->fail("loco_pca_add_rows: " + std::to_string(p->n) + " + " + std::to_string(b) + " rows need " + pca_bytes(p->n + b, p->d) +
                       ", the store was created for " + std::to_string(p->n_max) + " rows (" + pca_bytes(p->n_max, p->d) + ")");
    DeviceGuard dg(p->device);
    if (!pca_ok(p, hipMemcpyAsync(p->H + p->n * p->d, rows_dev, (size_t)b * d * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream),
                "loco_pca_add_rows: copy"))
        return -1;
    p->n += b;
    p->centred_valid = false;
    return 0;
}

int loco_pca_set_route(loco_pca* p, int32_t route) {
    if (!p) return -2;
    if (route < 0 || route > 2) return p->fail("loco_pca_set_route: 0 (by grid size), 1 (launch_gemm) or 2 (split contraction)");
    p->route = route;
    return 0;
}

const char* loco_pca_routes(loco_pca* p) { return p ? p->routes.c_str() : ""; }

int loco_pca_center(loco_pca* p, int32_t center, float* centered_dev, float* mean_dev, void* stream) {
    if (!p) return -2;
    if (p->n < 1) return p->fail("loco_pca_center: the store is empty");
    DeviceGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    if (pca_centre(p, center, st)) return -1;
    if (centered_dev && !pca_ok(p, hipMemcpyAsync(centered_dev, p->Hc, (size_t)p->n * p->d * sizeof(float), hipMemcpyDeviceToDevice, st), "loco_pca_center: copy"))
        return -1;
    if (mean_dev && !pca_ok(p, hipMemcpyAsync(mean_dev, p->meanf, (size_t)p->d * sizeof(float), hipMemcpyDeviceToDevice, st), "loco_pca_center: copy"))
        return -1;
    return 0;
}

int loco_pca_gram(loco_pca* p, const float* y_dev, int64_t rows, int32_t q, double* g_dev, void* stream) {
    if (!p) return -2;
    if (!y_dev || !g_dev) return p->fail("loco_pca_gram: null argument");
    if (pca_check_q(p, "loco_pca_gram", q)) return -1;
    if (rows < 1 || rows > std::max(p->n_max, p->d))
        return p->fail("loco_pca_gram: " + std::to_string(rows) + " rows, the workspace covers max(n_max, d) = " + std::to_string(std::max(p->n_max, p->d)));
    DeviceGuard dg(p->device);
    pca_gram(p, y_dev, rows, q, g_dev, (hipStream_t)stream);
    return pca_ok(p, hipGetLastError(), "loco_pca_gram: launch") ? 0 : -1;
}

int loco_pca_project(loco_pca* p, const float* w_dev, int32_t q, int32_t transpose, int32_t center, float* out_dev, void* stream) {
    if (!p) return -2;
    if (!w_dev || !out_dev) return p->fail("loco_pca_project: null argument");
    if (pca_check_q(p, "loco_pca_project", q)) return -1;
    if (p->n < 1) return p->fail("loco_pca_project: the store is empty");
    DeviceGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    if (pca_centre(p, center, st)) return -1;
    const char* r = transpose ? pca_product(p, p->Hc, 1, p->d, w_dev, out_dev, (int)p->d, q, (int)p->n, st)
                              : pca_product(p, p->Hc, p->d, 1, w_dev, out_dev, (int)p->n, q, (int)p->d, st);
    p->routes = std::string(transpose ? "HtQ:" : "HW:") + r;
    return pca_ok(p, hipGetLastError(), "loco_pca_project: launch") ? 0 : -1;
}

int loco_pca_fit(loco_pca* p, int32_t q, int32_t niter, const float* omega_dev, int32_t center, float* s_dev, float* v_dev, float* mean_dev,
                 void* stream) {
    if (!p) return -2;
    if (!omega_dev || !s_dev || !v_dev) return p->fail("loco_pca_fit: null argument");
    if (pca_check_q(p, "loco_pca_fit", q)) return -1;
    if (niter < 0) return p->fail("loco_pca_fit: niter must not be negative");
    const long N = p->n, D = p->d;
    const long most = std::min(center ? N - 1 : N, D);
    if (q > most)
        return p->fail("loco_pca_fit: q = " + std::to_string(q) + " exceeds " + (center ? "min(N - 1, D)" : "min(N, D)") + " = " + std::to_string(most) +
                       " for N = " + std::to_string(N) + " rows of width D = " + std::to_string(D) + (center ? " with centring" : " without centring"));
    DeviceGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    if (pca_centre(p, center, st)) return -1;
    float *Y = p->Y0, *Yo = p->Y1, *Z = p->Z0, *Zo = p->Z1;
    const char* r_hw = pca_product(p, p->Hc, D, 1, omega_dev, Y, (int)N, q, (int)D, st);                   // Hc Omega
    if (pca_orth(p, &Y, &Yo, N, q, "Hc Omega", st)) return -1;
    const char* r_htq = nullptr;
    for (int it = 0; it < niter; ++it) {
        r_htq = pca_product(p, p->Hc, 1, D, Y, Z, (int)D, q, (int)N, st);                                 // Hc^T Q
        if (pca_orth(p, &Z, &Zo, D, q, "Hc^T Q", st)) return -1;
        pca_product(p, p->Hc, D, 1, Z, Y, (int)N, q, (int)D, st);                                         // Hc Z
        if (pca_orth(p, &Y, &Yo, N, q, "Hc Z", st)) return -1;
    }
    r_htq = pca_product(p, p->Hc, 1, D, Y, Z, (int)D, q, (int)N, st);                                     // B = Hc^T Q
    p->routes = std::string("HW:") + r_hw + " HtQ:" + r_htq;
    pca_gram(p, Z, D, q, p->G, st);
    std::vector<double> G((size_t)q * q), w, E;
    if (!pca_ok(p, hipMemcpyAsync(G.data(), p->G, G.size() * sizeof(double), hipMemcpyDeviceToHost, st), "loco_pca_fit: Gram read-back") ||
        !pca_ok(p, hipStreamSynchronize(st), "loco_pca_fit: Gram read-back"))
        return -1;
    for (double g : G)
        if (!std::isfinite(g)) return p->fail("loco_pca_fit: the samples are not finite");
    pca_eig(G, q, w, E);
    std::vector<float> Ef((size_t)q * q), sf(q);
    for (int j = 0; j < q; ++j) {
        if (!(w[j] > PCA_PIVOT_FLOOR * w[0])) {
            char m[200];
            std::snprintf(m, sizeof(m), "loco_pca_fit: numerical rank %d is below q = %d (eigenvalue %d of B^T B is %.3g of the largest, floor %.3g)", j, q, j,
                          w[0] > 0.0 ? w[j] / w[0] : 0.0, PCA_PIVOT_FLOOR);
            return p->fail(m);
        }
        const double s = std::sqrt(w[j]);
        sf[j] = (float)s;
        for (int k = 0; k < q; ++k) Ef[(size_t)k * q + j] = (float)(E[(size_t)k * q + j] / s);
    }
    if (!pca_ok(p, hipMemcpyAsync(p->small, Ef.data(), Ef.size() * sizeof(float), hipMemcpyHostToDevice, st), "loco_pca_fit: upload") ||
        !pca_ok(p, hipMemcpyAsync(s_dev, sf.data(), sf.size() * sizeof(float), hipMemcpyHostToDevice, st), "loco_pca_fit: upload") ||
        !pca_ok(p, hipStreamSynchronize(st), "loco_pca_fit: upload"))
        return -1;
    pca_product(p, Z, q, 1, p->small, v_dev, (int)D, q, q, st);                                             // V = B E / s
    hipLaunchKernelGGL(pca_sign_kernel, dim3(q), dim3(256), 0, st, v_dev, D, q);
    if (mean_dev && !pca_ok(p, hipMemcpyAsync(mean_dev, p->meanf, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st), "loco_pca_fit: copy"))
        return -1;
    return pca_ok(p, hipGetLastError(), "loco_pca_fit: launch") ? 0 : -1;
}

const char* loco_pca_last_error(loco_pca* p) { return p ? p->err.c_str() : g_pca_create_err.c_str(); }

void loco_pca_destroy(loco_pca* p) { delete p; }

}  // extern "C"
