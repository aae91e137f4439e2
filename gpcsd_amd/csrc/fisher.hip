// Hyper-parameter uncertainty (gpcsd_fisher / gpcsd_trial_scores; capi_fisher.inl queues them), gfx950.
//
// In the eigen-basis Qs (x) Qt of K = Ks (x) Kt + sig2n I every derivative direction is Kronecker-structured:
//   spatial p   dK -> Ahat_p (x) Lambda_t     Ahat_p = Qs^T dKs/dp Qs
//   temporal q  dK -> Lambda_s (x) Bhat_q     Bhat_q = Qt^T dKt/dq Qt
//   noise       dK -> I
// and with U = 1 / D, B_r = (Qs^T Y_r Qt) / D the per-trial score and the expected information of one trial are sums over
// (x, i) of products of these with B_r and U.  This file holds
//
//   score_kernel         the fp64 MFMA product that stores no C: the epilogue multiplies each accumulator by the matching entry of
//                        B and by et[col % nt] (spatial: Ahat_p B, B as nx x (R nt)) or es[row / R] (temporal: B Bhat_q, B as
//                        (nx R) x nt) and leaves the sums over the tile's rows (columns) as one partial per column (row) and tile
//   score_reduce_kernel  one workgroup per (parameter, trial): the partials of that trial's columns (rows) in tile order
//   pair_kernel          <X_a o X_b, W> for all pairs a <= b of a stack of matrices (W = M or N), per-block partials + fixed sum
//   diag_kernel          the diagonal-weighted sums over U and U^2 (traces of the scores, cross and noise blocks), the same two stages
//   builders             dA/dR as a matrix, dKt / d(ell_c, sigma2_c) as matrices, and the small vectors around them
//
// No atomics anywhere, and no sum depends on the number of resident trials: a partial belongs to one column (row) of one tile, a
// trial's columns sit at the same place in the same tiles whatever follows them, and the second stage walks them in index order.
// So the same call returns the same bits, and a trial's scores do not depend on which other trials are resident beside it.
//
// Tile conventions of fungram.hip / masked.hip: 256 threads = four waves of 2 x 2 fragments of 16 x 16 (v_mfma_f64_16x16x4_f64),
// K tiles of 16, [o][k] operand tiles with a row stride of BK + 1, the next tile's global loads in flight under the current
// tile's MFMAs.  Edges: a row (column) past the end reads the last valid one -- its products are dropped in the epilogue --, an
// index past K is zeroed on its way to LDS.  Fragment maps: A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15],
// C/D lane l reg r holds C[(l >> 4) + 4 r][l & 15].
#include <algorithm>

#include "devutil.hpp"
#include "kernels.hpp"
#include "temporal_kernel.hpp"

namespace gpcsd {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef const volatile double __attribute__((address_space(3))) *lds_frag_ptr;
#define LDS_FRAG(p) (*(lds_frag_ptr)(p))

namespace {
constexpr int NT = 256, BO = 64, BK = 16, LDK = BK + 1;
constexpr int T_ELEMS = BO * LDK;
constexpr int PER = BO * BK / NT;          // 4 elements per thread and operand tile
constexpr int PAIR_BLOCKS = 64;            // partials per pair of pair_kernel (fixed: the sum's association never changes)

struct ScoreK {
    const double *A;             // (M, K) row-major per batch entry, sA apart
    long lda, sA;
    const double *B;             // (K, N) row-major per batch entry, sB apart
    long ldb, sB;
    const double *E;             // (M, N) row-major: the epilogue's factor
    long lde;
    const double *w;             // trial_in_col: w[col % nt], else w[row / R]
    int M, N, K;
    int trial_in_col, nt, R;
    int tiles_m, tiles_n;
    double *part;                // trial_in_col: [batch][tiles_m][N], else [batch][tiles_n][M]
};
}  // namespace

__global__ __launch_bounds__(256) void score_kernel(ScoreK g) {
    __shared__ double lds[2 * T_ELEMS];
    double *const lA = lds, *const lB = lds + T_ELEMS;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int tm = blockIdx.x / g.tiles_n, tn = blockIdx.x % g.tiles_n;
    const int batch = blockIdx.y;
    const int K = g.K, nkt = (K + BK - 1) / BK;

    // A tile: row ar, k = ak .. ak + 3 (contiguous in memory); B tile: k = bk, columns bn .. bn + 3 (contiguous in memory)
    const int ar = tid >> 2, ak = (tid & 3) * PER;
    const int bk = tid >> 4, bn = (tid & 15) * PER;
    const double *const baseA = g.A + batch * g.sA + (long)min(tm * BO + ar, g.M - 1) * g.lda;
    const double *const baseB = g.B + batch * g.sB;
    long colB[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) colB[i] = min(tn * BO + bn + i, g.N - 1);

    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

    double ra[PER], rb[PER];
    auto load = [&](int t) {
        const int k0 = t * BK;
#pragma unroll
        for (int i = 0; i < PER; ++i) ra[i] = baseA[min(k0 + ak + i, K - 1)];
        const double *pb = baseB + (long)min(k0 + bk, K - 1) * g.ldb;
#pragma unroll
        for (int i = 0; i < PER; ++i) rb[i] = pb[colB[i]];
    };
    auto store = [&](int t) {
        const int k0 = t * BK;
#pragma unroll
        for (int i = 0; i < PER; ++i) lA[ar * LDK + ak + i] = (k0 + ak + i < K) ? ra[i] : 0.0;
        const bool in = k0 + bk < K;
#pragma unroll
        for (int i = 0; i < PER; ++i) lB[(bn + i) * LDK + bk] = in ? rb[i] : 0.0;
    };
    const double *const srA = lA + (wr * 32 + fr) * LDK + fq;
    const double *const srB = lB + (wc * 32 + fr) * LDK + fq;

    load(0);
    for (int t = 0; t < nkt; ++t) {
        store(t);
        __syncthreads();
        if (t + 1 < nkt) load(t + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = LDS_FRAG(srA + i * 16 * LDK + ks * 4);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = LDS_FRAG(srB + j * 16 * LDK + ks * 4);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: v = acc * E * w, zero outside the matrix (the operand tiles are free: the loop ended with a barrier)
    double v[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int row = tm * BO + wr * 32 + i * 16 + fq + 4 * r4;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = tn * BO + wc * 32 + j * 16 + fr;
                double x = 0.0;
                if (row < g.M && col < g.N) {
                    const double wgt = g.trial_in_col ? g.w[col % g.nt] : g.w[row / g.R];
                    x = (acc[i][j][r4] * g.E[(long)row * g.lde + col]) * wgt;
                }
                v[i][j][r4] = x;
            }
        }
    double *const red = lds;
    if (g.trial_in_col) {
        // column sums over the tile's 64 rows: a lane's eight rows in order, then [wr][fq] in order -> red[(wr * 4 + fq)][col]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) s += v[i][j][r4];
            red[(wr * 4 + fq) * BO + wc * 32 + j * 16 + fr] = s;
        }
        __syncthreads();
        if (tid < BO) {
            const int col = tn * BO + tid;
            double s = red[tid];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += red[k * BO + tid];
            if (col < g.N) g.part[((long)batch * g.tiles_m + tm) * g.N + col] = s;
        }
    } else {
        // row sums over the tile's 64 columns: a lane's two columns, then [wc][fr] in order -> red[row][wc * 16 + fr]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                red[(wr * 32 + i * 16 + fq + 4 * r4) * 32 + wc * 16 + fr] = v[i][0][r4] + v[i][1][r4];
        __syncthreads();
        if (tid < BO) {
            const int row = tm * BO + tid;
            double s = red[tid * 32];
#pragma unroll
            for (int k = 1; k < 32; ++k) s += red[tid * 32 + k];
            if (row < g.M) g.part[((long)batch * g.tiles_n + tn) * g.M + row] = s;
        }
    }
}

// quad[batch][r] = the partials of trial r: trial_in_col: sum over tile rows tm and i < nt of part[batch][tm][r nt + i];
// else sum over tile columns tn and x < nx of part[batch][tn][x R + r].  One workgroup per (trial, batch); a thread walks its
// elements in index order, the workgroup's sum has a fixed association.
__global__ __launch_bounds__(256) void score_reduce_kernel(const double *__restrict__ part, int trial_in_col, int tiles, long len,
                                                           int n, int R, double *__restrict__ quad) {
    __shared__ double red[4];
    const int r = blockIdx.x, batch = blockIdx.y;
    const double *p = part + (long)batch * tiles * len;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t)
        for (int k = threadIdx.x; k < n; k += 256) s += p[(long)t * len + (trial_in_col ? (long)r * n + k : (long)k * R + r)];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) quad[(long)batch * R + r] = s;
}

void k_fisher_score(gpcsd_ctx *c, const FisherScoreDesc &d, hipStream_t s) {
    GP_REQUIRE(d.A && d.B && d.E && d.w && d.quad && d.M > 0 && d.N > 0 && d.K > 0 && d.batch > 0 && d.R > 0 && d.nt > 0, -3,
               "fisher_score: bad problem");
    GP_REQUIRE(d.trial_in_col ? d.N == (long)d.R * d.nt : d.M % d.R == 0, -3, "fisher_score: the shape does not hold R trials");
    ScoreK k;
    k.A = d.A; k.lda = d.lda; k.sA = d.sA; k.B = d.B; k.ldb = d.ldb; k.sB = d.sB; k.E = d.E; k.lde = d.lde; k.w = d.w;
    k.M = d.M; k.N = d.N; k.K = d.K; k.trial_in_col = d.trial_in_col ? 1 : 0; k.nt = d.nt; k.R = d.R;
    k.tiles_m = ceil_div(d.M, BO); k.tiles_n = ceil_div(d.N, BO);
    const long tiles = (long)k.tiles_m * k.tiles_n;
    GP_REQUIRE(tiles < (1L << 31) && d.batch <= 65535, GPCSD_ERR_CAPACITY, "fisher_score: %ld tiles x %d products exceed one launch",
               tiles, d.batch);
    const int ptiles = d.trial_in_col ? k.tiles_m : k.tiles_n;
    const long plen = d.trial_in_col ? d.N : d.M;
    k.part = c->buf<double>(d.trial_in_col ? "fisher_part_s" : "fisher_part_t", (size_t)d.batch * ptiles * plen);
    ProfScope ps(c, d.prof_name, 2.0 * (double)d.M * d.N * d.K * d.batch, s);
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)tiles, (unsigned)d.batch), dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
    const int n = d.trial_in_col ? d.nt : d.M / d.R;
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)d.R, (unsigned)d.batch), dim3(256), 0, s, (const double *)k.part,
                       k.trial_in_col, ptiles, plen, n, d.R, d.quad);
    GP_HIP(hipGetLastError());
}

// quad[r] = sum_{x,i} B[x][r][i]^2: the noise direction's quadratic part (one workgroup per trial, fixed order)
__global__ __launch_bounds__(256) void trial_sumsq_kernel(const double *__restrict__ B, int nx, int R, int nt, double *__restrict__ quad) {
    __shared__ double red[4];
    const int r = blockIdx.x;
    double s = 0.0;
    for (long e = threadIdx.x; e < (long)nx * nt; e += 256) {
        const double b = B[((e / nt) * R + r) * nt + e % nt];
        s += b * b;
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) quad[r] = s;
}
void k_fisher_trial_sumsq(gpcsd_ctx *c, const double *B, int nx, int R, int nt, double *quad, hipStream_t s) {
    hipLaunchKernelGGL(trial_sumsq_kernel, dim3(R), dim3(256), 0, s, B, nx, R, nt, quad);
    GP_HIP(hipGetLastError());
}

// scores[r][i] = 1/2 quad[i][r] - 1/2 trace[i]
__global__ __launch_bounds__(256) void scores_kernel(const double *__restrict__ quad, const double *__restrict__ trace, int R, int ng,
                                                     double *__restrict__ scores) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)R * ng) return;
    const int r = (int)(e / ng), i = (int)(e % ng);
    scores[e] = 0.5 * quad[(long)i * R + r] - 0.5 * trace[i];
}
void k_fisher_scores(gpcsd_ctx *c, const double *quad, const double *trace, int R, int ng, double *scores, hipStream_t s) {
    hipLaunchKernelGGL(scores_kernel, dim3((unsigned)ceil_div((long)R * ng, 256)), dim3(256), 0, s, quad, trace, R, ng, scores);
    GP_HIP(hipGetLastError());
}

// ---- <X_a o X_b, W> for all pairs a <= b of nm matrices of n2 elements: partials [pair][PAIR_BLOCKS], then their sum in order.
// The product X_a X_b commutes bit for bit, and only a <= b is formed: the caller mirrors it.
__global__ __launch_bounds__(256) void pair_kernel(const double *__restrict__ X, const double *__restrict__ W, long n2, int nm,
                                                   double *__restrict__ part) {
    __shared__ double red[4];
    int a = 0, rest = blockIdx.y;                     // pair index -> (a, b), rows of the upper triangle: a = 0: b = 0 .. nm - 1, ...
    while (rest >= nm - a) {
        rest -= nm - a;
        ++a;
    }
    const int b = a + rest;
    const double *xa = X + (long)a * n2, *xb = X + (long)b * n2;
    double s = 0.0;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n2; e += (long)PAIR_BLOCKS * 256) s += (xa[e] * xb[e]) * W[e];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[(long)blockIdx.y * PAIR_BLOCKS + blockIdx.x] = s;
}
__global__ __launch_bounds__(64) void pair_sum_kernel(const double *__restrict__ part, double *__restrict__ out) {
    const double v = part[(long)blockIdx.x * PAIR_BLOCKS + threadIdx.x];
    const double s = wave_sum(v);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}
void k_fisher_pairs(gpcsd_ctx *c, const double *X, const double *W, long n2, int nm, double *out, hipStream_t s) {
    static_assert(PAIR_BLOCKS == 64, "pair_sum_kernel adds one wave of partials");
    GP_REQUIRE(X && W && out && nm >= 1 && n2 > 0, -3, "fisher_pairs: bad problem");
    const int npair = nm * (nm + 1) / 2;
    double *part = c->buf<double>("fisher_pair_part", (size_t)npair * PAIR_BLOCKS);
    ProfScope ps(c, "fisher_pairs", 3.0 * (double)n2 * npair, s);
    hipLaunchKernelGGL(pair_kernel, dim3(PAIR_BLOCKS, (unsigned)npair), dim3(256), 0, s, X, W, n2, nm, part);
    hipLaunchKernelGGL(pair_sum_kernel, dim3((unsigned)npair), dim3(64), 0, s, (const double *)part, out);
    GP_HIP(hipGetLastError());
}

// ---- the diagonal-weighted sums.  Direction i has the diagonal sv[i][x] tv[i][t] in the eigen-basis; with U = Dinv
//   out[i]                 = sum_{x,t} sv_i[x] tv_i[t] U[x][t]                              i < ng   (the trace parts of the scores)
//   out[ng + pair(i <= j)] = sum_{x,t} (sv_i[x] sv_j[x]) (tv_i[t] tv_j[t]) U[x][t]^2        (cross and noise blocks of the information)
// PAIR_BLOCKS workgroups per output, each over a fixed slice of the elements; their partials are added in order by pair_sum_kernel.
__global__ __launch_bounds__(256) void diag_kernel(const double *__restrict__ sv, const double *__restrict__ tv,
                                                   const double *__restrict__ U, int nx, int nt, int ng, double *__restrict__ part) {
    __shared__ double red[4];
    const int o = blockIdx.y;
    const long n = (long)nx * nt, step = (long)PAIR_BLOCKS * 256;
    double s = 0.0;
    if (o < ng) {
        const double *a = sv + (long)o * nx, *b = tv + (long)o * nt;
        for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += step) s += (a[e / nt] * b[e % nt]) * U[e];
    } else {
        int i = 0, rest = o - ng;
        while (rest >= ng - i) {
            rest -= ng - i;
            ++i;
        }
        const int j = i + rest;
        const double *a = sv + (long)i * nx, *a2 = sv + (long)j * nx, *b = tv + (long)i * nt, *b2 = tv + (long)j * nt;
        for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += step) {
            const double u = U[e];
            s += ((a[e / nt] * a2[e / nt]) * (b[e % nt] * b2[e % nt])) * (u * u);
        }
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[(long)o * PAIR_BLOCKS + blockIdx.x] = s;
}
void k_fisher_diag(gpcsd_ctx *c, const double *sv, const double *tv, const double *U, int nx, int nt, int ng, double *out,
                   hipStream_t s) {
    const int nout = ng + ng * (ng + 1) / 2;
    double *part = c->buf<double>("fisher_diag_part", (size_t)nout * PAIR_BLOCKS);
    ProfScope ps(c, "fisher_diag", 0.0, s);
    hipLaunchKernelGGL(diag_kernel, dim3(PAIR_BLOCKS, (unsigned)nout), dim3(256), 0, s, sv, tv, U, nx, nt, ng, part);
    hipLaunchKernelGGL(pair_sum_kernel, dim3((unsigned)nout), dim3(64), 0, s, (const double *)part, out);
    GP_HIP(hipGetLastError());
}

// sv (ng, nx), tv (ng, nt): spatial p < nsp: (diag Ahat_p, et); temporal q < ntp: (es, diag Bhat_q); noise: (1, 1).
// es2 = es^2 and et2 = et^2 (the K scales of N and M) ride along.
__global__ __launch_bounds__(256) void weights_kernel(const double *__restrict__ Ah, const double *__restrict__ Bh,
                                                      const double *__restrict__ es, const double *__restrict__ et, int nx, int nt,
                                                      int nsp, int ntp, double *__restrict__ sv, double *__restrict__ tv,
                                                      double *__restrict__ es2, double *__restrict__ et2) {
    const int i = blockIdx.y;                         // direction, or nsp + ntp + 1: the squares
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (i == nsp + ntp + 1) {
        if (k < nx) es2[k] = es[k] * es[k];
        if (k < nt) et2[k] = et[k] * et[k];
        return;
    }
    if (k < nx) sv[(long)i * nx + k] = i < nsp ? Ah[(long)i * nx * nx + (long)k * nx + k] : (i < nsp + ntp ? es[k] : 1.0);
    if (k < nt)
        tv[(long)i * nt + k] = i < nsp ? et[k] : (i < nsp + ntp ? Bh[(long)(i - nsp) * nt * nt + (long)k * nt + k] : 1.0);
}
void k_fisher_weights(gpcsd_ctx *c, const double *Ah, const double *Bh, const double *es, const double *et, int nx, int nt, int nsp,
                      int ntp, double *sv, double *tv, double *es2, double *et2, hipStream_t s) {
    hipLaunchKernelGGL(weights_kernel, dim3((unsigned)ceil_div(std::max(nx, nt), 256), (unsigned)(nsp + ntp + 2)), dim3(256), 0, s, Ah,
                       Bh, es, et, nx, nt, nsp, ntp, sv, tv, es2, et2);
    GP_HIP(hipGetLastError());
}

// ---- builders.  dA/dR (nx, G) with the expressions of fwdR_grad_kernel (grad.hip):
//   1D: A = w_g (sqrt(q+1) - sqrt(q)), q = (r/R)^2   ->  dA/dR = w_g (sqrt(q) - q / sqrt(q+1)) / R
//   2D: A = w_g (log(R+eps+sqrt((R+eps)^2+w^2)) - ...)  ->  dA/dR = w_g / sqrt((R+eps)^2 + w^2)
__global__ __launch_bounds__(256) void dA_dR_kernel(const double *__restrict__ x, int nx, const double *__restrict__ gx1,
                                                    const double *__restrict__ gw1, const double *__restrict__ gx2,
                                                    const double *__restrict__ gw2, int G, int ngl2, double R, double eps,
                                                    double *__restrict__ out) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= (long)nx * G) return;
    const int i = (int)(e / G), g = (int)(e % G);
    double dA;
    if (ngl2 > 0) {
        const int g1 = g / ngl2, g2 = g % ngl2;
        const double d1 = gx1[g1] - x[2 * i], d2 = gx2[g2] - x[2 * i + 1];
        const double re = R + eps;
        dA = (gw1[g1] * gw2[g2]) / sqrt(re * re + (d1 * d1 + d2 * d2));
    } else {
        const double r = gx1[g] - x[i];
        const double q = (r / R) * (r / R);
        dA = gw1[g] * (sqrt(q) - q / sqrt(q + 1.0)) / R;
    }
    out[e] = dA;
}
void k_fisher_dA_dR(gpcsd_ctx *c, const double *x, int nx, const double *gx1, const double *gw1, const double *gx2, const double *gw2,
                    int G, int ngl2, double R, double eps, double *out, hipStream_t s) {
    hipLaunchKernelGGL(dA_dR_kernel, dim3((unsigned)ceil_div((long)nx * G, 256)), dim3(256), 0, s, x, nx, gx1, gw1, gx2, gw2, G, ngl2, R,
                       eps, out);
    GP_HIP(hipGetLastError());
}

// out[2c] = dKt / d ell_c, out[2c + 1] = dKt / d sigma2_c = k_c, (nt, nt) each, with the expressions of temporal_grad_kernel
__global__ __launch_bounds__(256) void temporal_dgram_kernel(TemporalSet p, const double *__restrict__ t, int nt, double *__restrict__ out) {
    const long e = blockIdx.x * 256L + threadIdx.x, n2 = (long)nt * nt;
    if (e >= n2) return;
    const int cc = blockIdx.y;
    const double d = t[e / nt] - t[e % nt];
    const double ell = p.ell[cc];
    double k, dk;                                     // unit-variance kernel and its ell-derivative (temporal_kernel.hpp)
    temporal_kernel_value_dell<double>(p.kind[cc], d, ell, k, dk);
    out[(2L * cc) * n2 + e] = p.sigma2[cc] * dk;
    out[(2L * cc + 1) * n2 + e] = k;
}
void k_fisher_temporal_dgram(gpcsd_ctx *c, const TemporalSet &set, const double *t, int nt, double *out, hipStream_t s) {
    hipLaunchKernelGGL(temporal_dgram_kernel, dim3((unsigned)ceil_div((long)nt * nt, 256), (unsigned)set.ncomp), dim3(256), 0, s, set, t,
                       nt, out);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
