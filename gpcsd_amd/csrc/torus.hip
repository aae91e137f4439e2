// Phase-difference torus graph by score matching (gfx950, v_mfma_f64_16x16x4_f64): the conditional phase coupling the reference's
// analyses end with (auditory_lfp/torus_graph_fit.py, neuropixels/fit_torus_graph.py), for all bootstrap replicates of the trials.
//
// Phases x[a][n] of d nodes over N trials as unit phasors; pairs p = (i, j), i < j, in the order of np.triu_indices(d, 1); per trial
// c_p = cos(x_i - x_j), s_p = sin(x_i - x_j), S = (c_0, s_0, c_1, s_1, ..), and the m x d Jacobian D with D[2p][i] = -s_p,
// D[2p][j] = s_p, D[2p + 1][i] = c_p, D[2p + 1][j] = -c_p.  Replicate b with weights w: Gamma = 1/W sum_n w_n D_n D_n^T,
// H = 2/W sum_n w_n S_n, phi = Gamma^-1 H.
//
//   tg_node_gram_kernel   G(a) = 1/W sum_n w_n v_n(a) v_n(a)^T for every node a: v(a) is column a of D at the rows of the pairs
//                         that hold a, (v[2 bi], v[2 bi + 1]) = (re_a im_b - im_a re_b, +-(re_a re_b + im_a im_b)) for the bi-th other
//                         node b (+ for b > a), followed by a constant 1 whose row of G(a) is the weighted mean of v(a) = -+ H / 2.
//                         v is formed from the phasor rows on its way to LDS and never stored; lower tiles only
//   tg_assemble_kernel    Gamma and H as a GATHER from the node blocks: an entry of Gamma has two terms on a pair's 2 x 2 diagonal block,
//                         one where two pairs share a node, and is an exact zero elsewhere
//   tg_dt_phi / tg_resid  r_n = D_n (D_n^T phi) - 2 S_n as an m x N array (inference of replicate 0)
//   tg_chi2_kernel        Sigma_pp = 1/W^2 sum_n w_n z_n z_n^T from rows 2p, 2p + 1 of Z = Gamma^-1 R, chi2 = phi_p^T Sigma_pp^-1 phi_p
//
// Conventions of phase.hip / gemm_f64.hip: 256 threads = four waves of 2 x 2 fragments of 16 x 16, K tiles of 16 with N as the K
// dimension, [o][k] operand tiles with a row stride of BK + 2, double-buffered with one barrier per K tile, the last K tile
// zero-masked in LDS; fragment maps: A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15], C/D lane l reg r holds
// C[(l >> 4) + 4 r][l & 15].  Sums run over n in index order, no atomics: the same call gives the same bits.
#include <algorithm>

#include "kernels.hpp"

namespace gpcsd {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef const volatile double __attribute__((address_space(3))) *lds_frag_ptr;
#define LDS_FRAG(p) (*(lds_frag_ptr)(p))

namespace {
constexpr int NT = 256, BO = 64, BK = 16, LD_OK = BK + 2;
constexpr int RB = TG_REPS_PER_WG;          // replicates that share a workgroup's operand tiles
constexpr int T_ELEMS = BO * LD_OK;
constexpr int PT = BO * BK / NT;
}  // namespace

struct TgGramK {
    const double *ure, *uim;     // phasors; node a's N trials start at off[a]
    const long *off;
    const double *w;             // [nrep][N] or nullptr (all ones)
    const double *W;             // [nrep] row sums
    int d, N, nrep, nv;          // nv = 2 d - 1
    double *G;                   // [rep][a][nv][nv], lower part written
};

// A workgroup owns one 64 x 64 tile on or below the diagonal of G(a) for up to RB replicates: both operand tiles are the
// UNWEIGHTED v (the same for every replicate), a replicate's weights multiply the A fragment on its way from LDS to the multiplier
// (one rounded product per element, as the GEMM core's kscale) -- RB x 4 MFMAs per 4 fragment reads and RB weight reads.
__global__ __launch_bounds__(256) void tg_node_gram_kernel(TgGramK g) {
    __shared__ double lds[2 * (2 * T_ELEMS + RB * BK)];       // per buffer: rows of tile i, rows of tile j, weights [RB][BK]
    constexpr int BUF = 2 * T_ELEMS + RB * BK;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int a = blockIdx.y;
    const int rep0 = blockIdx.z * RB;
    const int nrep = min(RB, g.nrep - rep0);                  // >= 1 by the grid
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const int r0 = ti * BO, c0 = tj * BO;
    const int K = g.N;

    d4 acc[RB][2][2];
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int f = 0; f < 2; ++f) acc[q][i][f] = d4{0.0, 0.0, 0.0, 0.0};

    // slots: (row o + 16 i, k) of both tiles, the 16 k of a row on 16 neighbouring lanes.  kind: 0 = -s, 1 = +c, 2 = -c,
    // 3 = the constant 1, 4 = a row past the end (zero)
    const int kt = tid & 15, o = tid >> 4;
    const long offa = g.off[a];
    long offb[2][PT];
    int kind[2][PT];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int r = (h ? c0 : r0) + o + 16 * i;
            int b = 0, kd = 4;
            if (r < g.nv - 1) {
                const int bi = r >> 1;
                b = bi + (bi >= a);
                kd = (r & 1) ? (b > a ? 1 : 2) : 0;
            } else if (r == g.nv - 1) {
                kd = 3;
            }
            offb[h][i] = g.off[b];
            kind[h][i] = kd;
        }
    double ra_re, ra_im, rb_re[2][PT], rb_im[2][PT], rw = 0.0;
    const int wq = tid >> 4;                                  // tid < RB * 16: weight slot (replicate wq, k = kt)
    auto load = [&](int t) {
        const int n = t * BK + kt < K ? t * BK + kt : K - 1;
        ra_re = g.ure[offa + n];
        ra_im = g.uim[offa + n];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                rb_re[h][i] = g.ure[offb[h][i] + n];
                rb_im[h][i] = g.uim[offb[h][i] + n];
            }
        if (tid < RB * BK) rw = (wq < nrep) ? (g.w ? g.w[(long)(rep0 + wq) * K + n] : 1.0) : 0.0;
    };
    auto store = [&](int buf, int t) {
        const bool ok = kt < K - t * BK;
        double *p = lds + buf * BUF + o * LD_OK + kt;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                // two multiply-adds each: -sin(x_a - x_b) = re_a im_b - im_a re_b, cos(x_a - x_b) = re_a re_b + im_a im_b
                const double ms = fma(ra_re, rb_im[h][i], -(ra_im * rb_re[h][i]));
                const double cs = fma(ra_re, rb_re[h][i], ra_im * rb_im[h][i]);
                const int kd = kind[h][i];
                const double v = kd == 0 ? ms : kd == 1 ? cs : kd == 2 ? -cs : kd == 3 ? 1.0 : 0.0;
                p[h * T_ELEMS + 16 * i * LD_OK] = ok ? v : 0.0;
            }
        if (tid < RB * BK) lds[buf * BUF + 2 * T_ELEMS + wq * BK + kt] = ok ? rw : 0.0;
    };
    auto mma = [&](int buf, int steps) {
        const double *sa = lds + buf * BUF + (wr * 32 + fr) * LD_OK + fq;
        const double *sb = lds + buf * BUF + T_ELEMS + (wc * 32 + fr) * LD_OK + fq;
        const double *sw = lds + buf * BUF + 2 * T_ELEMS + fq;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk < steps) {                      // wave-uniform
                double va[2], vb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    va[i] = LDS_FRAG(sa + i * 16 * LD_OK + kk * 4);
                    vb[i] = LDS_FRAG(sb + i * 16 * LD_OK + kk * 4);
                }
#pragma unroll
                for (int q = 0; q < RB; ++q) {
                    if (q < nrep) {                // block-uniform
                        const double wv = LDS_FRAG(sw + q * BK + kk * 4);
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const double wa = va[i] * wv;
#pragma unroll
                            for (int f = 0; f < 2; ++f) acc[q][i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, vb[f], acc[q][i][f], 0, 0, 0);
                        }
                    }
                }
            }
        }
    };
    const int nk = (K + BK - 1) / BK;
    const int last_steps = (K - (nk - 1) * BK + 3) / 4;
    load(0);
    store(0, 0);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const bool more = t + 1 < nk;              // block-uniform
        if (more) load(t + 1);
        mma(t & 1, more ? BK / 4 : last_steps);
        if (more) store((t + 1) & 1, t + 1);
        __syncthreads();
    }

    // ---- epilogue: entries (r, c) with r >= c
    const long nn = (long)g.nv * g.nv;
#pragma unroll
    for (int q = 0; q < RB; ++q) {
        if (q >= nrep) continue;
        const double Wd = g.W[rep0 + q];
        double *out = g.G + ((long)(rep0 + q) * g.d + a) * nn;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int c = c0 + wc * 32 + f * 16 + fr;
            if (c >= g.nv) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + wr * 32 + i * 16 + fq + 4 * r;
                    if (row >= g.nv || row < c) continue;
                    out[(long)row * g.nv + c] = acc[q][i][f][r] / Wd;
                }
        }
    }
}

// Gamma (m x m, interleaved order 2p, 2p + 1) and H of every replicate of a chunk, gathered from the node blocks.
struct TgAsmK {
    const double *G;
    const int *pi, *pj;          // the pairs
    int d, P, nv, nrep;
    double *Gamma, *H;           // [rep][m][m], [rep][m]
};

__device__ __forceinline__ double tg_glow(const double *Ga, int nv, int a, int b, int al, int b2, int be) {
    int r = 2 * (b - (b > a)) + al, c = 2 * (b2 - (b2 > a)) + be;
    if (r < c) { const int t = r; r = c; c = t; }
    return Ga[(long)r * nv + c];
}

__global__ __launch_bounds__(256) void tg_assemble_kernel(TgAsmK g) {
    const int m = 2 * g.P;
    const int rep = blockIdx.y;
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= (long)m * m) return;
    const int x = (int)(e / m), y = (int)(e % m);
    const int p = x >> 1, al = x & 1, q = y >> 1, be = y & 1;
    const int i = g.pi[p], j = g.pj[p], k = g.pi[q], l = g.pj[q];
    const long nn = (long)g.nv * g.nv;
    const double *G = g.G + (long)rep * g.d * nn;
    double v = 0.0;
    if (p == q) {
        v = tg_glow(G + i * nn, g.nv, i, j, al, j, be) + tg_glow(G + j * nn, g.nv, j, i, al, i, be);
    } else {
        int a = -1, b = 0, b2 = 0;
        if (i == k) { a = i; b = j; b2 = l; }
        else if (i == l) { a = i; b = j; b2 = k; }
        else if (j == k) { a = j; b = i; b2 = l; }
        else if (j == l) { a = j; b = i; b2 = k; }
        if (a >= 0) v = tg_glow(G + a * nn, g.nv, a, b, al, b2, be);
    }
    g.Gamma[(long)rep * m * m + e] = v;
    if (y == 0) {
        // H[2p] = 2 mean c_p = 2 mean v(i)[j, 1], H[2p + 1] = 2 mean s_p = -2 mean v(i)[j, 0]   (i < j: the signs of node i's column)
        const double mean = G[i * nn + (long)(g.nv - 1) * g.nv + 2 * (j - 1) + (al ? 0 : 1)];
        g.H[(long)rep * m + x] = al ? -2.0 * mean : 2.0 * mean;
    }
}

__global__ __launch_bounds__(256) void tg_diag_save_kernel(const double *Gamma, int m, double *dg) {
    const long base = (long)blockIdx.y * m;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) dg[base + i] = Gamma[(long)blockIdx.y * m * m + (long)i * m + i];
}

// After the factorisation: a pivot that is not above TG_PIVOT_TOL m u times the diagonal entry it started from counts as failed (a
// singular Gamma -- fewer trials with weight than parameters need -- leaves pivots of rounding size and either sign: the
// factorisation's own test, pivot <= 0, catches only half of them).  status = the first such pivot + 1, or what potrf reported if
// that came earlier.
__global__ __launch_bounds__(256) void tg_pivot_check_kernel(const double *L, const double *dg, int m, int *status) {
    __shared__ int sh[256];
    const double tol = TG_PIVOT_TOL * m * 1.1102230246251565e-16;
    int first = m + 1;
    for (int i = threadIdx.x; i < m; i += 256) {
        const double l = L[(long)i * m + i];
        if (!(l * l > tol * dg[i]) && i + 1 < first) first = i + 1;
    }
    sh[threadIdx.x] = first;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = min(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] <= m) {
        const int cur = *status;
        *status = cur > 0 ? min(cur, sh[0]) : sh[0];
    }
}

// g[a][n] = (D_n^T phi)[a] = sum over the other nodes b of v(a)[b, 0] phi[p(a, b)][0] + v(a)[b, 1] phi[p(a, b)][1]
struct TgResK {
    const double *ure, *uim;
    const long *off;
    const int *pi, *pj;
    const double *phi;           // [m]
    int d, N, P;
    double *g;                   // [d][N]
    double *R;                   // [m][N]
};

__device__ __forceinline__ int tg_pair_index(int d, int i, int j) {     // i < j, the order of np.triu_indices(d, 1)
    return i * (2 * d - i - 1) / 2 + (j - i - 1);
}

__global__ __launch_bounds__(256) void tg_dt_phi_kernel(TgResK k) {
    const int a = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= k.N) return;
    const double ra = k.ure[k.off[a] + n], ia = k.uim[k.off[a] + n];
    double s = 0.0;
    for (int b = 0; b < k.d; ++b) {
        if (b == a) continue;
        const double rb = k.ure[k.off[b] + n], ib = k.uim[k.off[b] + n];
        const double ms = fma(ra, ib, -(ia * rb));
        const double cs = fma(ra, rb, ia * ib);
        const int p = b > a ? tg_pair_index(k.d, a, b) : tg_pair_index(k.d, b, a);
        s = fma(ms, k.phi[2 * p], s);
        s = fma(b > a ? cs : -cs, k.phi[2 * p + 1], s);
    }
    k.g[(long)a * k.N + n] = s;
}

// r[2p] = s_p (g_j - g_i) - 2 c_p,   r[2p + 1] = c_p (g_i - g_j) - 2 s_p
__global__ __launch_bounds__(256) void tg_resid_kernel(TgResK k) {
    const int p = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= k.N) return;
    const int i = k.pi[p], j = k.pj[p];
    const double ri = k.ure[k.off[i] + n], ii = k.uim[k.off[i] + n], rj = k.ure[k.off[j] + n], ij = k.uim[k.off[j] + n];
    const double cs = fma(ri, rj, ii * ij);
    const double sn = fma(ii, rj, -(ri * ij));
    const double dg = k.g[(long)j * k.N + n] - k.g[(long)i * k.N + n];
    k.R[(long)(2 * p) * k.N + n] = fma(sn, dg, -2.0 * cs);
    k.R[(long)(2 * p + 1) * k.N + n] = fma(-cs, dg, -2.0 * sn);
}

// One workgroup per pair: the three sums of w z z^T over the trials (thread-strided partial sums in index order, then a fixed tree)
// and the 2 x 2 solve.
__global__ __launch_bounds__(256) void tg_chi2_kernel(const double *Z, const double *w, const double *phi, int N, double W, double *chi2) {
    __shared__ double sh[3][256];
    const int p = blockIdx.x;
    const double *z0 = Z + (long)(2 * p) * N, *z1 = z0 + N;
    double s00 = 0.0, s01 = 0.0, s11 = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const double wn = w ? w[n] : 1.0, a = z0[n], b = z1[n];
        s00 = fma(wn * a, a, s00);
        s01 = fma(wn * a, b, s01);
        s11 = fma(wn * b, b, s11);
    }
    sh[0][threadIdx.x] = s00; sh[1][threadIdx.x] = s01; sh[2][threadIdx.x] = s11;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a = sh[0][0], b = sh[1][0], c = sh[2][0];
        const double f0 = phi[2 * p], f1 = phi[2 * p + 1];
        // Sigma_pp = [[a, b], [b, c]] / W^2
        chi2[p] = W * W * (f0 * f0 * c - 2.0 * f0 * f1 * b + f1 * f1 * a) / (a * c - b * b);
    }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
void k_tg_node_gram(gpcsd_ctx *c, const TgDesc &t, const double *w, const double *W, int nrep, double *G, hipStream_t s) {
    GP_REQUIRE(t.d >= 2 && t.d <= TG_MAX_NODES && t.N >= 1 && nrep >= 1, -3, "torus_graph: bad node Gram shape");
    const int nv = 2 * t.d - 1, T = ceil_div(nv, BO);
    ProfScope ps(c, "tg_node_gram", (double)t.d * nrep * nv * (nv + 1.0) * t.N, s);
    TgGramK k;
    k.ure = t.ure; k.uim = t.uim; k.off = t.off; k.w = w; k.W = W;
    k.d = t.d; k.N = t.N; k.nrep = nrep; k.nv = nv;
    k.G = G;
    GP_REQUIRE(ceil_div(nrep, RB) < 65536, GPCSD_ERR_CAPACITY, "torus_graph: too many replicates in one chunk");
    hipLaunchKernelGGL(tg_node_gram_kernel, dim3(T * (T + 1) / 2, t.d, ceil_div(nrep, RB)), dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
}

void k_tg_assemble(gpcsd_ctx *c, const TgDesc &t, const double *G, int nrep, double *Gamma, double *H, hipStream_t s) {
    const int P = t.d * (t.d - 1) / 2, m = 2 * P;
    GP_REQUIRE(nrep >= 1 && nrep < 65536, GPCSD_ERR_CAPACITY, "torus_graph: too many replicates in one chunk");
    ProfScope ps(c, "tg_assemble", 0.0, s);
    TgAsmK k;
    k.G = G; k.pi = t.pi; k.pj = t.pj; k.d = t.d; k.P = P; k.nv = 2 * t.d - 1; k.nrep = nrep;
    k.Gamma = Gamma; k.H = H;
    hipLaunchKernelGGL(tg_assemble_kernel, dim3(ceil_div((long)m * m, 256), nrep), dim3(256), 0, s, k);
    GP_HIP(hipGetLastError());
}

void k_tg_diag_save(gpcsd_ctx *c, const double *Gamma, int m, int nrep, double *dg, hipStream_t s) {
    hipLaunchKernelGGL(tg_diag_save_kernel, dim3(ceil_div(m, 256), nrep), dim3(256), 0, s, Gamma, m, dg);
    GP_HIP(hipGetLastError());
}

void k_tg_pivot_check(gpcsd_ctx *c, const double *L, const double *dg, int m, int *status, hipStream_t s) {
    hipLaunchKernelGGL(tg_pivot_check_kernel, dim3(1), dim3(256), 0, s, L, dg, m, status);
    GP_HIP(hipGetLastError());
}

void k_tg_residuals(gpcsd_ctx *c, const TgDesc &t, const double *phi, double *g, double *R, hipStream_t s) {
    ProfScope ps(c, "tg_residuals", 0.0, s);
    TgResK k;
    k.ure = t.ure; k.uim = t.uim; k.off = t.off; k.pi = t.pi; k.pj = t.pj; k.phi = phi;
    k.d = t.d; k.N = t.N; k.P = t.d * (t.d - 1) / 2; k.g = g; k.R = R;
    hipLaunchKernelGGL(tg_dt_phi_kernel, dim3(ceil_div(t.N, 256), t.d), dim3(256), 0, s, k);
    hipLaunchKernelGGL(tg_resid_kernel, dim3(ceil_div(t.N, 256), k.P), dim3(256), 0, s, k);
    GP_HIP(hipGetLastError());
}

void k_tg_chi2(gpcsd_ctx *c, const double *Z, const double *w, const double *phi, int P, int N, double W, double *chi2, hipStream_t s) {
    hipLaunchKernelGGL(tg_chi2_kernel, dim3(P), dim3(256), 0, s, Z, w, phi, N, W, chi2);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
