// Missing samples (gfx950, v_mfma_f64_16x16x4_f64): the Schur complement G = (A^-1)_MM of a trial's missing set M in the Kronecker
// eigenbasis, A = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T, and the small passes around it (gpcsd_predict_masked, gpcsd_loglik_masked,
// gpcsd_masked_gram; capi_masked.inl).
//
// The m missing samples p = (x_p, i_p) are sorted by time, then electrode; the nu distinct times are the time GROUPS.  With
//   H_a = Qt_u diag(1 / D[a, :]) Qt_u^T  (nu x nu; Qt_u = the rows of Qt at the distinct times; one batched K-scaled GEMM over a)
// the block of G of the groups (g, g') is  Us_g diag_a(H_a[g][g']) Us_g'^T,  Us_g = the rows of Qs at the group's electrodes: a
// product over the nx eigen-indices a whose scale depends on the PAIR of groups.
//
//   masked_gram_kernel    the grouped, K-scaled symmetric product.  The sorted samples are cut into STRIPS of up to 16 samples of one
//                         group (a group of n samples is ceil(n / 16) strips, a scattered sample a strip of its own), so that a 16 x 16
//                         MFMA fragment belongs to exactly one pair of groups and the scale H_a[g][g'] multiplies the A fragment on its
//                         way from LDS to the multiplier (one rounded product per element, as the GEMM core's kscale).  A workgroup owns
//                         4 x 4 strips (a 64 x 64 tile of the padded index space) on or below the diagonal; rows of Qs are gathered
//                         through the sample -> electrode table on their way to LDS (never stored), padding rows are zeros BY SELECTION.
//                         Entries with row >= column are stored together with their mirror images from the same register: G is
//                         symmetric bit for bit.  The sum runs over a in index order, no atomics: the same call gives the same bits.
//   the small passes      zero-fill of the masked-out data by selection (a masked-out value is never an arithmetic operand), the gather
//                         of c = (A^-1 y~)_M, the scatter of u = -G^-1 c, per-trial sums in a fixed order.
//
// Conventions of torus.hip / phase.hip / gemm_f64.hip: 256 threads = four waves of 2 x 2 fragments of 16 x 16, K tiles of 16,
// [o][k] operand tiles with a row stride of BK + 2, double-buffered with one barrier per K tile, the last K tile zero-masked in LDS;
// fragment maps: A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15], C/D lane l reg r holds C[(l >> 4) + 4 r][l & 15].
#include <algorithm>

#include "kernels.hpp"

namespace gpcsd {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef const volatile double __attribute__((address_space(3))) *lds_frag_ptr;
#define LDS_FRAG(p) (*(lds_frag_ptr)(p))

namespace {
constexpr int NT = 256, BO = 64, BK = 16, LD_OK = BK + 2;
constexpr int T_ELEMS = BO * LD_OK;
constexpr int SW = MASKED_STRIP, ST = MASKED_TILE_STRIPS;      // 16 samples per strip, 4 strips per tile side
constexpr int H_ELEMS = ST * ST * BK;
constexpr int BUF = 2 * T_ELEMS + H_ELEMS;
static_assert(SW == 16 && ST == 4 && SW * ST == BO && NT == ST * ST * BK, "one thread per (strip pair, k) scale and per (row, k) operand slot");
}  // namespace

struct MgK {
    const double *Qs;            // (nx, nx) row-major: row x = electrode, column a = eigen-index (the contracted one)
    int nx;
    const int *xi;               // electrode of sorted sample p
    const int *s_off, *s_cnt, *s_grp;      // strips (padded to a multiple of 4 with empty ones): first sample, samples, time group
    const double *H;             // [a][g - gA][g']: rows = the groups of this launch's tile rows, ldh columns
    long sH, ldh;
    int gA;
    int t0;                      // first tile row of this launch
    int m;
    double *G;                   // (m, m)
};

__global__ __launch_bounds__(256) void masked_gram_kernel(MgK g) {
    const int ti = g.t0 + (int)blockIdx.y, tj = (int)blockIdx.x;
    if (tj > ti) return;                                       // block-uniform: lower tiles only
    __shared__ double lds[2 * BUF];
    __shared__ int soff[2][ST], scnt[2][ST];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int K = g.nx;

    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[i][f] = d4{0.0, 0.0, 0.0, 0.0};

    // operand slots: (row o of strip i, k) of both tiles, the 16 k of a row on 16 neighbouring lanes (128 contiguous bytes of Qs)
    const int kt = tid & 15, o = tid >> 4;
    long qoff[2][ST];
    bool qok[2][ST];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int sp = ST * (h ? tj : ti) + i;
            const bool ok = o < g.s_cnt[sp];
            qok[h][i] = ok;
            qoff[h][i] = ok ? (long)g.xi[g.s_off[sp] + o] * g.nx : 0;
        }
    // scale slot: strip pair (hi, hf) of the tile at k = kt; pairs above the diagonal and empty strips read nothing
    const int hi = tid >> 6, hf = (tid >> 4) & 3;
    const int rs = ST * ti + hi, cs = ST * tj + hf;
    const bool hok = rs >= cs && g.s_cnt[rs] > 0 && g.s_cnt[cs] > 0;
    const long hoff = hok ? (long)(g.s_grp[rs] - g.gA) * g.ldh + g.s_grp[cs] : 0;
    if (tid < 2 * ST) {
        const int sp = ST * (tid < ST ? ti : tj) + (tid & 3);
        soff[tid >> 2][tid & 3] = g.s_off[sp];
        scnt[tid >> 2][tid & 3] = g.s_cnt[sp];
    }

    double rq[2][ST], rh = 0.0;
    auto load = [&](int t) {
        const int a = t * BK + kt < K ? t * BK + kt : K - 1;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < ST; ++i) rq[h][i] = g.Qs[qoff[h][i] + a];
        rh = g.H[(long)a * g.sH + hoff];
    };
    auto store = [&](int buf, int t) {
        const bool ok = kt < K - t * BK;
        double *p = lds + buf * BUF + o * LD_OK + kt;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < ST; ++i) p[h * T_ELEMS + SW * i * LD_OK] = (ok && qok[h][i]) ? rq[h][i] : 0.0;
        lds[buf * BUF + 2 * T_ELEMS + (tid >> 4) * BK + kt] = (ok && hok) ? rh : 0.0;
    };
    auto mma = [&](int buf, int steps) {
        const double *sa = lds + buf * BUF + (wr * 32 + fr) * LD_OK + fq;
        const double *sb = lds + buf * BUF + T_ELEMS + (wc * 32 + fr) * LD_OK + fq;
        const double *sh = lds + buf * BUF + 2 * T_ELEMS + ((2 * wr) * ST + 2 * wc) * BK + fq;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk < steps) {                      // wave-uniform
                double va[2], vb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    va[i] = LDS_FRAG(sa + i * SW * LD_OK + kk * 4);
                    vb[i] = LDS_FRAG(sb + i * SW * LD_OK + kk * 4);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        const double hv = LDS_FRAG(sh + (i * ST + f) * BK + kk * 4);
                        acc[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[i] * hv, vb[f], acc[i][f], 0, 0, 0);
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

    // ---- epilogue: entries with row >= column and their mirror images, from the same register
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int sc = 2 * wc + f;
        if (fr >= scnt[1][sc]) continue;
        const long pc = soff[1][sc] + fr;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int sr = 2 * wr + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ro = fq + 4 * r;
                if (ro >= scnt[0][sr]) continue;
                const long pr = soff[0][sr] + ro;
                if (pr < pc) continue;
                const double v = acc[i][f][r];
                g.G[pr * g.m + pc] = v;
                if (pr > pc) g.G[pc * g.m + pr] = v;
            }
        }
    }
}

void k_masked_gram(gpcsd_ctx *c, const MaskedGramDesc &d, hipStream_t s) {
    GP_REQUIRE(d.m > 0 && d.nx > 0 && d.t1 > d.t0 && d.t0 >= 0 && d.Qs && d.xi && d.s_off && d.s_cnt && d.s_grp && d.H && d.G, -3,
               "masked_gram: bad problem");
    ProfScope ps(c, "masked_gram", 2.0 * BO * BO * (double)d.nx * (d.t1 - d.t0) * (d.t0 + d.t1 + 1) / 2.0, s);
    MgK k;
    k.Qs = d.Qs; k.nx = d.nx; k.xi = d.xi; k.s_off = d.s_off; k.s_cnt = d.s_cnt; k.s_grp = d.s_grp;
    k.H = d.H; k.sH = d.sH; k.ldh = d.ldh; k.gA = d.gA; k.t0 = d.t0; k.m = d.m; k.G = d.G;
    hipLaunchKernelGGL(masked_gram_kernel, dim3(d.t1, d.t1 - d.t0), dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ the small passes
// out[j][b] = Q[rows[j]][b]
__global__ __launch_bounds__(256) void gather_rows_kernel(const double *__restrict__ Q, int n, const int *__restrict__ rows, int nr,
                                                          double *__restrict__ out) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)nr * n) return;
    const int j = (int)(i / n), b = (int)(i - (long)j * n);
    out[i] = Q[(long)rows[j] * n + b];
}
void k_gather_rows(gpcsd_ctx *c, const double *Q, int n, const int *rows, int nr, double *out, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div((long)nr * n, 256)), dim3(256), 0, s, Q, n, rows, nr, out);
    GP_HIP(hipGetLastError());
}

// out[x][r][t] = mask[x][t][r (or 0)] ? y[x][r][t] : 0 -- a selection: the masked-out value is not an operand
__global__ __launch_bounds__(256) void mask_fill_kernel(const double *__restrict__ y, const unsigned char *__restrict__ mask, int MT, int nx,
                                                        int R, int nt, double *__restrict__ out) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)nx * R * nt) return;
    const int t = (int)(i % nt);
    const long xr = i / nt;
    const int r = (int)(xr % R), x = (int)(xr / R);
    const bool on = mask[((long)x * nt + t) * MT + (MT > 1 ? r : 0)] != 0;
    out[i] = on ? y[i] : 0.0;
}
void k_mask_fill(gpcsd_ctx *c, const double *y, const unsigned char *mask, int MT, int nx, int R, int nt, double *out, hipStream_t s) {
    hipLaunchKernelGGL(mask_fill_kernel, dim3(ceil_div((long)nx * R * nt, 256)), dim3(256), 0, s, y, mask, MT, nx, R, nt, out);
    GP_HIP(hipGetLastError());
}

// out[r] = sum over the observed samples of trial r of y V, both [x][r][t]; one workgroup per trial, a fixed order
__global__ __launch_bounds__(256) void mask_dot_kernel(const double *__restrict__ y, const double *__restrict__ V,
                                                       const unsigned char *__restrict__ mask, int MT, int nx, int R, int nt,
                                                       double *__restrict__ out) {
    __shared__ double sh[256];
    const int r = blockIdx.x;
    double acc = 0.0;
    for (long i = threadIdx.x; i < (long)nx * nt; i += 256) {
        const int x = (int)(i / nt), t = (int)(i - (long)x * nt);
        const long at = ((long)x * R + r) * nt + t;
        if (mask[((long)x * nt + t) * MT + (MT > 1 ? r : 0)] != 0) acc += y[at] * V[at];
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[r] = sh[0];
}
void k_mask_dot(gpcsd_ctx *c, const double *y, const double *V, const unsigned char *mask, int MT, int nx, int R, int nt, double *out,
                hipStream_t s) {
    hipLaunchKernelGGL(mask_dot_kernel, dim3(R), dim3(256), 0, s, y, V, mask, MT, nx, R, nt, out);
    GP_HIP(hipGetLastError());
}

// C[p][k] = V[xi[p]][trial[k]][ti[p]], V as [x][r][t]
__global__ __launch_bounds__(256) void mask_gather_kernel(const double *__restrict__ V, const int *__restrict__ xi, const int *__restrict__ ti,
                                                          int m, const int *__restrict__ trial, int nr, int R, int nt,
                                                          double *__restrict__ C) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)m * nr) return;
    const int p = (int)(i / nr), k = (int)(i - (long)p * nr);
    C[i] = V[((long)xi[p] * R + trial[k]) * nt + ti[p]];
}
void k_mask_gather(gpcsd_ctx *c, const double *V, const int *xi, const int *ti, int m, const int *trial, int nr, int R, int nt, double *C,
                   hipStream_t s) {
    hipLaunchKernelGGL(mask_gather_kernel, dim3(ceil_div((long)m * nr, 256)), dim3(256), 0, s, V, xi, ti, m, trial, nr, R, nt, C);
    GP_HIP(hipGetLastError());
}

// U[xi[p]][slot[k]][ti[p]] = -X[p][k], U as [x][q][t] with na slots
__global__ __launch_bounds__(256) void mask_scatter_kernel(const double *__restrict__ X, const int *__restrict__ xi, const int *__restrict__ ti,
                                                           int m, const int *__restrict__ slot, int nr, int na, int nt,
                                                           double *__restrict__ U) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)m * nr) return;
    const int p = (int)(i / nr), k = (int)(i - (long)p * nr);
    U[((long)xi[p] * na + slot[k]) * nt + ti[p]] = -X[i];
}
void k_mask_scatter(gpcsd_ctx *c, const double *X, const int *xi, const int *ti, int m, const int *slot, int nr, int na, int nt, double *U,
                    hipStream_t s) {
    hipLaunchKernelGGL(mask_scatter_kernel, dim3(ceil_div((long)m * nr, 256)), dim3(256), 0, s, X, xi, ti, m, slot, nr, na, nt, U);
    GP_HIP(hipGetLastError());
}

// out[trial[k]] = sum_p Z[p][k]^2; one workgroup per column, a fixed order
__global__ __launch_bounds__(256) void mask_colsumsq_kernel(const double *__restrict__ Z, int m, int nr, const int *__restrict__ trial,
                                                            double *__restrict__ out) {
    __shared__ double sh[256];
    const int k = blockIdx.x;
    double acc = 0.0;
    for (int p = threadIdx.x; p < m; p += 256) {
        const double z = Z[(long)p * nr + k];
        acc += z * z;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[trial[k]] = sh[0];
}
void k_mask_colsumsq(gpcsd_ctx *c, const double *Z, int m, int nr, const int *trial, double *out, hipStream_t s) {
    hipLaunchKernelGGL(mask_colsumsq_kernel, dim3(nr), dim3(256), 0, s, Z, m, nr, trial, out);
    GP_HIP(hipGetLastError());
}

// B[x'][trial[q]][i] += B2[x'][q][i], q < na
__global__ __launch_bounds__(256) void mask_add_kernel(double *__restrict__ B, const double *__restrict__ B2, const int *__restrict__ trial,
                                                       int nx, int R, int na, int nt) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)nx * na * nt) return;
    const int t = (int)(i % nt);
    const long xq = i / nt;
    const int q = (int)(xq % na), x = (int)(xq / na);
    B[((long)x * R + trial[q]) * nt + t] += B2[i];
}
void k_mask_add(gpcsd_ctx *c, double *B, const double *B2, const int *trial, int nx, int R, int na, int nt, hipStream_t s) {
    hipLaunchKernelGGL(mask_add_kernel, dim3(ceil_div((long)nx * na * nt, 256)), dim3(256), 0, s, B, B2, trial, nx, R, na, nt);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
