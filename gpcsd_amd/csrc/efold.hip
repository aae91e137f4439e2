// Leave-electrodes-out cross-validation in the temporal eigen-basis (gpcsd_cv_electrodes, gpcsd_efold_contract; no reference
// counterpart): factor and solve of the f x f blocks G_j = (K^-1)_FF at temporal eigen-index j of every held-out electrode set F.
//
// Inputs, all contiguous in j:  Gp[row0(F) + i (i + 1) / 2 + k][j] = G_j[i][k], k <= i  (the packed lower triangles, one product of
// gemm_var's pair form),  V[(x, r)][j] = (K^-1 y_r)[x] in the temporal eigen-basis.  efold_kernel: one wave per (fold, chunk of
// EFOLD_CHUNK = 64 eigen-indices), a lane per j, so every load and store of a wave is 512 contiguous bytes.  Per lane
//   G_j = L L^T (a non-positive or non-finite pivot marks the lane bad and sets status[fold] = 1; nothing is addressed by data, so
//   a bad block can neither fault nor hang -- its outputs are NaN),  log det G_j = sum_i log(pivot_i),
//   pdiag[a_i][j] = (G_j^-1)[i][i] = sum_{k >= i} (L^-1)[k][i]^2   by forward substitution of the unit vector e_i,
//   per trial r:  u = V[F][(r, j)],  L z = u,  L^T e = z,  q = sum_i u_i e_i,  e_i^2,  E[(a_i, r)][j] = e_i when the mean is wanted.
// The factor lives in registers for f <= 8 (1, 3, 10, 36 doubles: kernels of 1, 2, 4 and 8 rows, fully unrolled, rows past f
// skipped on a wave-uniform test) and in LDS above that ([element][lane], 136 + 16 doubles per lane: 76 KB per wave, conflict
// free since a lane only ever reads its own column).  A launch covers one size class; a wave whose fold belongs to another returns.
// The trials of a (fold, chunk) are shared out over grid z in blocks of rb, each of which factors G_j again (the factor is a few
// trials' worth of work) so that few large folds still fill the chip; a trial's numbers do not depend on rb.
// Sums over j: log det, q and e^2 are added over the 64 lanes of a chunk by a fixed butterfly, one partial per chunk, and
// efold_finish_kernel adds a row's chunks in index order.  The chunk length is a constant: the order is a function of nt alone, not
// of the grid, the other folds of the call or their order.  No atomics.
#include "kernels.hpp"

#include <algorithm>
#include <limits>

namespace gpcsd {

constexpr int EFOLD_CHUNK = 64;
constexpr int EFOLD_LDS_BYTES = (GPCSD_CV_MAX_FOLD * (GPCSD_CV_MAX_FOLD + 1) / 2 + GPCSD_CV_MAX_FOLD) * 64 * 8;        // factor + work vector

__device__ __forceinline__ double wave_sum64(double v) {      // fixed butterfly: every lane ends with the same sum
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// smallest kernel size (rows) of a fold of f electrodes: 1, 2, 4, 8 in registers, 16 in LDS
__host__ __device__ static inline int efold_class(int f) { return f <= 1 ? 1 : f <= 2 ? 2 : f <= 4 ? 4 : f <= 8 ? 8 : 16; }

template <int FM, bool INLDS>
__global__ __launch_bounds__(64) void efold_kernel(EfoldDesc g, int nchunks, int rb) {
    constexpr int UNROLL = INLDS ? 1 : 64;              // (a count above every trip count: the register form unrolls fully)
    constexpr int NPK = FM * (FM + 1) / 2;
    extern __shared__ double efold_sh[];
    const int fold = blockIdx.y;
    const int m0 = g.fold_ptr[fold], f = g.fold_ptr[fold + 1] - m0;              // wave-uniform
    if (efold_class(f) != FM) return;
    const int lane = threadIdx.x, chunk = blockIdx.x;
    const int j = chunk * EFOLD_CHUNK + lane;
    const bool active = j < g.nt;
    const int jc = active ? j : g.nt - 1;                    // idle lanes of the last chunk repeat its last index and store nothing
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double Lr[NPK], wr[FM], ur[FM];                          // (the register form's; unused and removed in the LDS form)
    int el[FM];                                              // the fold's electrodes
    double *const Ls = efold_sh + lane, *const ws = efold_sh + NPK * 64 + lane;
#define EF_L(i, k) (INLDS ? Ls[((i) * ((i) + 1) / 2 + (k)) * 64] : Lr[(i) * ((i) + 1) / 2 + (k)])
#define EF_W(i) (INLDS ? ws[(i) * 64] : wr[(i)])
#define EF_EL(i) (INLDS ? g.fold_idx[m0 + (i)] : el[(i)])
#define EF_VIDX(i, r) (((long)EF_EL(i) * g.R + (r)) * g.nt)
    if (!INLDS) {
#pragma unroll
        for (int i = 0; i < FM; ++i) el[i] = i < f ? g.fold_idx[m0 + i] : 0;
    }

    const double *__restrict__ Gp = g.Gp + (long)g.row0[fold] * g.nt + jc;
#pragma unroll UNROLL
    for (int p = 0; p < NPK; ++p)
        if (p < f * (f + 1) / 2) EF_L(0, p) = Gp[(long)p * g.nt];

    // ---- G = L L^T in place, row by row ----
    bool bad = false;
    double logdet = 0.0;
#pragma unroll UNROLL
    for (int i = 0; i < FM; ++i) {
        if (i >= f) break;
#pragma unroll UNROLL
        for (int k = 0; k <= i; ++k) {
            double s = EF_L(i, k);
#pragma unroll UNROLL
            for (int m = 0; m < k; ++m) s = __builtin_fma(-EF_L(i, m), EF_L(k, m), s);
            if (k == i) {
                if (!(s > 0.0 && s < std::numeric_limits<double>::infinity())) bad = true;
                logdet += log(s);
                EF_L(i, i) = sqrt(s);
            } else {
                EF_L(i, k) = s / EF_L(k, k);
            }
        }
    }
    if (bad) g.status[fold] = 1;                             // (every bad lane stores the same word)

    // ---- diag(G^-1): column a of L^-1 by forward substitution, the sum of its squares (the first block of trials only) ----
    const bool first = blockIdx.z == 0;                      // wave-uniform
#pragma unroll UNROLL
    for (int a = 0; a < FM; ++a) {
        if (a >= f || !first) break;
        double acc = 0.0;
#pragma unroll UNROLL
        for (int k = a; k < FM; ++k) {
            if (k >= f) break;
            double s = k == a ? 1.0 : 0.0;
#pragma unroll UNROLL
            for (int m = a; m < k; ++m) s = __builtin_fma(-EF_L(k, m), EF_W(m), s);
            const double x = s / EF_L(k, k);
            EF_W(k) = x;
            acc = __builtin_fma(x, x, acc);
        }
        if (active) g.pdiag[(long)EF_EL(a) * g.nt + j] = bad ? nan : acc;
    }
    if (first) {
        const double ld = wave_sum64(active ? (bad ? nan : logdet) : 0.0);
        if (lane == 0) g.part_ld[(long)fold * nchunks + chunk] = ld;
    }

    // ---- the trials: e = G^-1 u through the factor ----
    const int r_lo = blockIdx.z * rb, r_hi = r_lo + rb < g.R ? r_lo + rb : g.R;
    for (int r = r_lo; r < r_hi; ++r) {
        // (the LDS form does not keep u: it reads it again for q, from the cache)
#define EF_U(i) (INLDS ? g.V[EF_VIDX(i, r) + jc] : ur[(i)])
        if (!INLDS) {
#pragma unroll
            for (int i = 0; i < FM; ++i)
                if (i < f) ur[i] = g.V[EF_VIDX(i, r) + jc];
        }
#pragma unroll UNROLL
        for (int i = 0; i < FM; ++i) {                       // L z = u
            if (i >= f) break;
            double s = EF_U(i);
#pragma unroll UNROLL
            for (int m = 0; m < i; ++m) s = __builtin_fma(-EF_L(i, m), EF_W(m), s);
            EF_W(i) = s / EF_L(i, i);
        }
#pragma unroll UNROLL
        for (int ii = 0; ii < FM; ++ii) {                    // L^T e = z, last row first
            const int i = FM - 1 - ii;
            if (i >= f) continue;
            double s = EF_W(i);
#pragma unroll UNROLL
            for (int m = i + 1; m < FM; ++m)
                if (m < f) s = __builtin_fma(-EF_L(m, i), EF_W(m), s);
            EF_W(i) = s / EF_L(i, i);
        }
        double q = 0.0;
#pragma unroll UNROLL
        for (int i = 0; i < FM; ++i) {
            if (i >= f) break;
            const double e = bad ? nan : EF_W(i);
            q = __builtin_fma(EF_U(i), e, q);
            if (g.E && active) g.E[EF_VIDX(i, r) + j] = e;
            EF_W(i) = active ? e * e : 0.0;
        }
#pragma unroll UNROLL
        for (int i = 0; i < FM; ++i) {                       // (no exit from a loop that holds the wave's shuffles)
            if (i < f) {
                const double s2 = wave_sum64(EF_W(i));
                if (lane == 0) g.part_sse[((long)(m0 + i) * g.R + r) * nchunks + chunk] = s2;
            }
        }
        const double qs = wave_sum64(active ? q : 0.0);
        if (lane == 0) g.part_q[((long)fold * g.R + r) * nchunks + chunk] = qs;
    }
#undef EF_L
#undef EF_W
#undef EF_U
#undef EF_EL
#undef EF_VIDX
}

// lpd[fold][r] = 1/2 sum_chunks logdet - 1/2 sum_chunks q - f nt log(2 pi) / 2,   sse[a][r] = sum_chunks e^2, chunks in index order;
// a fold whose status is set gets NaN.  One thread per (fold, r) and per (member, r).
__global__ __launch_bounds__(256) void efold_finish_kernel(EfoldDesc g, int nchunks, int nmem) {
    const long t = blockIdx.x * 256L + threadIdx.x;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const long nl = (long)g.nfolds * g.R;
    if (t < nl) {
        const int fold = (int)(t / g.R);
        const int f = g.fold_ptr[fold + 1] - g.fold_ptr[fold];
        double sl = 0.0, sq = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            sl += g.part_ld[(long)fold * nchunks + c];
            sq += g.part_q[t * nchunks + c];
        }
        const double v = (0.5 * sl - 0.5 * sq) - (double)((long)f * g.nt) * 0.91893853320467274178;
        g.lpd[t] = g.status[fold] ? nan : v;
    } else if (t < nl + (long)nmem * g.R) {
        const long u = t - nl;
        const int m = (int)(u / g.R), r = (int)(u % g.R);
        double s = 0.0;
        for (int c = 0; c < nchunks; ++c) s += g.part_sse[u * nchunks + c];
        g.sse[(long)g.fold_idx[m] * g.R + r] = g.status[g.mem_fold[m]] ? nan : s;
    }
}

long efold_partials(const EfoldDesc &d, int nmem) {
    const long nchunks = ceil_div(d.nt, EFOLD_CHUNK);
    return nchunks * ((long)d.nfolds + (long)d.nfolds * d.R + (long)nmem * d.R);
}

void efold_solve(gpcsd_ctx *c, EfoldDesc d, const int *h_fold_ptr, hipStream_t s) {
    GP_REQUIRE(d.nfolds > 0 && d.nt > 0 && d.R > 0 && d.Gp && d.V && d.fold_ptr && d.fold_idx && d.row0 && d.mem_fold && d.pdiag &&
                   d.lpd && d.sse && d.status && d.partials && h_fold_ptr, -3, "efold_solve: bad problem");
    const int nchunks = ceil_div(d.nt, EFOLD_CHUNK), nmem = h_fold_ptr[d.nfolds];
    GP_REQUIRE(d.nfolds < 65536, GPCSD_ERR_CAPACITY, "efold_solve: %d folds exceed one grid dimension", d.nfolds);
    bool have[5] = {false, false, false, false, false};
    for (int i = 0; i < d.nfolds; ++i) {
        const int f = h_fold_ptr[i + 1] - h_fold_ptr[i];
        GP_REQUIRE(f >= 1 && f <= GPCSD_CV_MAX_FOLD, -3, "efold_solve: fold %d holds %d electrodes", i, f);
        const int cl = efold_class(f);
        have[cl == 1 ? 0 : cl == 2 ? 1 : cl == 4 ? 2 : cl == 8 ? 3 : 4] = true;
    }
    d.part_ld = d.partials;
    d.part_q = d.part_ld + (long)nchunks * d.nfolds;
    d.part_sse = d.part_q + (long)nchunks * d.nfolds * d.R;
    GP_HIP(hipMemsetAsync(d.status, 0, (size_t)d.nfolds * sizeof(int), s));
    // blocks of trials: about 2048 waves in flight where the trials allow, at least four trials per factorisation
    const long want = ceil_div(2048L, (long)nchunks * d.nfolds);
    const int nz = (int)std::max(1L, std::min(want, (long)ceil_div(d.R, 4)));
    const int rb = ceil_div(d.R, nz);
    const dim3 grid((unsigned)nchunks, (unsigned)d.nfolds, (unsigned)ceil_div(d.R, rb));
    {
        ProfScope ps(c, "efold_solve", 0.0, s);
        if (have[0]) hipLaunchKernelGGL((efold_kernel<1, false>), grid, dim3(64), 0, s, d, nchunks, rb);
        if (have[1]) hipLaunchKernelGGL((efold_kernel<2, false>), grid, dim3(64), 0, s, d, nchunks, rb);
        if (have[2]) hipLaunchKernelGGL((efold_kernel<4, false>), grid, dim3(64), 0, s, d, nchunks, rb);
        if (have[3]) hipLaunchKernelGGL((efold_kernel<8, false>), grid, dim3(64), 0, s, d, nchunks, rb);
        if (have[4]) {
            static PerDeviceOnce attr_once;
            if (attr_once.first())
                GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(efold_kernel<16, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           EFOLD_LDS_BYTES));
            hipLaunchKernelGGL((efold_kernel<16, true>), grid, dim3(64), EFOLD_LDS_BYTES, s, d, nchunks, rb);
        }
        GP_HIP(hipGetLastError());
    }
    const long nthr = ((long)d.nfolds + nmem) * d.R;
    hipLaunchKernelGGL(efold_finish_kernel, dim3((unsigned)ceil_div(nthr, 256L)), dim3(256), 0, s, d, nchunks, nmem);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
