// Standard normals on the device (gpcsd_normals; the source of gpcsd_sample_posterior's draws) and the small elementwise passes of
// a posterior draw.  No reference counterpart: the reference draws with numpy.random on the host (gpcsd1d.py:300, gpcsd2d.py:341).
#include "kernels.hpp"
#include "philox.hpp"

namespace gpcsd {

static inline int ew_grid(long n, int per_block = 256) { return (int)std::max(1L, std::min((n + per_block - 1) / per_block, 8192L)); }

// ------------------------------------------------------------------------------------------------
// out[k] = normal[first + k], k < count, of stream `stream` under `seed` (philox.hpp)
// ------------------------------------------------------------------------------------------------
// One thread, one pair: ten Philox rounds, one log, one sqrt, one sincos, 16 bytes out.  No LDS, no atomics.  The pair of a lane
// is written by one 128-bit store when `first` is even (out[k] with k even starts a pair) and out is 16-byte aligned -- uniform
// over the launch --; consecutive lanes then write consecutive 16-byte pieces, 1 KB per wave instruction.  An odd `first` splits a
// pair at either end of the range: the two halves are then stored as doubles, each bounds-checked.
template <bool VEC>
__global__ __launch_bounds__(256) void normals_kernel(unsigned long long seed, unsigned stream, unsigned long long first, long count,
                                                      double *__restrict__ out) {
    const unsigned long long pair0 = first >> 1;
    const long npairs = (long)(((first + (unsigned long long)count + 1) >> 1) - pair0);
    for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < npairs; j += (long)gridDim.x * blockDim.x) {
        double n0, n1;
        philox_normal_pair(seed, stream, pair0 + (unsigned long long)j, n0, n1);
        if (VEC) {                                        // first even: k = 2 j
            const long k = 2 * j;
            if (k + 1 < count) *reinterpret_cast<double2 *>(out + k) = make_double2(n0, n1);
            else out[k] = n0;                             // (the last pair of an odd count)
        } else {
            const long k = 2 * j - (long)(first & 1);     // index of the pair's first half in out: -1 for the split first pair
            if (k >= 0) out[k] = n0;                      // (k < count: the pair would not have been counted otherwise)
            if (k + 1 < count) out[k + 1] = n1;
        }
    }
}

void k_normals(gpcsd_ctx *c, unsigned long long seed, unsigned stream, unsigned long long first, long count, double *out, hipStream_t s) {
    GP_REQUIRE(out && count > 0, -3, "normals: bad arguments");
    GP_REQUIRE(first + (unsigned long long)count >= first, -3, "normals: first + count wraps around 2^64");
    const long npairs = (long)(((first + (unsigned long long)count + 1) >> 1) - (first >> 1));
    ProfScope ps(c, "rng_normals", 0.0, s);
    const bool vec = (first & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (vec) hipLaunchKernelGGL(normals_kernel<true>, dim3(ew_grid(npairs)), dim3(256), 0, s, seed, stream, first, count, out);
    else hipLaunchKernelGGL(normals_kernel<false>, dim3(ew_grid(npairs)), dim3(256), 0, s, seed, stream, first, count, out);
    GP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// the residual of a posterior draw, in the layout the projection reads: (x, pseudo-trial, t)
// ------------------------------------------------------------------------------------------------
// out[x][q][t] = y[x][(p0 + q) / S][t] - phi[x][q][t] - eps[x][q][t] for the np pseudo-trials p0 .. p0 + np - 1 of a chunk
// (pseudo-trial p = r S + s: draw s of trial r; y holds the R resident trials as [x][r][t]).  out may be phi.
__global__ __launch_bounds__(256) void sample_residual_kernel(const double *__restrict__ y, const double *phi, const double *__restrict__ eps,
                                                              double *out, int nt, int R, long p0, int np, int S, long total) {
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long row = e / nt;                          // (x, q)
        const int t = (int)(e - row * nt);
        const long x = row / np;
        const long r = (p0 + (row - x * np)) / S;
        out[e] = y[(x * R + r) * nt + t] - phi[e] - eps[e];
    }
}

void k_sample_residual(gpcsd_ctx *c, const double *y, const double *phi, const double *eps, double *out, int nx, int nt, int R, long p0,
                       int np, int S, hipStream_t s) {
    GP_REQUIRE(np > 0 && S > 0 && p0 >= 0 && (p0 + np - 1) / S < R, -3, "sample residual: pseudo-trials %ld .. %ld are not draws of %d trials",
               p0, p0 + np - 1, R);
    const long total = (long)nx * np * nt;
    ProfScope ps(c, "sample_residual", 0.0, s);
    hipLaunchKernelGGL(sample_residual_kernel, dim3(ew_grid(total)), dim3(256), 0, s, y, phi, eps, out, nt, R, p0, np, S, total);
    GP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// assembling and factoring the joint prior covariances
// ------------------------------------------------------------------------------------------------
// One block of a symmetric matrix J (order n, row-major) and its mirror image, from ONE copy of the block: off the diagonal
// J[r0 + i][c0 + j] = J[c0 + j][r0 + i] = src[i][j]; on the diagonal (r0 == c0, nr == nc) both triangles from src's lower one.
__global__ __launch_bounds__(256) void sym_place_kernel(double *__restrict__ J, int n, int r0, int c0, const double *__restrict__ src,
                                                        int nr, int nc) {
    const long total = (long)nr * nc;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / nc), j = (int)(e - (long)i * nc);
        if (r0 == c0) {
            J[(long)(r0 + i) * n + c0 + j] = i >= j ? src[e] : src[(long)j * nc + i];
        } else {
            const double v = src[e];
            J[(long)(r0 + i) * n + c0 + j] = v;
            J[(long)(c0 + j) * n + r0 + i] = v;
        }
    }
}

void k_sym_place(gpcsd_ctx *c, double *J, int n, int r0, int c0, const double *src, int nr, int nc, hipStream_t s) {
    GP_REQUIRE(r0 >= 0 && c0 >= 0 && nr > 0 && nc > 0 && r0 + nr <= n && c0 + nc <= n && (r0 != c0 || nr == nc) &&
                   (r0 == c0 || r0 >= c0 + nc || c0 >= r0 + nr),
               -3, "sym place: block (%d, %d) + (%d, %d) does not fit a symmetric matrix of order %d", r0, c0, nr, nc, n);
    hipLaunchKernelGGL(sym_place_kernel, dim3(ew_grid((long)nr * nc)), dim3(256), 0, s, J, n, r0, c0, src, nr, nc);
    GP_HIP(hipGetLastError());
}

// dsq[i] = sqrt(J[i][i]), dinv[i] = 1 / dsq[i] (0 for a diagonal entry that is not positive: its row and column are then zeroed)
__global__ void equil_diag_kernel(const double *__restrict__ J, int n, double *__restrict__ dsq, double *__restrict__ dinv) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double d = J[(long)i * n + i];
        const double q = d > 0.0 ? sqrt(d) : 0.0;
        dsq[i] = q;
        dinv[i] = q > 0.0 ? 1.0 / q : 0.0;
    }
}
// J[i][j] *= dinv[i] dinv[j]: one rounded factor per entry, the same for (i, j) and (j, i), so a symmetric J stays symmetric
__global__ __launch_bounds__(256) void equil_scale_kernel(double *__restrict__ J, int n, const double *__restrict__ dinv) {
    const long total = (long)n * n;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / n), j = (int)(e - (long)i * n);
        J[e] *= dinv[i] * dinv[j];
    }
}

void k_sym_equilibrate(gpcsd_ctx *c, double *J, int n, double *dsq, double *dinv, hipStream_t s) {
    hipLaunchKernelGGL(equil_diag_kernel, dim3(ew_grid(n)), dim3(256), 0, s, J, n, dsq, dinv);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(equil_scale_kernel, dim3(ew_grid((long)n * n)), dim3(256), 0, s, J, n, dinv);
    GP_HIP(hipGetLastError());
}

// F[i][k] = rowscale[i] Q[i][k] sqrt(max(w[k], 0)): the factor F F^T = diag(rowscale) Q diag(max(w, 0)) Q^T diag(rowscale) of a
// positive semi-definite matrix from its eigen-decomposition; eigenvalues of rounding size below zero count as zero, nothing is
// added.  rowscale == nullptr: ones; nw == 1: every column takes w[0].  F may be Q.
__global__ __launch_bounds__(256) void eig_factor_kernel(const double *Q, const double *__restrict__ w, int nw,
                                                         const double *__restrict__ rowscale, double *F, int n) {
    const long total = (long)n * n;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / n), k = (int)(e - (long)i * n);
        const double wk = w[nw == 1 ? 0 : k];
        const double f = Q[e] * sqrt(wk > 0.0 ? wk : 0.0);
        F[e] = rowscale ? rowscale[i] * f : f;
    }
}

void k_eig_factor(gpcsd_ctx *c, const double *Q, const double *w, int nw, const double *rowscale, double *F, int n, hipStream_t s) {
    GP_REQUIRE(nw == 1 || nw == n, -3, "eig factor: %d eigenvalues for a matrix of order %d", nw, n);
    hipLaunchKernelGGL(eig_factor_kernel, dim3(ew_grid((long)n * n)), dim3(256), 0, s, Q, w, nw, rowscale, F, n);
    GP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// out[z][j][p0 + q] = upd[z][j][q] + prior[z][q][j]: a chunk of draws into the output layout (z, t*, pseudo-trial)
// ------------------------------------------------------------------------------------------------
// upd is the chunk's update P (y - phi - eps) as the last product of a prediction writes it, prior the matching block of the joint
// prior draw as its batched product writes it (pseudo-trial before time): per site a 32 x 32 LDS-tiled transpose of the (q, j)
// block, so that both reads and the write run along their innermost index.
__global__ __launch_bounds__(256) void sample_combine_kernel(const double *__restrict__ upd, const double *__restrict__ prior,
                                                             double *__restrict__ out, int nts, int np, long P, long p0) {
    __shared__ double tile[32][33];
    const long z = blockIdx.z;
    const int j0 = blockIdx.x * 32, q0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    const double *pz = prior + z * (long)np * nts;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + ty + 8 * k, j = j0 + tx;
        if (q < np && j < nts) tile[ty + 8 * k][tx] = pz[(long)q * nts + j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + ty + 8 * k, q = q0 + tx;
        if (q < np && j < nts) out[(z * nts + j) * P + p0 + q] = upd[(z * nts + j) * (long)np + q] + tile[tx][ty + 8 * k];
    }
}

void k_sample_combine(gpcsd_ctx *c, const double *upd, const double *prior, double *out, int nz, int nts, int np, long P, long p0,
                      hipStream_t s) {
    GP_REQUIRE(nz > 0 && nz < 65536 && nts > 0 && np > 0 && p0 >= 0 && p0 + np <= P && ceil_div(np, 32) < 65536, -3,
               "sample combine: chunk %ld + %d of %ld pseudo-trials at %d sites", p0, np, P, nz);
    ProfScope ps(c, "sample_combine", 0.0, s);
    hipLaunchKernelGGL(sample_combine_kernel, dim3(ceil_div(nts, 32), ceil_div(np, 32), nz), dim3(256), 0, s, upd, prior, out, nts, np, P, p0);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
