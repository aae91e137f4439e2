// The trial-shift objective and its analytic gradient on the device (gfx950): what auditory_lfp/fit_mean_function.py:306-321 evaluates
// on the host for every trial and every L-BFGS-B step -- background + time-shifted component means (scipy.interpolate.interp1d, linear,
// fill_value="extrapolate"), the residual whitened by (Qs, Qt, D), a Gaussian prior on the shifts -- for B points (trial_b, tau_b) at once.
//
//   shift_slope_kernel    slope_i[x][k] = (y_i[x][k+1] - y_i[x][k]) / (t[k+1] - t[k])                 once per plan
//   shift_locate_kernel   lo = clip(searchsorted_left(t, t_k + tau_i), 1, nt - 1) - 1,  dt = (t_k + tau_i) - t_lo   per (b, i, k)
//   shift_resid_kernel    R[x][b][k] = lfp[x][trial_b][k] - (mu_0[x][k] + sum_i y_i[x][lo] + slope_i[x][lo] dt)
//   shift_quad_kernel     beta = alpha / D,  f[b] = 1/2 sum alpha beta + prior        (alpha = Qs^T R Qt: two gemm_f64 launches)
//   shift_grad_kernel     g[b][i] = -sum_{x,k} Z[x][b][k] slope_i[x][lo] + prior'     (Z = Qs beta Qt^T: two more)
//   (both reduce per (point, slab of 16 electrodes); shift_*_finish_kernel adds a point's slabs in order and the prior's term)
//
// Between knots f is quadratic in tau and g is its derivative on the segments the interpolation itself uses: a sample on a knot takes
// the segment to its LEFT (searchsorted "left"), so at such a point g is the left derivative.  The segment search is a binary search in
// t (grids need not be uniform) and is shared by all electrodes; lo is monotone in k, so the gathers of y_i and slope_i along k are as
// good as coalesced.  Every field is written in the (x, b, k) layout both projections read as flat GEMMs: no transpose pass.
//
// All kernels are memory- or latency-bound: 256 threads = four waves of 64, 8-byte accesses along k, LDS only for the workgroup sums.
// The sums run per thread, per wave (DPP), per workgroup, per slab in one fixed order and nothing is added atomically: a point's (f, g) has the
// same bits on every call and with or without the gradient, and these kernels do not see which other points share its batch.
#include "devutil.hpp"
#include "kernels.hpp"

namespace gpcsd {

namespace {
constexpr int XB = 4;      // electrodes per thread of the residual kernel: one (lo, dt) pair serves them all
constexpr int XSLAB = 16;  // electrodes per workgroup of the two reducing kernels
}  // namespace

int shift_slabs(int nx) { return ceil_div(nx, XSLAB); }

__global__ __launch_bounds__(256) void shift_slope_kernel(const double *__restrict__ mu, const double *__restrict__ t, int nx, int nt,
                                                          int nseg, double *__restrict__ slope) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= (long)nseg * nx * (nt - 1)) return;
    const int k = (int)(e % (nt - 1));
    const long r = e / (nt - 1);
    const int x = (int)(r % nx), i = (int)(r / nx);
    const double *y = mu + ((long)x * (nseg + 1) + i + 1) * nt;
    slope[e] = (y[k + 1] - y[k]) / (t[k + 1] - t[k]);
}

void k_shift_slopes(gpcsd_ctx *c, const double *mu, const double *t, int nx, int nt, int nseg, double *slope, hipStream_t s) {
    ProfScope ps(c, "shift_slopes", 0.0, s);
    hipLaunchKernelGGL(shift_slope_kernel, dim3(ceil_div((long)nseg * nx * (nt - 1), 256)), dim3(256), 0, s, mu, t, nx, nt, nseg, slope);
    GP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void shift_locate_kernel(const double *__restrict__ t, int nt, const double *__restrict__ tau, long n,
                                                           int *__restrict__ lo, double *__restrict__ dt) {
    const long e = blockIdx.x * 256L + threadIdx.x;      // (b * nseg + i) * nt + k
    if (e >= n) return;
    const double v = t[e % nt] + tau[e / nt];
    int a = 0, b = nt;                                   // first index with t[index] >= v
    while (a < b) {
        const int m = (a + b) >> 1;
        if (t[m] < v) a = m + 1;
        else b = m;
    }
    const int l = min(max(a, 1), nt - 1) - 1;
    lo[e] = l;
    dt[e] = v - t[l];
}

void k_shift_locate(gpcsd_ctx *c, const ShiftDesc &d, hipStream_t s) {
    const long n = (long)d.B * d.nseg * d.nt;
    ProfScope ps(c, "shift_locate", 0.0, s);
    hipLaunchKernelGGL(shift_locate_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, d.t, d.nt, d.tau, n, d.lo, d.dt);
    GP_HIP(hipGetLastError());
}

// threads along the flat (b, k) index of an electrode's row of R; blockIdx.y: a group of XB electrodes
__global__ __launch_bounds__(256) void shift_resid_kernel(ShiftDesc d, double *__restrict__ R) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= (long)d.B * d.nt) return;
    const int b = (int)(e / d.nt), k = (int)(e % d.nt);
    const int x0 = blockIdx.y * XB;
    const long cstride = (long)d.nt;                     // mu: [x][c][k]
    double acc[XB];
    const double *row[XB];
#pragma unroll
    for (int j = 0; j < XB; ++j) {
        const int x = min(x0 + j, d.nx - 1);            // (a group past the end repeats the last electrode and stores nothing)
        row[j] = d.mu + (long)x * (d.nseg + 1) * cstride;
        acc[j] = row[j][k];
    }
    for (int i = 0; i < d.nseg; ++i) {
        const long at = ((long)b * d.nseg + i) * d.nt + k;
        const int l = d.lo[at];
        const double h = d.dt[at];
#pragma unroll
        for (int j = 0; j < XB; ++j) {
            const int x = min(x0 + j, d.nx - 1);
            acc[j] += row[j][(i + 1) * cstride + l] + d.slope[((long)i * d.nx + x) * (d.nt - 1) + l] * h;
        }
    }
    const int tr = d.trial[b];
#pragma unroll
    for (int j = 0; j < XB; ++j) {
        const int x = x0 + j;
        if (x < d.nx) R[((long)x * d.B + b) * d.nt + k] = d.lfp[((long)x * d.ntrials + tr) * d.nt + k] - acc[j];
    }
}

void k_shift_resid(gpcsd_ctx *c, const ShiftDesc &d, double *R, hipStream_t s) {
    ProfScope ps(c, "shift_resid", 0.0, s);
    hipLaunchKernelGGL(shift_resid_kernel, dim3(ceil_div((long)d.B * d.nt, 256), ceil_div(d.nx, XB)), dim3(256), 0, s, d, R);
    GP_HIP(hipGetLastError());
}

// One workgroup per (point, slab of XSLAB electrodes): at 384 electrodes one workgroup per point leaves most of the chip idle and
// each workgroup with 1.5 MB to walk.  The slabs depend on nx alone, so a point's partial sums -- and, added in slab order by the
// finishing kernels, its results -- do not depend on the batch.  The arithmetic does not depend on whether beta is stored.
__global__ __launch_bounds__(256) void shift_quad_kernel(ShiftDesc d, const double *__restrict__ alpha, double *__restrict__ beta,
                                                         double *__restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.x, x0 = blockIdx.y * XSLAB, x1 = min(x0 + XSLAB, d.nx);
    double s = 0.0;
    for (long e = (long)x0 * d.nt + threadIdx.x; e < (long)x1 * d.nt; e += 256) {
        const int x = (int)(e / d.nt), i = (int)(e % d.nt);
        const long at = ((long)x * d.B + b) * d.nt + i;
        const double a = alpha[at], w = a / d.D[e];
        if (beta) beta[at] = w;
        s += a * w;
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[(long)b * gridDim.y + blockIdx.y] = s;
}

__global__ __launch_bounds__(256) void shift_quad_finish_kernel(ShiftDesc d, const double *__restrict__ part, int nslab,
                                                                double *__restrict__ f) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= d.B) return;
    double s = 0.0, p = 0.0;
    for (int k = 0; k < nslab; ++k) s += part[(long)b * nslab + k];
    for (int i = 0; i < d.nseg; ++i) {
        const double z = (d.tau[(long)b * d.nseg + i] - d.mutau) / d.sigtau;
        p += z * z;
    }
    f[b] = 0.5 * s + 0.5 * p;
}

void k_shift_quad(gpcsd_ctx *c, const ShiftDesc &d, const double *alpha, double *beta, double *part, double *f, hipStream_t s) {
    const int nslab = shift_slabs(d.nx);
    ProfScope ps(c, "shift_quad", 0.0, s);
    hipLaunchKernelGGL(shift_quad_kernel, dim3(d.B, nslab), dim3(256), 0, s, d, alpha, beta, part);
    hipLaunchKernelGGL(shift_quad_finish_kernel, dim3(ceil_div(d.B, 256)), dim3(256), 0, s, d, (const double *)part, nslab, f);
    GP_HIP(hipGetLastError());
}

// One workgroup per (point, slab).  Lanes run along k in chunks of 64 (a chunk's nseg segment indices stay in registers), the four
// waves take the slab's electrodes x = x0 + wave, x0 + wave + 4, ...: an element of Z is read once and meets all nseg gathered slopes.
// NS >= nseg is the compile-time length of the per-thread partial sums (runtime-indexed arrays would live in scratch).
template <int NS>
__global__ __launch_bounds__(256) void shift_grad_kernel(ShiftDesc d, const double *__restrict__ Z, double *__restrict__ part) {
    __shared__ double red[4][NS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.y * XSLAB, x1 = min(x0 + XSLAB, d.nx);
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int k0 = 0; k0 < d.nt; k0 += 64) {
        const int k = k0 + lane;
        if (k < d.nt) {
            int l[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) l[i] = i < d.nseg ? d.lo[((long)b * d.nseg + i) * d.nt + k] : 0;
            for (int x = x0 + wave; x < x1; x += 4) {
                const double z = Z[((long)x * d.B + b) * d.nt + k];
#pragma unroll
                for (int i = 0; i < NS; ++i)
                    if (i < d.nseg) acc[i] += z * d.slope[((long)i * d.nx + x) * (d.nt - 1) + l[i]];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < d.nseg) {
        const int i = threadIdx.x;
        part[((long)b * gridDim.y + blockIdx.y) * d.nseg + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

__global__ __launch_bounds__(256) void shift_grad_finish_kernel(ShiftDesc d, const double *__restrict__ part, int nslab,
                                                                double *__restrict__ g) {
    const long e = blockIdx.x * 256L + threadIdx.x;      // b * nseg + i
    if (e >= (long)d.B * d.nseg) return;
    const long b = e / d.nseg;
    const int i = (int)(e % d.nseg);
    double sum = 0.0;
    for (int k = 0; k < nslab; ++k) sum += part[(b * nslab + k) * d.nseg + i];
    g[e] = (d.tau[e] - d.mutau) / (d.sigtau * d.sigtau) - sum;
}

void k_shift_grad(gpcsd_ctx *c, const ShiftDesc &d, const double *Z, double *part, double *g, hipStream_t s) {
    GP_REQUIRE(d.nseg >= 1 && d.nseg <= SHIFT_MAX_NSEG, GPCSD_ERR_CAPACITY, "shift_grad: nseg = %d exceeds %d components", d.nseg, SHIFT_MAX_NSEG);
    const int nslab = shift_slabs(d.nx);
    const dim3 grid(d.B, nslab);
    ProfScope ps(c, "shift_grad", 0.0, s);
    if (d.nseg <= 4) hipLaunchKernelGGL(shift_grad_kernel<4>, grid, dim3(256), 0, s, d, Z, part);
    else if (d.nseg <= 8) hipLaunchKernelGGL(shift_grad_kernel<8>, grid, dim3(256), 0, s, d, Z, part);
    else if (d.nseg <= 16) hipLaunchKernelGGL(shift_grad_kernel<16>, grid, dim3(256), 0, s, d, Z, part);
    else hipLaunchKernelGGL(shift_grad_kernel<SHIFT_MAX_NSEG>, grid, dim3(256), 0, s, d, Z, part);
    hipLaunchKernelGGL(shift_grad_finish_kernel, dim3(ceil_div((long)d.B * d.nseg, 256)), dim3(256), 0, s, d, (const double *)part, nslab, g);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
