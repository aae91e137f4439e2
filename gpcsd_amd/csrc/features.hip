// Region features of a field (gpcsd_region_features, gpcsd_sample_features): per labelled region of the (z, t*) plane and per column
// (a trial of a prediction, a pseudo-trial of posterior draws) the extrema with the place of their first occurrence, the sums that
// give the centre of mass, and the largest standardised deviation from a mean.  No reference counterpart as a routine: the reference's
// analysis takes scipy.ndimage.center_of_mass of each segmented region of ONE evoked field on the host
// (auditory_lfp/fit_mean_function.py:350-353); here the same reductions run over every column where the field lies.
//
// The field is F[(i * nts + k) * ld + p], the column p innermost (the layout of a prediction and of the draws).  The host turns the
// label map into the list of every region's points in row-major (z, t*) order and cuts each region's list into slices of FEAT_SLICE
// points.  feat_slice_kernel: one wave per (slice, tile of 64 columns), a lane per column -- the 64 loads of a point are 512
// contiguous bytes --, the point loop unrolled eight times so that eight such loads are in flight per wave, the ten accumulators in
// registers; everything about a point that does not depend on the column (its index, coordinates, 1 / sd) is the same in every lane
// and comes from the list.  It writes one partial per slice; feat_fold_kernel folds a region's partials in slice order.
// Order: a column's sums are taken over the points of a slice in list order and over the slices in order -- a function of the label
// map alone, not of the number of columns, of which columns share the call, or of the grid: the same call returns the same bits, and
// a column's result does not change with its neighbours.  Extrema are replaced on a strict comparison only, so the first point in
// row-major order wins a tie.  No atomics, no LDS.  NaN inputs are NOT supported (comparisons with NaN are false: a NaN is skipped
// by the extrema and poisons the sums); nothing checks for them.
#include "kernels.hpp"

#include <limits>

namespace gpcsd {

struct SliceAcc {
    double mx, imx, mn, imn, s, sa, st, s0, s1, sup;
};

template <bool BAND>
__device__ __forceinline__ void feat_point(SliceAcc &a, double v, int id, double tau, double z0, double z1, double mean, double isd) {
    if (v > a.mx) { a.mx = v; a.imx = (double)id; }
    if (v < a.mn) { a.mn = v; a.imn = (double)id; }
    const double av = fabs(v);
    a.s += v;
    a.sa += av;
    a.st += av * tau;
    a.s0 += av * z0;
    a.s1 += av * z1;
    if (BAND) {
        const double d = fabs(v - mean) * isd;
        if (d > a.sup) a.sup = d;
    }
}

template <bool BAND>
__global__ __launch_bounds__(64) void feat_slice_kernel(FeatPlan pl, FeatDesc d) {
    const int sl = blockIdx.x;
    const int col = blockIdx.y * 64 + threadIdx.x;
    const int cc = col < d.ncol ? col : d.ncol - 1;          // (idle lanes of the last tile repeat its last column: no divergence)
    const int beg = pl.slice_beg[sl], cnt = pl.slice_cnt[sl];
    const int *__restrict__ idx = pl.idx + beg;
    const double *__restrict__ ptau = pl.ptau + beg, *__restrict__ pz0 = pl.pz0 + beg, *__restrict__ pz1 = pl.pz1 + beg;
    const double *__restrict__ Fc = d.F + cc;
    const double *__restrict__ mc = BAND ? d.mean + (d.col0 + cc) / d.S : nullptr;      // the column's trial
    const double inf = std::numeric_limits<double>::infinity();
    SliceAcc a = {-inf, -1.0, inf, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -inf};
    int n = 0;
    for (; n + 8 <= cnt; n += 8) {
        int id[8];
        double v[8], m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            id[u] = idx[n + u];
            v[u] = Fc[(long)id[u] * d.ld];
            m[u] = BAND ? mc[(long)id[u] * d.R] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            feat_point<BAND>(a, v[u], id[u], ptau[n + u], pz0[n + u], pz1[n + u], m[u], BAND ? d.isd[id[u]] : 0.0);
    }
    for (; n < cnt; ++n) {
        const int id = idx[n];
        feat_point<BAND>(a, Fc[(long)id * d.ld], id, ptau[n], pz0[n], pz1[n], BAND ? mc[(long)id * d.R] : 0.0, BAND ? d.isd[id] : 0.0);
    }
    if (col < d.ncol) {
        double *o = d.part + (long)sl * GPCSD_NFEAT * d.ncol + col;
        const double out[GPCSD_NFEAT] = {a.mx, a.imx, a.mn, a.imn, a.s, a.sa, a.st, a.s0, a.s1, a.sup};
#pragma unroll
        for (int k = 0; k < GPCSD_NFEAT; ++k) o[(long)k * d.ncol] = out[k];
    }
}

// feat[j][slot][col0 + col]: the partials of region j's slices folded in slice order; a region without a point gets the documented
// values.  Slot 9 is NaN when no mean was given.
__global__ __launch_bounds__(64) void feat_fold_kernel(FeatPlan pl, FeatDesc d, int band) {
    const int j = blockIdx.x;
    const int col = blockIdx.y * 64 + threadIdx.x;
    if (col >= d.ncol) return;
    const double inf = std::numeric_limits<double>::infinity();
    SliceAcc a = {-inf, -1.0, inf, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -inf};
    for (int sl = pl.reg_slice[j]; sl < pl.reg_slice[j + 1]; ++sl) {
        const double *p = d.part + (long)sl * GPCSD_NFEAT * d.ncol + col;
        const long n = d.ncol;
        if (p[0] > a.mx) { a.mx = p[0]; a.imx = p[n]; }
        if (p[2 * n] < a.mn) { a.mn = p[2 * n]; a.imn = p[3 * n]; }
        a.s += p[4 * n];
        a.sa += p[5 * n];
        a.st += p[6 * n];
        a.s0 += p[7 * n];
        a.s1 += p[8 * n];
        if (p[9 * n] > a.sup) a.sup = p[9 * n];
    }
    double *o = d.feat + (long)j * GPCSD_NFEAT * d.ldf + d.col0 + col;
    const double out[GPCSD_NFEAT] = {a.mx, a.imx, a.mn, a.imn, a.s, a.sa, a.st, a.s0, a.s1,
                                     band ? a.sup : std::numeric_limits<double>::quiet_NaN()};
#pragma unroll
    for (int k = 0; k < GPCSD_NFEAT; ++k) o[(long)k * d.ldf] = out[k];
}

void k_region_features(gpcsd_ctx *c, const FeatPlan &pl, const FeatDesc &d, hipStream_t s) {
    const bool band = d.mean != nullptr;
    const long tiles = ((long)d.ncol + 63) / 64;
    GP_REQUIRE(d.F && d.part && d.feat && pl.J > 0 && d.ncol > 0 && d.ld >= d.ncol && d.col0 >= 0 && d.col0 + d.ncol <= d.ldf, -3,
               "region features: bad arguments");
    GP_REQUIRE(band == (d.isd != nullptr) && (!band || (d.R > 0 && d.S > 0 && (d.col0 + d.ncol - 1) / d.S < d.R)), -3,
               "region features: the mean and 1 / sd come together, with R trials of S columns each");
    GP_REQUIRE(tiles < 65536, GPCSD_ERR_CAPACITY, "region features: %d columns in one launch", d.ncol);
    ProfScope ps(c, "region_features", 0.0, s);
    if (pl.nslice > 0) {
        const dim3 grid(pl.nslice, (unsigned)tiles);
        if (band) hipLaunchKernelGGL(feat_slice_kernel<true>, grid, dim3(64), 0, s, pl, d);
        else hipLaunchKernelGGL(feat_slice_kernel<false>, grid, dim3(64), 0, s, pl, d);
        GP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(feat_fold_kernel, dim3(pl.J, (unsigned)tiles), dim3(64), 0, s, pl, d, band ? 1 : 0);
    GP_HIP(hipGetLastError());
}

// ptau / pz0 / pz1 [n] = tau[k], zeta[i][0], zeta[i][1] (0 for dim = 1) of list entry n, idx[n] = i * nts + k
__global__ __launch_bounds__(256) void feat_coords_kernel(const int *__restrict__ idx, int npts, int nts, const double *__restrict__ tau,
                                                          const double *__restrict__ zeta, int dim, double *__restrict__ ptau,
                                                          double *__restrict__ pz0, double *__restrict__ pz1) {
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < npts; n += gridDim.x * blockDim.x) {
        const int i = idx[n] / nts, k = idx[n] - i * nts;
        ptau[n] = tau[k];
        pz0[n] = zeta[(long)i * dim];
        pz1[n] = dim == 2 ? zeta[(long)i * dim + 1] : 0.0;
    }
}

void k_feat_coords(gpcsd_ctx *c, const int *idx, int npts, int nts, const double *tau, const double *zeta, int dim, double *ptau,
                   double *pz0, double *pz1, hipStream_t s) {
    if (npts <= 0) return;
    GP_REQUIRE(idx && tau && zeta && ptau && pz0 && pz1 && nts > 0 && (dim == 1 || dim == 2), -3, "feature coordinates: bad arguments");
    hipLaunchKernelGGL(feat_coords_kernel, dim3(std::min((npts + 255) / 256, 4096)), dim3(256), 0, s, idx, npts, nts, tau, zeta, dim, ptau,
                       pz0, pz1);
    GP_HIP(hipGetLastError());
}

// isd[k] = 1 / sqrt(var[k]) where var[k] > floor * max(var), 0 elsewhere: one block finds the maximum (vmax, one double), the
// second launch applies the rule.  (A variance that rounding left at or below zero has no band: its point drops out of the supremum.)
__global__ __launch_bounds__(1024) void feat_varmax_kernel(const double *__restrict__ var, long n, double *__restrict__ vmax) {
    __shared__ double red[1024];
    double m = -std::numeric_limits<double>::infinity();
    for (long k = threadIdx.x; k < n; k += 1024) m = var[k] > m ? var[k] : m;
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && red[threadIdx.x + w] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *vmax = red[0];
}
__global__ __launch_bounds__(256) void feat_isd_kernel(const double *__restrict__ var, long n, double floor, const double *__restrict__ vmax,
                                                       double *__restrict__ isd) {
    const double cut = floor * *vmax;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x)
        isd[k] = var[k] > cut ? 1.0 / sqrt(var[k]) : 0.0;
}

void k_feat_isd(gpcsd_ctx *c, const double *var, long n, double floor, double *vmax, double *isd, hipStream_t s) {
    GP_REQUIRE(var && vmax && isd && n > 0, -3, "feature band: bad arguments");
    hipLaunchKernelGGL(feat_varmax_kernel, dim3(1), dim3(1024), 0, s, var, n, vmax);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(feat_isd_kernel, dim3((unsigned)std::min((n + 255) / 256, 4096L)), dim3(256), 0, s, var, n, floor, vmax, isd);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
