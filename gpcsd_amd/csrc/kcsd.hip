// Kernel CSD in one dimension with Gaussian sources (gfx950, v_mfma_f64_16x16x4_f64): the third estimator of the reference's
// comparisons (simulation_studies/sim_from_gp_1D.py:112-127, simple_template_1D.py:99-105, auditory_lfp/fit_mean_function.py:112-115),
// which those scripts take from the external kcsd package.  Stated here in closed form:
//
//   kcsd_basis_kernel   source basis g(z - s_j) or potential basis b_j(x) = 1/(2 varsigma) int_{-R}^{R} [sqrt((u - d)^2 + h^2) - |u - d|]
//                       g(u) du, d = x - s_j, by Gauss-Legendre on two panels split at the kink u = clip(d, -R, R); the bracket as
//                       h^2 / (sqrt(v^2 + h^2) + v), v = |u - d| (no cancellation for v >> h); 2 ngl terms, summed in node order
//   kcsd_diag_kernel    per (R, lambda): d_k = 1 / (max(s_k, 0) + lambda), a_i = (A^-1)_ii = sum_k U_ik^2 d_k, and the flag of a
//                       numerically singular pair (s_min + lambda < n 2^-52 s_max, or not positive)
//   kcsd_cv_kernel      per R and block of 64 columns t: beta[t][i] = sum_k W[k][t] (U[i][k] d_k) on the matrix cores (the transposed
//                       product, as gemm_loo_kernel: the long axis t fills the tiles however few electrodes there are), beta never
//                       stored: the epilogue forms (beta / a_i)^2 and adds it over the block's columns in a fixed order.  The
//                       workgroup's block of W stays in LDS (n <= KCSD_WRES_MAX_N; beyond it the block is read through the caches)
//                       while the workgroup goes through the lambda values, rescaling a 16-electrode panel of U each time
//   kcsd_fold_kernel    err(R, lambda) = sum_i sqrt(sum over column blocks in index order), electrodes in index order
//
// Fragment maps (torus.hip, gemm_f64.hip): A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15], C/D lane l reg r holds
// C[(l >> 4) + 4 r][l & 15].  No atomics: the same call gives the same bits, and an entry for one lambda does not depend on which
// other lambda values the call holds.
#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace gpcsd {

typedef double d4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int KC_PANEL = 128;                 // contracted indices per panel of U in LDS
constexpr int PANEL_LD = 17;                  // doubles per k row of the panel: 16 electrodes + 1, so that the fill's stores (16 lanes
                                              // along k) and the fragment reads (16 lanes along the electrodes) both spread over the banks
constexpr double INV_SQRT_2PI = 0.39894228040143267794;
}  // namespace

// ---------------------------------------------------------------- bases
struct KcsdBasisK {
    const double *src, *pts, *gx, *gw;
    int M, npts, ngl, which;
    double R, h, scale;          // scale = 1 / (2 varsigma)
    double *out;                 // (M, npts)
};

__global__ __launch_bounds__(256) void kcsd_basis_kernel(KcsdBasisK g) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)g.M * g.npts) return;
    const int j = (int)(idx / g.npts), p = (int)(idx - (long)j * g.npts);
    const double x = g.pts[p], s = g.src[j], R = g.R;
    // d = x - s without its rounding error: dh + dl exactly
    const double dh = x - s;
    const double bb = dh - x;
    const double dl = (x - (dh - bb)) + (-s - bb);
    const double cg = (3.0 * INV_SQRT_2PI) / R;                  // 1 / (sqrt(2 pi) sigma_b), sigma_b = R / 3
    if (g.which == 1) {
        // g(d) = cg exp(-4.5 (d / R)^2), the argument carried with its rounding error (a relative error e of the argument is a
        // relative error 4.5 (d / R)^2 e of the value)
        const double q = dh / R;
        const double ql = (fma(-q, R, dh) + dl) / R;
        const double ph = q * q;
        const double pl = fma(q, q, -ph) + 2.0 * q * ql;
        const double ah = 4.5 * ph;
        const double al = fma(4.5, ph, -ah) + 4.5 * pl;
        g.out[idx] = (cg * exp(-ah)) * (1.0 - al);
        return;
    }
    const double c = fmin(fmax(dh, -R), R);
    const double h2 = g.h * g.h;
    double acc = 0.0;
    for (int panel = 0; panel < 2; ++panel) {
        const double lo = panel ? c : -R, hi = panel ? R : c;
        const double half = 0.5 * (hi - lo), mid = 0.5 * (hi + lo);
        for (int qn = 0; qn < g.ngl; ++qn) {
            const double u = fma(half, g.gx[qn], mid);
            const double v = fabs((u - dh) - dl);
            const double br = h2 / (sqrt(fma(v, v, h2)) + v);
            const double t = u / R;
            acc += (half * g.gw[qn]) * (br * exp(-4.5 * (t * t)));
        }
    }
    g.out[idx] = acc * (cg * g.scale);
}

void k_kcsd_basis(gpcsd_ctx *c, const double *src, int M, const double *pts, int npts, double R, double h, double varsigma,
                  const double *gx, const double *gw, int ngl, int which, double *out, hipStream_t s) {
    KcsdBasisK k;
    k.src = src; k.pts = pts; k.gx = gx; k.gw = gw;
    k.M = M; k.npts = npts; k.ngl = ngl; k.which = which;
    k.R = R; k.h = h; k.scale = 1.0 / (2.0 * varsigma);
    k.out = out;
    ProfScope ps(c, "kcsd_basis", 0.0, s);
    hipLaunchKernelGGL(kcsd_basis_kernel, dim3((unsigned)(((long)M * npts + 255) / 256)), dim3(256), 0, s, k);
    GP_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- cross-validation table
struct KcsdCvK {
    const double *U;             // [nR][n][n], eigenvectors in columns
    const double *s;             // [nR][n]
    const double *W;             // [nR][n][T] = U^T V
    const double *lam;           // [nlam]
    int n, T, nR, nlam;
    int l0, nl;                  // the lambda values of this launch (the partial sums hold nl of them)
    int tiles;                   // blocks of 64 columns
    double *dtab, *adiag;        // [nR][nlam][n] each
    int *status;                 // [nR][nlam]: 1 = numerically singular
    double *partial;             // [nR][nl][tiles][n]
    double *err;                 // [nR][nlam]
};

__global__ __launch_bounds__(256) void kcsd_diag_kernel(KcsdCvK g) {
    __shared__ double dl[GPCSD_MAX_EIG_N];
    __shared__ double red[2][256];
    const int tid = threadIdx.x, l = blockIdx.x, r = blockIdx.y, n = g.n;
    const double *sr = g.s + (long)r * n;
    const double lam = g.lam[l];
    double mn = INFINITY, mx = 0.0;
    for (int k = tid; k < n; k += 256) {
        const double sk = fmax(sr[k], 0.0);
        mn = fmin(mn, sk);
        mx = fmax(mx, sk);
    }
    red[0][tid] = mn;
    red[1][tid] = mx;
    __syncthreads();
    mn = INFINITY;
    mx = 0.0;
    for (int i = 0; i < 256; ++i) {                              // (min and max are exact: any order gives the same result)
        mn = fmin(mn, red[0][i]);
        mx = fmax(mx, red[1][i]);
    }
    const long pair = (long)r * g.nlam + l;
    const bool singular = !(mn + lam > 0.0) || mn + lam < (double)n * 0x1p-52 * mx;
    if (tid == 0) g.status[pair] = singular ? 1 : 0;
    if (singular) return;                                        // (the whole workgroup)
    for (int k = tid; k < n; k += 256) {
        const double d = 1.0 / (fmax(sr[k], 0.0) + lam);
        dl[k] = d;
        g.dtab[pair * n + k] = d;
    }
    __syncthreads();
    const double *Ur = g.U + (long)r * n * n;
    for (int i = tid; i < n; i += 256) {
        const double *row = Ur + (long)i * n;
        double a = 0.0;
        for (int k = 0; k < n; ++k) {
            const double u = row[k];
            a += (u * u) * dl[k];
        }
        g.adiag[pair * n + i] = a;
    }
}

template <bool WRES>
__global__ __launch_bounds__(256) void kcsd_cv_kernel(KcsdCvK g) {
    extern __shared__ double wl[];                               // WRES: [wave][npad][16] -- a wave's 16 columns of every row of W
    __shared__ double panel[KC_PANEL * PANEL_LD];                // [k][electrode]: U[i0 + ii][k] d_k
    __shared__ double wsum[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int r = blockIdx.y, tile = blockIdx.x;
    const int n = g.n, T = g.T, npad = (n + 3) & ~3;
    const int t0 = tile * 64;
    const double *Wr = g.W + (long)r * n * T;
    const double *Ur = g.U + (long)r * n * n;
    if (WRES) {
        for (int idx = tid; idx < npad * 64; idx += 256) {
            const int k = idx >> 6, tt = idx & 63;
            const int t = min(t0 + tt, T - 1);                   // a column past the end repeats the last one; it is never summed
            wl[((long)(tt >> 4) * npad + k) * 16 + (tt & 15)] = k < n ? Wr[(long)k * T + t] : 0.0;
        }
        __syncthreads();
    }
    const int tw = min(t0 + wid * 16 + fr, T - 1);               // this lane's column of the A fragment
    const int pi = tid >> 4, pk = tid & 15;                      // panel fill: electrode, first k
    for (int l = g.l0; l < g.l0 + g.nl; ++l) {
        const long pair = (long)r * g.nlam + l;
        if (g.status[pair]) continue;                            // (workgroup-uniform) a singular pair costs nothing and touches nothing
        const double *dt = g.dtab + pair * n;
        const double *av = g.adiag + pair * n;
        double *pout = g.partial + (((long)r * g.nl + (l - g.l0)) * g.tiles + tile) * n;
        for (int i0 = 0; i0 < n; i0 += 16) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int kc = 0; kc < npad; kc += KC_PANEL) {
                const int kn = min(KC_PANEL, npad - kc);         // a multiple of 4
                // beyond the LDS-resident limit: this panel's fragments of W are asked for before the panel is filled, so that they
                // arrive under the fill and its barriers (a row past the end repeats the last one; its panel row is zero)
                double afr[KC_PANEL / 4];
                if (!WRES) {
#pragma unroll
                    for (int j = 0; j < KC_PANEL / 4; ++j) afr[j] = Wr[(long)min(kc + 4 * j + fq, n - 1) * T + tw];
                }
                __syncthreads();                                 // the previous panel (and wsum) has been read
                {
                    const int i = i0 + pi;
                    for (int kk = pk; kk < kn; kk += 16) {
                        const int k = kc + kk;
                        panel[kk * PANEL_LD + pi] = (i < n && k < n) ? Ur[(long)i * n + k] * dt[k] : 0.0;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < KC_PANEL / 4; ++j) {
                    if (4 * j < kn) {                            // (wave-uniform)
                        const double a = WRES ? wl[((long)wid * npad + kc + 4 * j + fq) * 16 + fr] : afr[j];
                        const double b = panel[(4 * j + fq) * PANEL_LD + fr];
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                    }
                }
            }
            // epilogue: this lane holds electrode i0 + fr at the columns t0 + 16 wid + fq + 4 r4
            const int i = i0 + fr;
            double ss = 0.0;
            if (i < n) {
                const double ai = av[i];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int tt = t0 + wid * 16 + fq + 4 * r4;
                    if (tt < T) {
                        const double e = acc[r4] / ai;
                        ss += e * e;
                    }
                }
            }
            ss += __shfl_xor(ss, 16, 64);                        // (commutative exchanges: every lane ends with the same bits)
            ss += __shfl_xor(ss, 32, 64);
            if (fq == 0) wsum[wid][fr] = ss;
            __syncthreads();
            if (tid < 16 && i0 + tid < n) pout[i0 + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
        }
    }
}

__global__ __launch_bounds__(256) void kcsd_fold_kernel(KcsdCvK g) {
    __shared__ double e[GPCSD_MAX_EIG_N];
    const int tid = threadIdx.x, bl = blockIdx.x, r = blockIdx.y, n = g.n;
    const long pair = (long)r * g.nlam + g.l0 + bl;
    if (g.status[pair]) {
        if (tid == 0) g.err[pair] = INFINITY;
        return;
    }
    const double *p = g.partial + ((long)r * g.nl + bl) * g.tiles * n;
    for (int i = tid; i < n; i += 256) {
        double s = 0.0;
        for (int t = 0; t < g.tiles; ++t) s += p[(long)t * n + i];
        e[i] = sqrt(s);
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < n; ++i) tot += e[i];
        g.err[pair] = tot;
    }
}

void k_kcsd_cv(gpcsd_ctx *c, const double *U, const double *s, const double *W, int n, int T, int nR, const double *lam, int nlam,
               double *err, int *status, hipStream_t st) {
    GP_REQUIRE(n > 0 && n <= GPCSD_MAX_EIG_N && T > 0 && nR > 0 && nlam > 0 && (long)nR * nlam <= 65535, -3, "kcsd_cv: bad problem");
    KcsdCvK k;
    k.U = U; k.s = s; k.W = W; k.lam = lam;
    k.n = n; k.T = T; k.nR = nR; k.nlam = nlam;
    k.tiles = ceil_div(T, 64);
    k.dtab = c->buf<double>("kcsd_dtab", (size_t)nR * nlam * n);
    k.adiag = c->buf<double>("kcsd_adiag", (size_t)nR * nlam * n);
    k.status = status;
    k.err = err;
    // lambda values per launch: the partial sums of a launch stay within a fixed budget (an entry does not depend on the grouping)
    const size_t per_lam = (size_t)nR * k.tiles * n * sizeof(double);
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)nlam, ((size_t)256 << 20) / per_lam));
    k.partial = c->buf<double>("kcsd_partial", (size_t)group * nR * k.tiles * n);
    k.l0 = 0; k.nl = nlam;
    {
        ProfScope ps(c, "kcsd_diag", 3.0 * (double)n * n * nR * nlam, st);
        hipLaunchKernelGGL(kcsd_diag_kernel, dim3(nlam, nR), dim3(256), 0, st, k);
        GP_HIP(hipGetLastError());
    }
    const int npad = (n + 3) & ~3;
    const bool wres = n <= KCSD_WRES_MAX_N;
    const size_t lds = wres ? (size_t)npad * 64 * sizeof(double) : 0;
    if (wres) {
        static PerDeviceOnce attr_once;
        if (attr_once.first())
            GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kcsd_cv_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       KCSD_WRES_MAX_N * 64 * (int)sizeof(double)));
    }
    for (int l0 = 0; l0 < nlam; l0 += group) {
        k.l0 = l0;
        k.nl = std::min(group, nlam - l0);
        {
            ProfScope ps(c, "kcsd_cv", 2.0 * (double)n * n * T * nR * k.nl, st);
            if (wres) hipLaunchKernelGGL(kcsd_cv_kernel<true>, dim3(k.tiles, nR), dim3(256), lds, st, k);
            else hipLaunchKernelGGL(kcsd_cv_kernel<false>, dim3(k.tiles, nR), dim3(256), 0, st, k);
            GP_HIP(hipGetLastError());
        }
        {
            ProfScope ps(c, "kcsd_fold", 0.0, st);
            hipLaunchKernelGGL(kcsd_fold_kernel, dim3(k.nl, nR), dim3(256), 0, st, k);
            GP_HIP(hipGetLastError());
        }
    }
}

// ---------------------------------------------------------------- the estimate's two scalings of the spectrum
// d[k] = 1 / (max(s_k, 0) + lambda), sd[k] = max(s_k, 0) d[k]; *status = 1 for a numerically singular pair (d and sd then hold zeros)
__global__ __launch_bounds__(256) void kcsd_scale_kernel(const double *__restrict__ s, int n, double lam, double *d, double *sd, int *status) {
    __shared__ int sing;
    const int tid = threadIdx.x;
    if (tid == 0) {
        double mn = INFINITY, mx = 0.0;
        for (int k = 0; k < n; ++k) {
            const double sk = fmax(s[k], 0.0);
            mn = fmin(mn, sk);
            mx = fmax(mx, sk);
        }
        sing = (!(mn + lam > 0.0) || mn + lam < (double)n * 0x1p-52 * mx) ? 1 : 0;
        *status = sing;
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
        const double sk = fmax(s[k], 0.0);
        const double dk = sing ? 0.0 : 1.0 / (sk + lam);
        d[k] = dk;
        sd[k] = sk * dk;
    }
}

void k_kcsd_scale(gpcsd_ctx *c, const double *s, int n, double lam, double *d, double *sd, int *status, hipStream_t st) {
    ProfScope ps(c, "kcsd_scale", 0.0, st);
    hipLaunchKernelGGL(kcsd_scale_kernel, dim3(1), dim3(256), 0, st, s, n, lam, d, sd, status);
    GP_HIP(hipGetLastError());
}

// out[k][t] = d[k] W[k][t]
__global__ __launch_bounds__(256) void kcsd_rowscale_kernel(const double *__restrict__ W, const double *__restrict__ d, int n, long T,
                                                            double *__restrict__ out) {
    const long total = (long)n * T;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) out[i] = d[i / T] * W[i];
}

void k_kcsd_rowscale(gpcsd_ctx *c, const double *W, const double *d, int n, int T, double *out, hipStream_t st) {
    ProfScope ps(c, "kcsd_rowscale", 0.0, st);
    const unsigned nb = (unsigned)std::min<long>(((long)n * T + 255) / 256, 4096);
    hipLaunchKernelGGL(kcsd_rowscale_kernel, dim3(nb), dim3(256), 0, st, W, d, n, (long)T, out);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
