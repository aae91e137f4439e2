// Power spectrum, cross-spectrum and coherence of a field on the device (gfx950, v_mfma_f64_16x16x4_f64): what the reference's analysis
// scripts do on the host with scipy.signal.periodogram(..., axis=1) and a mean over the trials (auditory_lfp/fit_gpcsd_baseline.py:189-195,
// neuropixels/fit_gpcsd2d.py:120-128).
//
//   power_kernel         X[z][j][m] = sum_t A[j][t] x[z][t][m]  ->  |X|^2 (epilogue)  ->  per-tile sums over the trials, in trial order
//   power_reduce_kernel  psd[z][j][s] = 1/R (sum of a site's tile sums, in tile order)
//   coherence_kernel     coh[a][b] = |Sx[a][b]|^2 / (Sx[a][a] Sx[b][b]),  0 where the denominator is 0
//
// Every step of a periodogram of fixed length is linear except the final modulus (window, detrend, zero-padded FFT, scaling): ONE
// complex matrix A (utility_functions.spectral_operator builds it on the host; keeping a frequency keeps a row).  The product is the
// one of analytic_kernel (phase.hip) with the same tiles and LDS conventions -- 256 threads = four waves of 16 x 16 fragments, a
// workgroup owns 32 rows x 64 columns, K tiles of 16 register-staged global -> LDS and double-buffered with one barrier per tile,
// [o][k] tiles with a row stride of BK + 2 and [k][o] tiles with BO + 16, a row or column past the end reads the last valid one, the
// last K tile is zero-masked in LDS -- written out again here and not shared: analytic_kernel's outputs keep their bits whatever
// this file becomes.  The cross-spectral matrix is plv_kernel (phase.hip), unchanged, on the stored coefficients:
// Sx[s][j][a][b] = 1/R sum_r X_a conj(X_b), which is scipy.signal.csd(x_b, x_a) averaged over the trials (SciPy conjugates its FIRST
// argument) -- the orientation of the PLV's phase_a - phase_b.
//
// The reduction over the trials.  Columns c = z M + m run over ALL sites (M = R S, m = r S + s, the draw index innermost; S = 1 for a
// prediction), so a short M does not leave the multiplier's columns empty; a 64-column tile then holds parts of several sites, and a
// site several tiles.  Each workgroup writes |X|^2 of its tile to LDS and sums, for every (site, draw) it holds, the trials of its
// tile in increasing r: one partial per (z, j, s, tile of the site), slot k = tile - first tile of the site, at most
// ceil((M - 1) / 64) + 1 slots.  power_reduce_kernel adds the slots that were written (it works out which from the same geometry; a
// tile that holds no column of a (site, draw) leaves its slot alone) in increasing k and divides by R.  No floating-point atomics,
// a fixed order throughout: the same call gives the same bits, with or without the optional per-trial outputs.
#include <algorithm>
#include <type_traits>

#include "kernels.hpp"

namespace gpcsd {

typedef double d4 __attribute__((ext_vector_type(4)));
// fragment reads as volatile LDS loads: keeps them ds_read_b64 (64 banks) instead of fused ds_read2_b64 (gemm_f64.hip)
typedef const volatile double __attribute__((address_space(3))) *lds_frag_ptr;
#define LDS_FRAG(p) (*(lds_frag_ptr)(p))

namespace {
constexpr int NT = 256, BK = 16;
constexpr int LD_OK = BK + 2;      // row stride of an [o][k] tile
constexpr int PAD_KO = 16;         // an [k][o] tile's rows are BO + 16 doubles apart
constexpr int BJ = 32, BN = 64;    // rows (frequencies) and columns ((site, trial, draw)) of a workgroup
constexpr int LD_P = BN + 1;       // row stride of the |X|^2 tile: the reduction's lanes run along the rows
}  // namespace

int power_slots(long M) { return (int)((M - 1 + BN - 1) / BN) + 1; }

struct PowerK {
    const double *X;             // [z][t][m]
    const double *Are, *Aim;     // [nrow][nts] row-major
    int nts, nrow, M, R, S;
    long ncol;                   // nz * M
    double *part;                // [z][j][s][slot]
    int nslot;
    double *power, *re, *im;     // [z][j][m] each; nullptr: not stored
    int tiles_j;
};

__global__ __launch_bounds__(256) void power_kernel(PowerK g) {
    constexpr int A_ELEMS = 2 * BJ * LD_OK;          // rows [0, BJ): A_re, [BJ, 2 BJ): A_im
    constexpr int X_ELEMS = BK * (BN + PAD_KO);
    constexpr int PA = 2 * BJ * BK / NT, PX = BN * BK / NT;
    __shared__ double lds[2 * (A_ELEMS + X_ELEMS)];
    static_assert(BJ * LD_P <= 2 * (A_ELEMS + X_ELEMS), "the |X|^2 tile reuses the operand tiles");
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int tile_j = blockIdx.x % g.tiles_j;
    const long tile_c = blockIdx.x / g.tiles_j;
    const int j0 = tile_j * BJ;
    const long n0 = tile_c * BN;
    const int K = g.nts;

    d4 are[2], aim[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) are[f] = aim[f] = d4{0.0, 0.0, 0.0, 0.0};

    // operand slots of this thread.  A: (row oa + 16 i, k = ka), 16 consecutive k of a row per 16 lanes; X: (k = kx + 4 i, column ox),
    // 64 consecutive columns per wave
    const int ka = tid & 15, oa = tid >> 4;
    const int ox = tid & 63, kx = tid >> 6;
    // A: 32-bit byte offsets from a wave-uniform base (the host side checks that the operator fits); the first PA / 2 slots are rows
    // of A_re, the others of A_im.  X: one 64-bit pointer per thread (its column's plane), advanced per tile.
    unsigned offA[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int jj = j0 + (oa + 16 * i) % BJ;
        offA[i] = (unsigned)(((long)(jj < g.nrow ? jj : g.nrow - 1) * K + ka) * 8);
    }
    const double *px;
    {
        const long c = n0 + ox < g.ncol ? n0 + ox : g.ncol - 1;
        const long z = c / g.M;
        px = g.X + z * (long)K * g.M + (c - z * g.M) + (long)kx * g.M;
    }
    const long xstep = 4L * g.M;
    double ra[PA], rx[PX];
    auto load_full = [&](int t) {
        const char *const bre = reinterpret_cast<const char *>(g.Are + t * BK), *const bim = reinterpret_cast<const char *>(g.Aim + t * BK);
#pragma unroll
        for (int i = 0; i < PA; ++i) ra[i] = *reinterpret_cast<const double *>((i < PA / 2 ? bre : bim) + offA[i]);
        const double *p = px + (long)t * BK * g.M;
#pragma unroll
        for (int i = 0; i < PX; ++i) rx[i] = p[i * xstep];
    };
    auto load_tail = [&](int t) {                  // partial K tile: an index past the end reads the last valid one (zeroed by the store)
        const int k0 = t * BK;
        const int dk = (k0 + ka < K ? k0 + ka : K - 1) - ka;
#pragma unroll
        for (int i = 0; i < PA; ++i)
            ra[i] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>((i < PA / 2 ? g.Are : g.Aim) + dk) + offA[i]);
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int kq = k0 + kx + 4 * i < K ? k0 + kx + 4 * i : K - 1;
            rx[i] = px[(long)(kq - kx) * g.M];
        }
    };
    double *const swA = lds + oa * LD_OK + ka, *const swX = lds + 2 * A_ELEMS + kx * (BN + PAD_KO) + ox;
    auto store = [&](auto bufc, int kleft) {       // kleft >= BK: a full tile (the comparisons fold away when inlined with a constant)
        constexpr int buf = decltype(bufc)::value;
#pragma unroll
        for (int i = 0; i < PA; ++i) swA[buf * A_ELEMS + 16 * i * LD_OK] = ka < kleft ? ra[i] : 0.0;
#pragma unroll
        for (int i = 0; i < PX; ++i) swX[buf * X_ELEMS + 4 * i * (BN + PAD_KO)] = kx + 4 * i < kleft ? rx[i] : 0.0;
    };
    const double *const srA = lds + (wr * 16 + fr) * LD_OK + fq;
    const double *const srX = lds + 2 * A_ELEMS + fq * (BN + PAD_KO) + wc * 16 + fr;
    auto mma = [&](auto bufc, int steps) {
        constexpr int buf = decltype(bufc)::value;
        const double *sa = srA + buf * A_ELEMS, *sx = srX + buf * X_ELEMS;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk < steps) {                      // wave-uniform: the all-zero steps of a partial last tile are skipped
                const double a_re = LDS_FRAG(sa + kk * 4), a_im = LDS_FRAG(sa + BJ * LD_OK + kk * 4);
                double b[2];
#pragma unroll
                for (int f = 0; f < 2; ++f) b[f] = LDS_FRAG(sx + (kk * 4) * (BN + PAD_KO) + f * 32);
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    are[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_re, b[f], are[f], 0, 0, 0);
                    aim[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_im, b[f], aim[f], 0, 0, 0);
                }
            }
        }
    };
    using Buf0 = std::integral_constant<int, 0>;
    using Buf1 = std::integral_constant<int, 1>;
    const int nk = (K + BK - 1) / BK, nfull = K / BK;
    const int last_steps = (K - (nk - 1) * BK + 3) / 4;
    auto load_any = [&](int t) {
        if (t < nfull) load_full(t);
        else load_tail(t);
    };
    load_any(0);
    store(Buf0{}, K);
    __syncthreads();
    // steady state as the GEMM core's: two full K tiles per trip (the buffer index is a compile-time constant), in the order
    // loads | MFMAs | LDS stores, one barrier per tile
    int t = 0;
    for (; t + 2 < nfull; t += 2) {
        load_full(t + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(Buf0{}, BK / 4);
        __builtin_amdgcn_sched_barrier(0);
        store(Buf1{}, BK);
        __syncthreads();
        load_full(t + 2);
        __builtin_amdgcn_sched_barrier(0);
        mma(Buf1{}, BK / 4);
        __builtin_amdgcn_sched_barrier(0);
        store(Buf0{}, BK);
        __syncthreads();
    }
    // tile t sits in buffer 0 and at most two more follow (the last one possibly partial)
    if (t + 1 < nk) {
        load_any(t + 1);
        mma(Buf0{}, BK / 4);
        store(Buf1{}, K - (t + 1) * BK);
        __syncthreads();
        if (t + 2 < nk) {
            load_any(t + 2);
            mma(Buf1{}, BK / 4);
            store(Buf0{}, K - (t + 2) * BK);
            __syncthreads();
            mma(Buf0{}, last_steps);
        } else {
            mma(Buf1{}, last_steps);
        }
    } else {
        mma(Buf0{}, last_steps);
    }

    // ---- epilogue 1: lane (fq, fr) of fragment f holds Re and Im of rows j0 + 16 wr + fq + 4 r, column n0 + 32 f + 16 wc + fr.
    // |X|^2 of the whole tile goes to LDS (over the operand tiles: every wave has left the K loop), the optional outputs to memory.
    __syncthreads();
    double *const P = lds;
    const long plane = (long)g.nrow * g.M;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int cc = f * 32 + wc * 16 + fr;
        const long c = n0 + cc;
        const bool col_ok = c < g.ncol;
        const long z = (col_ok ? c : g.ncol - 1) / g.M;
        const long base = z * plane + (c - z * g.M);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jj = wr * 16 + fq + 4 * r;
            const double re = are[f][r], im = aim[f][r];
            const double p = re * re + im * im;
            P[jj * LD_P + cc] = p;                 // (a clamped row or column: computed from valid data, never read below)
            if (!col_ok || j0 + jj >= g.nrow) continue;
            const long o = base + (long)(j0 + jj) * g.M;
            if (g.power) g.power[o] = p;           // (wave-uniform tests)
            if (g.re) g.re[o] = re;
            if (g.im) g.im[o] = im;
        }
    }
    __syncthreads();

    // ---- epilogue 2: the trials of every (site, draw) of this tile, in increasing r.  Thread (jj, q) owns row jj and the columns
    // q, q + 8, ...; a column leads its (site, draw) when no earlier column of the tile belongs to it (r == 0, or cc < S), and the
    // leader adds the columns cc, cc + S, ... up to the site's last trial or the tile's end.
    // (one division per thread -- ncol < 2^31 -- then the site z and the offset w in it follow the columns by stepping)
    const int jj = tid & 31, q = tid >> 5;
    if (j0 + jj < g.nrow && n0 + q < g.ncol) {
        const unsigned M = (unsigned)g.M, S = (unsigned)g.S;
        unsigned z = (unsigned)(n0 + q) / M;
        unsigned w = (unsigned)(n0 + q) - z * M;
        for (int cc = q; cc < BN && n0 + cc < g.ncol; cc += 8) {
            if (w < S || (unsigned)cc < S) {
                const unsigned r = w / S, s = w - r * S;
                double sum = 0.0;
                for (long r2 = r, c2 = cc; r2 < g.R && c2 < BN; ++r2, c2 += S) sum += P[jj * LD_P + c2];
                const long slot = tile_c - (long)(z * M / BN);
                g.part[(((long)z * g.nrow + (j0 + jj)) * g.S + s) * g.nslot + slot] = sum;
            }
            w += 8;
            while (w >= M) {
                w -= M;
                ++z;
            }
        }
    }
}

// psd[z][j][s] = 1/R (the partial sums of (z, j, s), in tile order).  Slot k of site z is column tile z M / 64 + k; it was written
// iff that tile holds a column of (z, ., s): with [lo, hi) the tile's share of the site's columns, the first trial at or after lo
// that has draw s lies before hi.  Only those slots are read (the buffer is not cleared).
__global__ __launch_bounds__(256) void power_reduce_kernel(const double *part, double *psd, long n, int nrow, int M, int S, int nslot, double R) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long z = i / ((long)nrow * S);
    const int s = (int)(i % S);
    const long c0 = z * M, first = c0 / BN;                // the site's first column and first tile
    const double *p = part + i * nslot;
    double sum = 0.0;
    for (int k = 0; k < nslot; ++k) {
        const long t0 = (first + k) * BN;
        const int lo = (int)((t0 > c0 ? t0 : c0) - c0), hi = (int)((t0 + BN < c0 + M ? t0 + BN : c0 + M) - c0);
        if (hi <= lo) break;                               // past the site's last tile
        const int w = lo <= s ? s : lo + (S - 1 - (lo - s - 1) % S);      // the first offset >= lo that is s modulo S
        if (w < hi) sum += p[k];
    }
    psd[i] = sum / R;
}

void k_power(gpcsd_ctx *c, const PowerDesc &d, hipStream_t s) {
    GP_REQUIRE(d.X && d.Are && d.Aim && d.part && d.psd && d.nz > 0 && d.nts > 0 && d.R > 0 && d.S > 0 && d.nrow > 0, -3, "power: empty problem");
    const long M = (long)d.R * d.S, ncol = (long)d.nz * M;
    const int tiles_j = ceil_div(d.nrow, BJ);
    const long tiles_c = (ncol + BN - 1) / BN;
    const int nslot = power_slots(M);
    const long nout = (long)d.nz * d.nrow * d.S;
    GP_REQUIRE(M < (1L << 31) && ncol < (1L << 31) && tiles_c * tiles_j < (1L << 31) && nout / 256 < (1L << 31) - 1, GPCSD_ERR_CAPACITY,
               "power: too many columns or tiles");
    // (the kernel's 32-bit byte offsets span the operator)
    GP_REQUIRE((long)d.nrow * d.nts < (1L << 28), GPCSD_ERR_CAPACITY, "power: an operator of %d x %d exceeds 2^28 entries", d.nrow, d.nts);
    ProfScope ps(c, "power", 4.0 * (double)ncol * d.nrow * d.nts, s);
    PowerK k;
    k.X = d.X; k.Are = d.Are; k.Aim = d.Aim;
    k.nts = d.nts; k.nrow = d.nrow; k.M = (int)M; k.R = d.R; k.S = d.S; k.ncol = ncol;
    k.part = d.part; k.nslot = nslot;
    k.power = d.power; k.re = d.re; k.im = d.im;
    k.tiles_j = tiles_j;
    hipLaunchKernelGGL(power_kernel, dim3((unsigned)(tiles_c * tiles_j)), dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(power_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, (const double *)d.part, d.psd, nout, d.nrow,
                       (int)M, d.S, nslot, (double)d.R);
    GP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------------
// Magnitude-squared coherence from the cross-spectral matrices Sx = sre + i sim, nmat matrices of nz x nz (plv_kernel's layout
// [s][j][a][b]): coh[a][b] = (sre^2 + sim^2) / (sre[a][a] sre[b][b]), 0 where that product is 0 (an all-zero site).  sre is symmetric
// and sim antisymmetric bit for bit, the product of the two diagonal entries commutes: coh is symmetric bit for bit, its diagonal 1.
__global__ __launch_bounds__(256) void coherence_kernel(const double *sre, const double *sim, double *coh, int nz, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long nn = (long)nz * nz;
    const long mat = i / nn, rem = i - mat * nn;
    const long a = rem / nz, b = rem - a * nz;
    const double den = sre[mat * nn + a * (nz + 1)] * sre[mat * nn + b * (nz + 1)];
    const double re = sre[i], im = sim[i];
    const double num = re * re + im * im;
    coh[i] = den > 0.0 ? num / den : 0.0;
}

void k_coherence(gpcsd_ctx *c, const double *sre, const double *sim, double *coh, int nz, long nmat, hipStream_t s) {
    GP_REQUIRE(sre && sim && coh && nz > 0 && nmat > 0, -3, "coherence: empty problem");
    const long total = nmat * nz * nz;
    GP_REQUIRE(total / 256 < (1L << 31) - 1, GPCSD_ERR_CAPACITY, "coherence: too many entries");
    ProfScope ps(c, "coherence", 6.0 * (double)total, s);
    hipLaunchKernelGGL(coherence_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sre, sim, coh, nz, total);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
