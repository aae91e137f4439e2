// Band phase and phase-locking value on the device (gfx950, v_mfma_f64_16x16x4_f64): the step every analysis of a CSD estimate
// ends with -- band-pass along time, analytic signal, phase at a few times, phase locking over the trials.
//
//   analytic_kernel   Re/Im[z][j][m] = sum_t A_re/A_im[j][t] X[z][t][m]  ->  amp = hypot, phase = atan2, unit phasor   (epilogue)
//   plv_kernel        c[s][j][a][b] = 1/R sum_r u[a][j][r][s] conj(u[b][j][r][s]), plv = |c|   (lower tiles + their mirror images)
//
// Band-pass (filtfilt / sosfiltfilt) followed by the Hilbert transform along a time axis of fixed length is ONE complex matrix A
// (utility_functions.analytic_operator builds it on the host); keeping a few times keeps those rows of A.  Both kernels follow
// the conventions of the GEMM core (gemm_f64.hip): 256 threads = four waves of 16 x 16 fragments, K tiles of 16 (8 for the PLV), operand tiles
// register-staged global -> LDS and double-buffered with one barrier per K tile, [o][k] tiles with a row stride of BK + 2 and
// [k][o] tiles with BO + 16 (conflict-free ds_read_b64 fragment reads), a row or column past the end reads the last valid one
// (its accumulators are never stored), the last K tile is zero-masked in LDS.  Fragment maps (cdna_hip_programming.md section 3):
// A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15], C/D lane l reg r holds C[(l >> 4) + 4 r][l & 15].
// Unlike the core they address their operands with 64-bit per-thread pointers (the columns of the analytic product run over
// (site, trial) pairs of different planes, the phasors of one (time, draw) are a strided slice): nothing limits an operand's size.
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
}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// Analytic signal of every (site, trial) column, amplitude / phase / unit phasor in the epilogue.
//
// The transposed product, as gemm_pred_at_kernel: rows = kept times j, columns = (z, m) with m the innermost index of the input
// and of the outputs, so the lanes of a wave run along m and a store instruction writes 16 consecutive m (128 bytes) of four
// times.  The columns run over ALL planes (column c = z M + m reads X + z nts M + m with stride M along t): a short m -- five
// trials, one trial -- does not leave the multiplier's columns empty.  A workgroup owns 32 times x 64 columns; wave (wr, wc)
// holds, for each of its two column fragments, the accumulators of A_re and of A_im fed by the SAME X fragment: Re and Im of one
// (j, m) sit in one lane and the epilogue is register arithmetic -- no complex scratch, no second pass.
struct AnalyticK {
    const double *X;             // [z][t][m]
    const double *Are, *Aim;     // [nsel][nts] row-major
    int nts, nsel, M;
    long ncol;                   // nz * M
    double *phase, *amp, *ure, *uim;     // [z][j][m] each; nullptr: not stored
    int tiles_j;
};

__global__ __launch_bounds__(256) void analytic_kernel(AnalyticK g) {
    // FJ = row fragments (of A_re and of A_im each) per wave.  Two -- 64 times per workgroup, 8 MFMAs per 6 fragment reads -- measured
    // SLOWER at 384 x 500 x 50 with all times kept (0.418 against 0.368 ms): 57 KB of LDS leave two workgroups per CU instead of four.
    constexpr int FJ = 1;
    constexpr int BJ = 32 * FJ, BN = 64;
    constexpr int A_ELEMS = 2 * BJ * LD_OK;          // rows [0, BJ): A_re, [BJ, 2 BJ): A_im
    constexpr int X_ELEMS = BK * (BN + PAD_KO);
    constexpr int PA = 2 * BJ * BK / NT, PX = BN * BK / NT;
    __shared__ double lds[2 * (A_ELEMS + X_ELEMS)];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int tile_j = blockIdx.x % g.tiles_j;
    const long tile_c = blockIdx.x / g.tiles_j;
    const int j0 = tile_j * BJ;
    const long n0 = tile_c * BN;
    const int K = g.nts;

    d4 are[FJ][2], aim[FJ][2];
#pragma unroll
    for (int i = 0; i < FJ; ++i)
#pragma unroll
        for (int f = 0; f < 2; ++f) are[i][f] = aim[i][f] = d4{0.0, 0.0, 0.0, 0.0};

    // operand slots of this thread.  A: (row oa + 16 i, k = ka), 16 consecutive k of a row per 16 lanes; X: (k = kx + 4 i, column ox),
    // 64 consecutive columns per wave
    const int ka = tid & 15, oa = tid >> 4;
    const int ox = tid & 63, kx = tid >> 6;
    // A: 32-bit byte offsets from a wave-uniform base (the operator is small: the host side checks it fits), so a full tile's loads
    // are `global_load_dwordx2 v, v_off, s[base]` with the tile's advance on the scalar unit; the first PA / 2 slots are rows of
    // A_re, the others of A_im.  X: one 64-bit pointer per thread (its column's plane), advanced per tile.
    unsigned offA[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int jj = j0 + (oa + 16 * i) % BJ;
        offA[i] = (unsigned)(((long)(jj < g.nsel ? jj : g.nsel - 1) * K + ka) * 8);
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
                double a_re[FJ], a_im[FJ], b[2];
#pragma unroll
                for (int i = 0; i < FJ; ++i) {
                    a_re[i] = LDS_FRAG(sa + (i * 32) * LD_OK + kk * 4);
                    a_im[i] = LDS_FRAG(sa + (BJ + i * 32) * LD_OK + kk * 4);
                }
#pragma unroll
                for (int f = 0; f < 2; ++f) b[f] = LDS_FRAG(sx + (kk * 4) * (BN + PAD_KO) + f * 32);
#pragma unroll
                for (int i = 0; i < FJ; ++i)
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        are[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_re[i], b[f], are[i][f], 0, 0, 0);
                        aim[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_im[i], b[f], aim[i][f], 0, 0, 0);
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

    // ---- epilogue: lane (fq, fr) of fragment (i, f) holds Re and Im of times j0 + 32 i + 16 wr + fq + 4 r, column n0 + 32 f + 16 wc + fr
    const long plane = (long)g.nsel * g.M;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const long c = n0 + f * 32 + wc * 16 + fr;
        if (c >= g.ncol) continue;
        const long z = c / g.M;
        const long base = z * plane + (c - z * g.M);
#pragma unroll
        for (int i = 0; i < FJ; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + i * 32 + wr * 16 + fq + 4 * r;
                if (j >= g.nsel) continue;
                const long o = base + (long)j * g.M;
                const double re = are[i][f][r], im = aim[i][f][r];
                const double amp = hypot(re, im);
                // amp == 0: the phasor is (1, 0) and the phase 0, whatever the signs of the zeros (np.angle / np.exp of a zero)
                const bool nonzero = amp > 0.0;
                if (g.amp) g.amp[o] = amp;                                        // (wave-uniform tests)
                if (g.phase) g.phase[o] = nonzero ? atan2(im, re) : 0.0;
                if (g.ure) g.ure[o] = nonzero ? re / amp : 1.0;
                if (g.uim) g.uim[o] = nonzero ? im / amp : 0.0;
            }
    }
}

void k_analytic(gpcsd_ctx *c, const AnalyticDesc &d, hipStream_t s) {
    GP_REQUIRE(d.X && d.Are && d.Aim && d.nz > 0 && d.nts > 0 && d.M > 0 && d.nsel > 0, -3, "analytic: empty problem");
    const long ncol = (long)d.nz * d.M;
    const int tiles_j = ceil_div(d.nsel, 32);
    const long tiles_c = (ncol + 63) / 64;
    GP_REQUIRE(ncol < (1L << 31) && tiles_c * tiles_j < (1L << 31), GPCSD_ERR_CAPACITY, "analytic: too many columns or tiles");
    // (the kernel's 32-bit byte offsets span the operator)
    GP_REQUIRE((long)d.nsel * d.nts < (1L << 28), GPCSD_ERR_CAPACITY, "analytic: an operator of %d x %d exceeds 2^28 entries", d.nsel, d.nts);
    ProfScope ps(c, "analytic", 4.0 * (double)ncol * d.nsel * d.nts, s);
    AnalyticK k;
    k.X = d.X; k.Are = d.Are; k.Aim = d.Aim;
    k.nts = d.nts; k.nsel = d.nsel; k.M = (int)d.M; k.ncol = ncol;
    k.phase = d.phase; k.amp = d.amp; k.ure = d.ure; k.uim = d.uim;
    k.tiles_j = tiles_j;
    const dim3 grid((unsigned)(tiles_c * tiles_j));
    hipLaunchKernelGGL(analytic_kernel, grid, dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------------------------
// Phase-locking value of all site pairs: for every (draw s, time j) the complex mean resultant of u_a conj(u_b) over the R trials,
//   c_re[a][b] = 1/R sum_r (re_a re_b + im_a im_b),   c_im[a][b] = 1/R sum_r (im_a re_b - re_a im_b),   plv = hypot(c_re, c_im).
//
// A Hermitian rank-R product per (s, j): the phasors of one (s, j) are the nz x R matrix with rows nsel R S apart and trials S apart
// (S = 1: the posterior mean's layout; S > 1: the draw index innermost, sample_posterior's layout -- the loads are then strided, and
// s is the fastest index of the grid so that the S workgroups that share every cache line they touch run together).  A workgroup
// owns one 64 x 64 tile ON OR BELOW the diagonal: four waves of 2 x 2 fragments, two accumulator sets, four real MFMA products per
// k step (re re + im im -> c_re; im re + (-re) im -> c_im).  Every entry strictly below the diagonal is stored together with its
// mirror image FROM THE SAME REGISTERS (c_im negated), the diagonal's c_im is the exact zero it is: plv and c_re are symmetric and
// c_im antisymmetric bit for bit.  Sums run over r in index order, no atomics: the same call gives the same bits.
struct PlvK {
    const double *ure, *uim;     // [z][j][r][s]
    int nz, nsel, R, S;
    double *cre, *cim, *plv;     // [s][j][a][b]; nullptr: not stored
    int npairs;                  // tiles on or below the diagonal
};

__global__ __launch_bounds__(256) void plv_kernel(PlvK g) {
    // K tiles of 8: four operand tiles, double-buffered, in 40 KB (rows 10 doubles apart: 10 i mod 32 are 16 distinct even slots)
    constexpr int BO = 64, BK = 8, LD_OK = BK + 2;
    constexpr int T_ELEMS = BO * LD_OK;              // one [o][k] tile
    constexpr int PT = BO * BK / NT;
    __shared__ double lds[2 * 4 * T_ELEMS];          // per buffer: re_a, im_a, re_b, im_b
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int s = blockIdx.x % g.S;
    const int rest = blockIdx.x / g.S;
    const int pair = rest % g.npairs, j = rest / g.npairs;
    int ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= pair) ++ta;    // (a handful of tiles per side)
    const int tb = pair - ta * (ta + 1) / 2;
    const int a0 = ta * BO, b0 = tb * BO;
    const int K = g.R;

    d4 cre[2][2], cim[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int f = 0; f < 2; ++f) cre[i][f] = cim[i][f] = d4{0.0, 0.0, 0.0, 0.0};

    // slots: (row o + 32 i, k), the 8 k of a row on 8 neighbouring lanes
    const int kt = tid & 7, o = tid >> 3;
    const long row_stride = (long)g.nsel * g.R * g.S;
    const long js = (long)j * g.R * g.S + s;
    long offa[PT], offb[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const int ra = a0 + o + 32 * i, rb = b0 + o + 32 * i;
        offa[i] = (long)(ra < g.nz ? ra : g.nz - 1) * row_stride + js;
        offb[i] = (long)(rb < g.nz ? rb : g.nz - 1) * row_stride + js;
    }
    double r_ra[PT], r_ia[PT], r_rb[PT], r_ib[PT];
    auto load = [&](int t) {
        const int kk = t * BK + kt < K ? t * BK + kt : K - 1;
        const long ko = (long)kk * g.S;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            r_ra[i] = g.ure[offa[i] + ko];
            r_ia[i] = g.uim[offa[i] + ko];
            r_rb[i] = g.ure[offb[i] + ko];
            r_ib[i] = g.uim[offb[i] + ko];
        }
    };
    auto store = [&](int buf, int t) {
        const bool ok = kt < K - t * BK;
        double *p = lds + buf * 4 * T_ELEMS + o * LD_OK + kt;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            p[32 * i * LD_OK] = ok ? r_ra[i] : 0.0;
            p[T_ELEMS + 32 * i * LD_OK] = ok ? r_ia[i] : 0.0;
            p[2 * T_ELEMS + 32 * i * LD_OK] = ok ? r_rb[i] : 0.0;
            p[3 * T_ELEMS + 32 * i * LD_OK] = ok ? r_ib[i] : 0.0;
        }
    };
    auto mma = [&](int buf, int steps) {
        const double *sa = lds + buf * 4 * T_ELEMS + (wr * 32 + fr) * LD_OK + fq;
        const double *sb = lds + buf * 4 * T_ELEMS + 2 * T_ELEMS + (wc * 32 + fr) * LD_OK + fq;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk < steps) {                      // wave-uniform
                double are[2], aim[2], bre[2], bim[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    are[i] = LDS_FRAG(sa + i * 16 * LD_OK + kk * 4);
                    aim[i] = LDS_FRAG(sa + T_ELEMS + i * 16 * LD_OK + kk * 4);
                    bre[i] = LDS_FRAG(sb + i * 16 * LD_OK + kk * 4);
                    bim[i] = LDS_FRAG(sb + T_ELEMS + i * 16 * LD_OK + kk * 4);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        cre[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(are[i], bre[f], cre[i][f], 0, 0, 0);
                        cre[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim[i], bim[f], cre[i][f], 0, 0, 0);
                        cim[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim[i], bre[f], cim[i][f], 0, 0, 0);
                        cim[i][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(-are[i], bim[f], cim[i][f], 0, 0, 0);
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

    // ---- epilogue: entry (a, b) with a >= b and its mirror image from the same registers
    const long nn = (long)g.nz * g.nz;
    const long out0 = ((long)s * g.nsel + j) * nn;
    const double Rd = (double)g.R;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int b = b0 + wc * 32 + f * 16 + fr;
        if (b >= g.nz) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = a0 + wr * 32 + i * 16 + fq + 4 * r;
                if (a >= g.nz || a < b) continue;              // (a < b: the diagonal tile's upper half, written by its mirror)
                const double vre = cre[i][f][r] / Rd;
                const double vim = a == b ? 0.0 : cim[i][f][r] / Rd;
                const double vabs = hypot(vre, vim);
                const long lo = out0 + (long)a * g.nz + b, up = out0 + (long)b * g.nz + a;
                if (g.cre) g.cre[lo] = vre;
                if (g.cim) g.cim[lo] = vim;
                if (g.plv) g.plv[lo] = vabs;
                if (a != b) {
                    if (g.cre) g.cre[up] = vre;
                    if (g.cim) g.cim[up] = -vim;
                    if (g.plv) g.plv[up] = vabs;
                }
            }
    }
}

void k_plv(gpcsd_ctx *c, const PlvDesc &d, hipStream_t s) {
    GP_REQUIRE(d.ure && d.uim && d.nz > 0 && d.nsel > 0 && d.R > 0 && d.S > 0, -3, "plv: empty problem");
    const long T = (d.nz + 63) / 64, npairs = T * (T + 1) / 2;
    const long nblocks = npairs * d.nsel * d.S;
    GP_REQUIRE(T < (1L << 15) && nblocks < (1L << 31), GPCSD_ERR_CAPACITY, "plv: too many tiles");
    ProfScope ps(c, "plv", 4.0 * (double)d.nz * d.nz * d.R * d.nsel * d.S, s);
    PlvK k;
    k.ure = d.ure; k.uim = d.uim;
    k.nz = d.nz; k.nsel = d.nsel; k.R = d.R; k.S = d.S;
    k.cre = d.cre; k.cim = d.cim; k.plv = d.plv;
    k.npairs = (int)npairs;
    hipLaunchKernelGGL(plv_kernel, dim3((unsigned)nblocks), dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
