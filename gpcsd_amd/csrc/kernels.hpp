// Device-pointer launchers shared between translation units of libgpcsd_hip.so.
#pragma once
#include <functional>
#include "ctx.hpp"

namespace gpcsd {

// ---------------------------------------------------------------- fp64 MFMA GEMM core
enum Epi : int {
    EPI_STORE = 0,   // C = alpha * acc
    EPI_DIV_D = 1,   // C = acc * D[(row / rdiv) * ldd + col]   with D = the RECIPROCALS 1/D_xi (k_build_D's Dinv)
    EPI_QUAD = 2,    // no store; partial sums of acc^2 * D[...] (reciprocals; deterministic two-stage reduce)
    EPI_ACCUM = 3,   // C += alpha * acc
    EPI_GRAD = 4,    // b = acc * D (reciprocals): C = b, C2 = b*colscale[col], C3 = b*rowscale[row/rdiv]; sums of acc*b and b*b
    EPI_DUAL_INIT = 6, // C = alpha*acc and C2 = alpha*acc (first term of a running sum).  NOT instantiated any more (dropped with the
                       // other unused variants): gemm_f64 refuses it with -3; the number stays reserved
    EPI_SUB = 7        // C = C - acc with C read at the START of the tile (accumulators initialised to -C, plain-store epilogue with
                       // alpha = -1): the rank-k trailing updates of the Cholesky -- EPI_ACCUM's read-modify-write sits at the end
                       // of a tile, where nothing hides its latency.  A (M,K) row-major, B stored (N,K) only.
};

struct GemmDesc {
    int M = 0, N = 0, K = 0;
    const double *A = nullptr;
    long lda = 0;
    bool transA = false;   // false: A is (M,K) row-major; true: A stored (K,M) row-major
    const double *B = nullptr;
    long ldb = 0;
    bool transB = false;   // false: B is (K,N) row-major; true: B stored (N,K) row-major
    double *C = nullptr;
    long ldc = 0;
    double *C2 = nullptr;  // EPI_GRAD
    double *C3 = nullptr;  // EPI_GRAD
    const double *colscale = nullptr, *rowscale = nullptr;   // EPI_GRAD; EPI_STORE: optional C = alpha*acc*colscale[col]
    long sColscale = 0;                                      // batch stride of colscale (EPI_STORE)
    // optional scaling of operand A along the contracted index: C = (A diag(kscale)) B, applied to A's tile on its way to LDS
    // (one rounded product per element: the same bits as a pre-scaled copy of A, without writing and re-reading that copy)
    const double *kscale = nullptr;
    long sKscale = 0, sKscale2 = 0;                          // batch strides
    int batch = 1;
    long sA = 0, sB = 0, sC = 0;
    // second (outer) batch level: entry z = z2 * batch + z1 adds z2 * s?2 to the operand bases.  Used to run the same
    // product for several hyper-parameter sets (replicas) whose buffers sit a fixed stride apart.
    int batch2 = 1;
    long sA2 = 0, sB2 = 0, sC2 = 0, sD2 = 0, sColscale2 = 0, sRowscale2 = 0, sDyn2 = 0;
    long sQuad2 = 0;              // EPI_QUAD / EPI_GRAD: quad_out of outer entry z2 is quad_out + z2 * sQuad2
    double alpha = 1.0;
    int epi = EPI_STORE;
    const double *D = nullptr;
    int rdiv = 1;
    long ldd = 0;
    long sD = 0;                  // batch stride of D
    double *quad_out = nullptr;   // EPI_QUAD: one double (EPI_GRAD: two), written by the final reduce
    const double *extra_sum_in = nullptr;   // EPI_QUAD: an unrelated vector of partials summed by the same reduce launch
    int extra_sum_n = 0;                     //   (sum_small_kernel's association: bit-identical to k_build_D's own sum)
    double *extra_sum_out = nullptr;
    const int *dyn = nullptr;     // device int per batch entry: effective N = K = dyn[batch] (tiles beyond it exit)
    bool lower = false;           // square symmetric update (C and its mirror image equal): tiles strictly above the diagonal exit at once
    int lower_shift = 0;          // ... of a launch that covers rows lower_shift.. of such an update (row i of C is row lower_shift + i)
    int prio = 0;                 // 1: the launch's waves run at raised issue priority (small products of a dependent chain that share
                                  // their CUs with another stream's flood of tiles: Cholesky's diagonal chain)
    int cfg = 0;                  // 0 = choose the tile configuration automatically, 1 / 2 / 3 / 5 = force (see gemm_f64.hip)
    const char *prof_name = "gemm_f64";
};

int gemm_auto_cfg(int M, int N, int K, int batch);      // the configuration gemm_f64 picks for a plain product when GemmDesc::cfg == 0
void gemm_f64(gpcsd_ctx *c, const GemmDesc &g, hipStream_t s = nullptr);

// Last product of a folded prediction with the unfold, the (r, t) -> (t, r) relayout and the sum over components fused into
// its epilogue (gemm_f64.hip: gemm_pred_unfold_kernel).  S~ [(zq, r)][nt]; Pcat_tp [K_tp][C * npP_tp], tp = time parity.
struct PredUnfoldDesc {
    const double *S;
    long lds;
    const double *Pc[2];
    long ldp[2];
    int npP[2], K[2], kcol0[2];
    int nb, nba;                    // time orbits (symmetric block); those with an antisymmetric partner
    long ncolS, ncolA, anti_row0;   // (site orbit, trial) columns of the symmetric / antisymmetric site block; first anti row of S~
    int R, nt, C;
    SymDev sz, st;
    double *list;
    long list_stride;
    double *sum;
    long tile_c0 = 0, tile_c1 = -1;     // column tiles (32 columns (site orbit, trial) each) of this launch; tile_c1 < 0: all
};
constexpr int PRED_UNFOLD_BN = 32;      // columns (site orbit, trial) per tile of the fused last product
bool gemm_pred_unfold_supported(int C, long nrows_S, int nt);
void gemm_pred_unfold(gpcsd_ctx *c, const PredUnfoldDesc &d, hipStream_t s);

// Last product of a prediction at arbitrary times, written in the output layout with the component sum in its epilogue
// (gemm_f64.hip: gemm_pred_at_kernel): out[cc][z][j][r] = sum_i Pc[i][cc * nts + j] S[(z, r)][i], sum[z][j][r] = sum over cc.
struct PredAtDesc {
    const double *S;                // [(z, r)][K] row-major
    long lds;
    const double *Pc;               // [K][C * nts]
    long ldp;
    int K, nts, C, R;
    long ncol;                      // nz * R
    double *list;                   // (C, nz, nts, R) or nullptr
    long list_stride;
    double *sum;                    // (nz, nts, R)
};
void gemm_pred_at(gpcsd_ctx *c, const PredAtDesc &d, hipStream_t s);

// The two products of a posterior variance (gpcsd_predict_var; gemm_f64.hip: gemm_var_kernel), one operand squared on its way to
// LDS so that no squared copy exists in memory:
//   sq_a:  out[z][i] = sum_k A[z][k]^2 B[k][i]                                  (G = (M1 o M1) Dinv; C = 1, prior = nullptr)
//   else:  list[c][z][j] = prior[z] kd[c] - sum_k A[z][k] B[k][c * ncol + j]^2                                   c = 0..C-1
//          sum[z][j]     = prior[z] sum_c kd[c] - sum_k A[z][k] (sum_c B[k][c * ncol + j])^2     (the components are correlated)
//   pair:  out[p][i] = sum_k A[pair_a[p]][k] A[pair_b[p]][k] B[k][i]       (sq_a with gathered rows: the Gram blocks of gpcsd_cv_electrodes)
// prior == nullptr: the plain product is stored (no subtraction).  One launch: grid y = the C (+ 1 when sum != nullptr) planes.
struct VarDesc {
    const double *A = nullptr;      // [nrow][K] row-major
    long lda = 0;
    const double *B = nullptr;      // [K][C * ncol] row-major
    long ldb = 0;
    int nrow = 0, ncol = 0, K = 0, C = 1;
    bool sq_a = false;
    const int *pair_a = nullptr, *pair_b = nullptr;     // device [nrow] each, entries in [0, a_rows); sq_a stays false
    int a_rows = 0;                 // rows of A in the pair form
    const double *prior = nullptr;  // [nrow]
    double kd[GPCSD_MAX_TEMPORAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double *list = nullptr;         // (C, nrow, ncol)
    double *sum = nullptr;          // (nrow, ncol) or nullptr
    const char *prof_name = "gemm_var";
};
void gemm_var(gpcsd_ctx *c, const VarDesc &d, hipStream_t s);

// Last product of the leave-one-out scores (gpcsd_loo; gemm_f64.hip: gemm_loo_kernel) with everything that follows it in its
// epilogue: beta[(x, r)][t] = sum_i V[(x, r)][i] Qt[t][i] = (K^-1 y_r)[x, t] is never stored.  Per element, with c[x][t] the
// diagonal of K^-1 and y[(x, r)][t] the data in the resident row layout,
//   e = beta / c                          (the leave-one-out residual y - loo_mean)
//   mean[x][t][r] = y - e                 (optional; the reference's (nx, nt, ntrials) layout)
//   lpd[(x, r)] = sum_t 1/2 log c - 1/2 beta e - 1/2 log 2 pi,      sse[(x, r)] = sum_t e^2
// The two row sums are deterministic: registers, the four lane groups of a wave, the two waves of a tile's time half through LDS,
// then one partial per time tile and row in `partials` ([2][tiles_t][nrow]), added in tile order by a second small launch.
struct LooDesc {
    const double *V = nullptr;      // [(x, r)][K] row-major
    long ldv = 0;
    const double *Qt = nullptr;     // [nt][K] row-major
    long ldq = 0;
    const double *c = nullptr;      // [nx][nt]
    const double *y = nullptr;      // [(x, r)][nt]
    int K = 0, nt = 0, R = 0;
    long nrow = 0;                  // nx * R
    double *mean = nullptr;         // (nx, nt, R) or nullptr
    double *lpd = nullptr, *sse = nullptr;      // [nrow] each
};
void gemm_loo(gpcsd_ctx *c, const LooDesc &d, hipStream_t s);
void k_loo_var(gpcsd_ctx *c, const double *cdiag, double *var, long n, hipStream_t s);      // var = 1 / cdiag elementwise

// ---------------------------------------------------------------- leave-electrodes-out cross-validation (efold.hip)
// Factor and solve of the blocks G_j = (K^-1)_FF of every fold F and temporal eigen-index j (gpcsd_cv_electrodes): Cholesky, log det,
// diag(G_j^-1) and e = G_j^-1 u for every trial, with the sums over j of log det, u^T e and e^2 formed in a fixed order.  Folds in
// CSR form; row0[fold] = first row of the fold's packed lower triangle in Gp (rows i (i + 1) / 2 + k, k <= i, in fold order),
// mem_fold[m] = the fold of member m of fold_idx.  Outputs indexed by ELECTRODE: pdiag[a][j], sse[a][r], E[(a, r)][j] (rows of
// electrodes in no fold are not written); lpd[fold][r]; status[fold] = 1 where some G_j lost positive definiteness (NaN outputs).
struct EfoldDesc {
    const double *Gp = nullptr;     // [rows][nt]
    const double *V = nullptr;      // [(x, r)][nt]
    const int *fold_ptr = nullptr, *fold_idx = nullptr, *row0 = nullptr, *mem_fold = nullptr;      // device
    int nfolds = 0, nt = 0, R = 0;
    double *E = nullptr;            // [(x, r)][nt] or nullptr
    double *pdiag = nullptr;        // [nx][nt]
    double *lpd = nullptr;          // [nfolds][R]
    double *sse = nullptr;          // [nx][R]
    int *status = nullptr;          // [nfolds]
    double *partials = nullptr;     // efold_partials() doubles of scratch
    double *part_ld = nullptr, *part_q = nullptr, *part_sse = nullptr;      // (set by efold_solve)
};
long efold_partials(const EfoldDesc &d, int nmem);
void efold_solve(gpcsd_ctx *c, EfoldDesc d, const int *h_fold_ptr, hipStream_t s);

// ---------------------------------------------------------------- band phase and phase locking (phase.hip)
// Analytic signal of X[z][t][m] under the complex operator A = Are + i Aim (nsel, nts) -- band-pass + Hilbert along t as one matrix,
// rows = the kept times -- with its nonlinear functions in the epilogue: Re/Im[z][j][m] = sum_t Are/Aim[j][t] X[z][t][m] (never
// stored), amp = hypot(Re, Im), phase = atan2(Im, Re), unit phasor (Re, Im) / amp; amp == 0 gives phase 0 and phasor (1, 0).
// Outputs in the layout [z][j][m]; a null output is not stored.
struct AnalyticDesc {
    const double *X = nullptr;      // (nz, nts, M)
    int nz = 0, nts = 0;
    long M = 0;
    const double *Are = nullptr, *Aim = nullptr;      // (nsel, nts) row-major
    int nsel = 0;
    double *phase = nullptr, *amp = nullptr, *ure = nullptr, *uim = nullptr;
};
void k_analytic(gpcsd_ctx *c, const AnalyticDesc &d, hipStream_t s);
// Complex mean resultant over the R trials and its modulus for all site pairs, per (draw s, time j), phasors u = ure + i uim in the
// layout (nz, nsel, R, S):  cre + i cim = 1/R sum_r u_a conj(u_b),  plv = |.|; outputs (S, nsel, nz, nz), a null one is not stored.
// Hermitian bit for bit (lower tiles computed, mirror images written from the same registers); fixed summation order, no atomics.
struct PlvDesc {
    const double *ure = nullptr, *uim = nullptr;
    int nz = 0, nsel = 0, R = 0, S = 1;
    double *cre = nullptr, *cim = nullptr, *plv = nullptr;
};
void k_plv(gpcsd_ctx *c, const PlvDesc &d, hipStream_t s);

// ---------------------------------------------------------------- power spectrum and coherence (spectrum.hip)
// Coefficients X[z][j][m] = sum_t (Are + i Aim)[j][t] x[z][t][m] of the field x (nz, nts, R, S) under a spectral operator (nrow, nts),
// m = r S + s with the draw index innermost, and the power averaged over the trials: psd[z][j][s] = 1/R sum_r |X[z][j][r S + s]|^2,
// summed in a fixed order through per-tile partial sums (part: nz nrow S power_slots(R S) doubles of scratch), no atomics.  The
// per-trial outputs power = |X|^2, re, im, each (nz, nrow, R, S), are optional: a null one is not stored.
struct PowerDesc {
    const double *X = nullptr;      // (nz, nts, R, S)
    int nz = 0, nts = 0, R = 0, S = 1;
    const double *Are = nullptr, *Aim = nullptr;      // (nrow, nts) row-major
    int nrow = 0;
    double *part = nullptr, *psd = nullptr;
    double *power = nullptr, *re = nullptr, *im = nullptr;
};
int power_slots(long M);
void k_power(gpcsd_ctx *c, const PowerDesc &d, hipStream_t s);
// coh = (sre^2 + sim^2) / (sre[a][a] sre[b][b]) for nmat Hermitian nz x nz matrices in k_plv's layout; 0 where the denominator is 0;
// symmetric bit for bit when sre is symmetric and sim antisymmetric bit for bit
void k_coherence(gpcsd_ctx *c, const double *sre, const double *sim, double *coh, int nz, long nmat, hipStream_t s);

// ---------------------------------------------------------------- phase-difference torus graph (torus.hip)
// d nodes, N trials; node a's phasors are ure / uim [off[a] .. off[a] + N) (off: device table, so a strided slice of the resident
// phasors and a dense (d, N) upload are one code path); pi / pj: device tables of the P = d (d - 1) / 2 pairs (i < j) in the order
// of np.triu_indices(d, 1).  m = 2 P parameters in the interleaved order (2p: cos, 2p + 1: sin).
constexpr int TG_MAX_NODES = 128;
constexpr int TG_REPS_PER_WG = 4;          // replicates that share the operand tiles of a node-Gram workgroup
constexpr double TG_PIVOT_TOL = 64.0;      // a pivot below TG_PIVOT_TOL m u of its diagonal entry is a failed pivot
struct TgDesc {
    const double *ure = nullptr, *uim = nullptr;
    const long *off = nullptr;
    const int *pi = nullptr, *pj = nullptr;
    int d = 0, N = 0;
};
// G[rep][a] (nv x nv, nv = 2 d - 1, lower part) = 1/W sum_n w[rep][n] v_n(a) v_n(a)^T on MFMA; w == nullptr: unit weights
void k_tg_node_gram(gpcsd_ctx *c, const TgDesc &t, const double *w, const double *W, int nrep, double *G, hipStream_t s);
// Gamma[rep] (m x m, symmetric bit for bit, exact zeros between pairs without a common node) and H[rep] (m) gathered from G
void k_tg_assemble(gpcsd_ctx *c, const TgDesc &t, const double *G, int nrep, double *Gamma, double *H, hipStream_t s);
void k_tg_diag_save(gpcsd_ctx *c, const double *Gamma, int m, int nrep, double *dg, hipStream_t s);
// status = first pivot (+ 1) of the factor L whose square is not above TG_PIVOT_TOL m u dg[pivot], merged with potrf's own report
void k_tg_pivot_check(gpcsd_ctx *c, const double *L, const double *dg, int m, int *status, hipStream_t s);
// R (m x N) = D_n (D_n^T phi) - 2 S_n per trial; g (d x N) scratch
void k_tg_residuals(gpcsd_ctx *c, const TgDesc &t, const double *phi, double *g, double *R, hipStream_t s);
// chi2[p] = phi_p^T Sigma_pp^-1 phi_p with Sigma_pp = 1/W^2 sum_n w_n z_n z_n^T over rows 2p, 2p + 1 of Z (m x N)
void k_tg_chi2(gpcsd_ctx *c, const double *Z, const double *w, const double *phi, int P, int N, double W, double *chi2, hipStream_t s);

// ---------------------------------------------------------------- kernel CSD, 1D, Gaussian sources (kcsd.hip)
constexpr int KCSD_WRES_MAX_N = 256;       // electrodes up to which a workgroup of kcsd_cv_kernel keeps its 64 columns of W in LDS
// out (M, npts): which == 0 the potential basis b_j(pts[p]) (two-panel Gauss-Legendre, nodes gx / weights gw on [-1, 1], summed in
// node order), which == 1 the source basis g(pts[p] - src[j]); sigma_b = R / 3
void k_kcsd_basis(gpcsd_ctx *c, const double *src, int M, const double *pts, int npts, double R, double h, double varsigma,
                  const double *gx, const double *gw, int ngl, int which, double *out, hipStream_t s);
// err[r][l] = sum_i sqrt(sum_t (beta_it / a_ii)^2) with beta = U_r diag(1 / (s_r + lam_l)) W_r, a_ii = sum_k U_ik^2 / (s_k + lam_l);
// U (nR, n, n) eigenvectors in columns, s (nR, n), W (nR, n, T), lam (nlam): device arrays.  status[r][l] = 1 and err = +inf for a
// numerically singular pair.  beta is never stored; fixed summation order.
void k_kcsd_cv(gpcsd_ctx *c, const double *U, const double *s, const double *W, int n, int T, int nR, const double *lam, int nlam,
               double *err, int *status, hipStream_t st);
// d[k] = 1 / (max(s_k, 0) + lam), sd[k] = max(s_k, 0) d[k]; *status = 1 (and zeros) for a numerically singular pair
void k_kcsd_scale(gpcsd_ctx *c, const double *s, int n, double lam, double *d, double *sd, int *status, hipStream_t st);
void k_kcsd_rowscale(gpcsd_ctx *c, const double *W, const double *d, int n, int T, double *out, hipStream_t st);      // out[k][t] = d[k] W[k][t]

// ---------------------------------------------------------------- missing samples (masked.hip)
// The grouped, K-scaled symmetric product G = (A^-1)_MM of m missing samples sorted by time, then electrode, cut into strips of up
// to MASKED_STRIP samples of one time group; a tile is MASKED_TILE_STRIPS x MASKED_TILE_STRIPS strips.  One launch covers the tile
// rows [t0, t1) and every tile column on or below the diagonal:
//   G[p][q] = sum_a Qs[xi[p]][a] Qs[xi[q]][a] H[a][grp(p) - gA][grp(q)],   p >= q, and its mirror image from the same register.
constexpr int MASKED_STRIP = 16, MASKED_TILE_STRIPS = 4;
struct MaskedGramDesc {
    const double *Qs = nullptr;     // (nx, nx) row-major
    int nx = 0;
    const int *xi = nullptr;        // [m] electrode of sample p
    const int *s_off = nullptr, *s_cnt = nullptr, *s_grp = nullptr;      // strips, padded with empty ones to a multiple of 4
    const double *H = nullptr;      // [a][g - gA][g'], g' < ldh
    long sH = 0, ldh = 0;
    int gA = 0;
    int t0 = 0, t1 = 0;
    int m = 0;
    double *G = nullptr;            // (m, m)
};
void k_masked_gram(gpcsd_ctx *c, const MaskedGramDesc &d, hipStream_t s);
void k_gather_rows(gpcsd_ctx *c, const double *Q, int n, const int *rows, int nr, double *out, hipStream_t s);     // out[j] = Q[rows[j]]
// out[x][r][t] = mask[x][t][r] ? y[x][r][t] : 0 (a selection); mask (nx, nt, MT) bytes, MT == 1: one mask for all R trials
void k_mask_fill(gpcsd_ctx *c, const double *y, const unsigned char *mask, int MT, int nx, int R, int nt, double *out, hipStream_t s);
// out[r] = sum over the observed samples of trial r of y V (both [x][r][t]), in a fixed order
void k_mask_dot(gpcsd_ctx *c, const double *y, const double *V, const unsigned char *mask, int MT, int nx, int R, int nt, double *out,
                hipStream_t s);
// C[p][k] = V[xi[p]][trial[k]][ti[p]]  and  U[xi[p]][slot[k]][ti[p]] = -X[p][k] (U of na slots), p < m, k < nr
void k_mask_gather(gpcsd_ctx *c, const double *V, const int *xi, const int *ti, int m, const int *trial, int nr, int R, int nt, double *C,
                   hipStream_t s);
void k_mask_scatter(gpcsd_ctx *c, const double *X, const int *xi, const int *ti, int m, const int *slot, int nr, int na, int nt, double *U,
                    hipStream_t s);
void k_mask_colsumsq(gpcsd_ctx *c, const double *Z, int m, int nr, const int *trial, double *out, hipStream_t s);   // out[trial[k]] = |Z[:, k]|^2
void k_mask_add(gpcsd_ctx *c, double *B, const double *B2, const int *trial, int nx, int R, int na, int nt, hipStream_t s);

// ---------------------------------------------------------------- batched hyper-parameter sets
// Device image of gpcsd_hparams for batched evaluations (gpcsd_loglik_grad_batch): one entry per hyper-parameter set.  The
// Gram builders / derivative kernels take an optional table: with `tab` they run once for all B sets (the set index is a grid
// dimension, scalars come from tab[set], outputs are `s_out` apart), without it they are the single-set kernels as before.
struct HpDev {
    double R, eps, ell_s[2];
    int ncomp;
    int kind[GPCSD_MAX_TEMPORAL];
    double ell_t[GPCSD_MAX_TEMPORAL], sigma2_t[GPCSD_MAX_TEMPORAL];
    double sig2n, jitter;
    __host__ __device__ double ell_of(int c) const { return ell_t[c]; }          // (the accessors TemporalSet has too: kernels
    __host__ __device__ double sigma2_of(int c) const { return sigma2_t[c]; }    //  templated on the parameter source)
};

// ---------------------------------------------------------------- elementwise / Gram builders (gram.hip)
void k_b_fwd_1d(gpcsd_ctx *c, const double *r, long n, double R, double *out, hipStream_t s);
void k_second_diff(gpcsd_ctx *c, const double *in, long n_outer, long n_axis, long n_inner, double edge, double *out, hipStream_t s);
void k_b_fwd_2d(gpcsd_ctx *c, const double *d1, const double *d2, const double *w, long n, double R, double eps,
                double *out, hipStream_t s);
// out(n,m) = sum_c sigma2_c k_c(t_i - tp_j); ncomp components fused (K1-K3 of SURVEY 2a)
void k_temporal_gram(gpcsd_ctx *c, int ncomp, const int *kind, const double *ell, const double *sigma2,
                     const double *t, int n, const double *tp, int m, double *out, hipStream_t s, const HpDev *tab = nullptr,
                     int B = 1, long s_out = 0);
// A(nx, G) = gl_w[g] * b_fwd_1d(gl_x[g] - x[i], R)
void k_fwd_weights_1d(gpcsd_ctx *c, const double *x, int nx, const double *gl_x, const double *gl_w, int ngl, double R,
                      double *A, hipStream_t s, const HpDev *tab = nullptr, int B = 1, long s_out = 0);
// A(nx, G=ngl1*ngl2) = w1[g1] w2[g2] * b_fwd_2d(|gl - x|)
void k_fwd_weights_2d(gpcsd_ctx *c, const double *xy, int nx, const double *gx1, const double *gw1, int ngl1,
                      const double *gx2, const double *gw2, int ngl2, double R, double eps, double *A, hipStream_t s,
                      const HpDev *tab = nullptr, int B = 1, long s_out = 0);
// SE kernel between two 1D point sets: out(n,m) = exp(-0.5 ((a_i - b_j)/ell)^2)
void k_se_1d(gpcsd_ctx *c, const double *a, int n, const double *b, int m, double ell, double *out, hipStream_t s,
             const HpDev *tab = nullptr, int B = 1, long s_out = 0);
// anisotropic SE between two 2D point sets given as separate coordinate generators:
// point i of set A = (a1[i / na2], a2[i % na2]) if na2 > 0 (tensor grid) else (a[2i], a[2i+1]) (explicit list)
void k_se_2d(gpcsd_ctx *c, const double *a1, const double *a2, int na, int na2, const double *b1, const double *b2,
             int nb, int nb2, double ell1, double ell2, double *out, hipStream_t s, const HpDev *tab = nullptr, int B = 1,
             long s_out = 0);
// one axis factor of the tensor-grid SE kernel: out(n,n) = exp(-0.5 (a_i - a_j)^2 / ell^2)
void k_se_axis(gpcsd_ctx *c, const double *a, int n, double ell, double *out, hipStream_t s);
// ... and with its derivative w.r.t. the length scale, for the B sets of a batched evaluation (ell = tab[set].ell_s[axis])
void k_se_axis_tab(gpcsd_ctx *c, const double *a, int n, int axis, const HpDev *tab, int B, double *K, double *dK, hipStream_t s);
// Log-likelihood pieces in the basis U (x) Q (gram.hip): with Kt_p = amax_p Q_p T_p Q_p^T (T_p tridiagonal: d_p, e_p) the
// block of Ks (x) Kt + sig2 I of spatial eigen-row x' and temporal parity p is Q_p (es[x'] amax_p T_p + sig2 I) Q_p^T;
// *out_sumlog = sum of the log pivots of all these tridiagonal matrices (= sum log D), *out_quad = sum over the rows w of
// W = U^T Y Q ([x'][r][t~], rows of nt) of w^T (.)^-1 w by one forward recurrence each.  No temporal eigenvectors.
// host_slot (pinned, device-accessible) != null: the final sums' launch also writes {sum log D, quadratic form} to host_slot[0..1]
// and the status_doubles doubles at status_src to host_slot + status_at -- returns true when it did (the caller then skips its copy)
// variant: 0 = the launcher's choice (the scan kernel for blocks of at most 256 columns unless GPCSD_LL_PIVOT_SCAN=0), 1 = the
// serial-pivot kernel, 2 = the scan kernel (-3 for a wider block); the per-item partials stay in the ctx buffer "ll_tridiag_partials"
bool k_ll_tridiag(gpcsd_ctx *c, const double *W, const double *es, const double *const d[2], const double *const e[2],
                  const double *const amax[2], const double *sig, int nx, int R, int nt, const int np[2], const int c0[2],
                  double *out_sumlog, double *out_quad, hipStream_t s, double *host_slot = nullptr, const double *status_src = nullptr,
                  int status_at = 0, int status_doubles = 0, int variant = 0);
// The same systems solved: B[x'][r][p block] = (es[x'] amax_p T_p + sig2 I)^-1 W[x'][r][p block] (B may be W).  The posterior mean
// in the basis U (x) Q -- what (W V) / D is in the basis U (x) V -- without the temporal eigenvectors.
// k_tridiag_solve_pass: trials per pass of the kernel for column blocks of up to npmax (its z lives in LDS); 0 = unsupported.
// pass: 0 = the launcher's choice (GPCSD_TS_P, then the caller's hint -- PredCall::solve_pass --, then the trial count), 32 or 64 = that form.
int k_tridiag_solve_pass(int npmax, int R);
void k_tridiag_solve(gpcsd_ctx *c, const double *W, double *B, const double *es, const double *const d[2], const double *const e[2],
                     const double *const amax[2], const double *sig, int nx, int R, int nt, const int np[2], const int c0[2],
                     hipStream_t s, int pass = 0, int hint = 0);
void k_add_diag(gpcsd_ctx *c, double *A, int n, double v, hipStream_t s, const HpDev *tab = nullptr, int B = 1, long s_out = 0);
void k_shift_copy(gpcsd_ctx *c, const double *src, double *dst, int n, double v, hipStream_t s);     // dst = src + v
void k_sum_partials(gpcsd_ctx *c, double *out, const double *P, long n, int parts, hipStream_t s);
// out[z] = sum_g T[z][g] A[z][g] (rows of G doubles): the diagonal of T A^T, i.e. of compKphi at the points themselves when
// T = A Kgl (covariances.py:90,95 / :223,231) -- the prior variance of the potential at a prediction site
void k_rowdot(gpcsd_ctx *c, const double *T, const double *A, int n, int G, double *out, hipStream_t s);
// D[x*nt + i] = es[x]*et[i] + sig[x or 0]; also sumlog -> *sumlog_out (deterministic)
// with a table (B sets): scalar noise from tab[b].sig2n when nsig == 1, else set b's list at sig + b * nx
// Dinv (optional) = 1/D elementwise.  sumlog_out == nullptr: no final sum; the per-block partials stay in the ctx buffer
// "buildD_partials" and the return value is their count (a later launch may fold the sum in, or nobody needs it)
int k_build_D(gpcsd_ctx *c, const double *es, int nx, const double *et, int nt, const double *sig, int nsig, double *D,
              double *Dinv, double *sumlog_out, hipStream_t s, const HpDev *tab = nullptr, int B = 1, long s_sumlog = 0);
// lfp host layout [x][t][r] -> device layout [x][r][t] (and back for predictions [z][r][t] -> [z][t][r])
void k_swap_last2(gpcsd_ctx *c, const double *in, double *out, int n0, int n1, int n2, hipStream_t s);
void k_fill(gpcsd_ctx *c, double *p, long n, double v, hipStream_t s);
// in[(z, r)][c*n2 + t] (C components side by side) -> list[c][z][t][r] (optional) and sum[z][t][r] = sum_c
void k_swap_last2_sum(gpcsd_ctx *c, const double *in, int C, double *list, long list_stride, double *sum, int n0, int n1, int n2,
                      hipStream_t s);

// folded-basis helpers (gram.hip): rectangular fold of a covariance that commutes with the reflections of its row and
// column grids (out_ss: rs.ns x cs.ns, out_aa: rs.na x cs.na), the fold of the resident data in both indices, and the
// final pass of a folded prediction (unfold in site and time, (r, t) -> (t, r), sum over components)
void k_sym_fold_rect(gpcsd_ctx *c, const double *K, long ldk, const SymDev &rs, const SymDev &cs, double *out_ss, double *out_aa,
                     hipStream_t s);
// G (n,n) = F^T diag(Gss, Gaa) F for B sets (inputs s_in apart: Gss (ns,ns) followed by Gaa (na,na); outputs n*n apart)
void k_sym_unfold_mat(gpcsd_ctx *c, const double *Gf, long s_in, const SymDev &sy, int n, double *out, hipStream_t s, int B = 1);
void k_fold_lfp(gpcsd_ctx *c, const double *Y, int nx, int R, int nt, const SymDev &ss, const SymDev &st, double *out,
                hipStream_t s);
// nsP / naP > 0: the (parity, component) column blocks of `in` are padded to that many columns (128-byte aligned blocks)
void k_unfold_swap_sum(gpcsd_ctx *c, const double *in, int C, double *list, long list_stride, double *sum, int R, int nt,
                       const SymDev &sz, const SymDev &st, hipStream_t s, int nsP = 0, int naP = 0, long ldin = 0);

// ---------------------------------------------------------------- device normals and the passes of a posterior draw (rng.hip)
// out[k] = standard normal number first + k of stream `stream` under `seed`, k < count: Philox4x32-10 + Box-Muller in fp64
// (philox.hpp), a function of (seed, stream, index) alone
void k_normals(gpcsd_ctx *c, unsigned long long seed, unsigned stream, unsigned long long first, long count, double *out, hipStream_t s);
// out[x][q][t] = y[x][(p0 + q) / S][t] - phi[x][q][t] - eps[x][q][t], q < np: the residual of the pseudo-trials p0 .. p0 + np - 1
// (p = r S + s) in the layout the projection reads; y holds R trials as [x][r][t]; out may be phi
void k_sample_residual(gpcsd_ctx *c, const double *y, const double *phi, const double *eps, double *out, int nx, int nt, int R, long p0,
                       int np, int S, hipStream_t s);
// block (r0.., c0..) of the symmetric J (n, n) and its mirror image from src (nr, nc); a diagonal block from src's lower triangle
void k_sym_place(gpcsd_ctx *c, double *J, int n, int r0, int c0, const double *src, int nr, int nc, hipStream_t s);
// dsq = sqrt(diag J), dinv = 1 / dsq, J <- diag(dinv) J diag(dinv) (unit diagonal; symmetric in, symmetric out)
void k_sym_equilibrate(gpcsd_ctx *c, double *J, int n, double *dsq, double *dinv, hipStream_t s);
// F[i][k] = rowscale[i] Q[i][k] sqrt(max(w[k], 0)); rowscale may be null, nw == 1 broadcasts w[0]; F may be Q
void k_eig_factor(gpcsd_ctx *c, const double *Q, const double *w, int nw, const double *rowscale, double *F, int n, hipStream_t s);
// out[z][j][p0 + q] = upd[z][j][q] + prior[z][q][j], q < np, out rows of P pseudo-trials
void k_sample_combine(gpcsd_ctx *c, const double *upd, const double *prior, double *out, int nz, int nts, int np, long P, long p0,
                      hipStream_t s);

// ---------------------------------------------------------------- region features of a field (features.hip)
// The label map as lists, on the device: idx the flat indices i * nts + k of every labelled point, region after region and in
// row-major order inside a region; slice sl is entries [slice_beg[sl], + slice_cnt[sl]) of it, at most FEAT_SLICE of one region;
// region j (0-based) owns slices [reg_slice[j], reg_slice[j + 1]).  ptau / pz0 / pz1: the coordinates of entry n (k_feat_coords).
constexpr int FEAT_SLICE = 256;
struct FeatPlan {
    int J = 0, nslice = 0, npts = 0;
    const int *idx = nullptr, *slice_beg = nullptr, *slice_cnt = nullptr, *reg_slice = nullptr;
    const double *ptau = nullptr, *pz0 = nullptr, *pz1 = nullptr;
};
// feat[j][slot][col0 + p] (J, GPCSD_NFEAT, ldf) of the columns p < ncol of F[point][p] (row length ld), slots as gpcsd_region_features
// documents them.  mean (points, R) and isd (points), both or neither: slot 9 = max |F - mean[.][(col0 + p) / S]| isd, NaN without.
// part: scratch of nslice * GPCSD_NFEAT * ncol doubles.  Fixed order, no atomics; a column does not depend on the others.
struct FeatDesc {
    const double *F = nullptr;
    long ld = 0;
    int ncol = 0;
    long col0 = 0;
    const double *mean = nullptr, *isd = nullptr;
    int R = 0, S = 1;
    double *part = nullptr, *feat = nullptr;
    long ldf = 0;
};
void k_region_features(gpcsd_ctx *c, const FeatPlan &pl, const FeatDesc &d, hipStream_t s);
void k_feat_coords(gpcsd_ctx *c, const int *idx, int npts, int nts, const double *tau, const double *zeta, int dim, double *ptau,
                   double *pz0, double *pz1, hipStream_t s);
// isd = 1 / sqrt(var) where var > floor * max(var), 0 elsewhere; vmax: one double of scratch
void k_feat_isd(gpcsd_ctx *c, const double *var, long n, double floor, double *vmax, double *isd, hipStream_t s);

// ---------------------------------------------------------------- eigensolver (eigh.hip)
// Symmetric eigendecomposition of A (n,n) on device.  evals ascending; evecs (n,n) row-major with
// eigenvectors in COLUMNS (numpy.linalg.eigh convention).  A is destroyed.  status: device int (0 ok).
// claim_psd: the caller vouches that A is positive semi-definite (EighCall::claim_psd)
void eigh_device(gpcsd_ctx *c, double *A, int n, double *evals, double *evecs, int *d_status, hipStream_t s,
                 bool claim_psd = false);
constexpr int MAX_EIG_BATCH = 4;
// One CLASS of eigenproblems: `count` replicas of the same order n whose inputs / outputs sit a fixed stride apart
// (replica r reads A + r*sA, writes w + r*sw and Z + r*sZ).  The launches of a chain are shared by up to MAX_EIG_BATCH
// classes (the symmetric / antisymmetric halves of Ks and Kt) times any number of replicas (hyper-parameter sets of a
// batched evaluation): kernel arguments describe the classes by value, a workgroup derives its replica's pointers by
// adding replica * stride -- no per-problem table in the arguments or in memory.
struct EigReq {
    double *A;
    int n;
    double *w, *Z;
    const char *tag;
    int count = 1;
    long sA = 0, sw = 0, sZ = 0;
    bool prefilled = false;      // the scaled matrix is already in the class arena (eigh_arena_view): no scaling / copy pass
};
// Where the tridiagonalisation of class `tag` (order n, `count` replicas) expects its input: A0 = the matrix divided by
// *amax (replica r at A0 + r*blk, *amax at amax + r*blk), with the reflector storage V ((n + 64) x n) and tau (n + 64) zeroed.
// A caller that can generate the scaled matrix itself (k_temporal_fold_fill) writes it there and submits the class as
// `prefilled`, which takes the fold / absmax / scale launches out of the dependent chain.
struct EigArenaView {
    double *A0, *V, *tau, *amax;
    long blk;
    double *d, *e;               // the tridiagonal of A0 = Q T Q^T once the tridiagonalisation has run (n entries each)
    bool *psd;                   // host flag of the class (gpcsd_ctx::arena_psd): a fill that writes a positive semi-definite matrix sets it
};
int eigh_regtail_rows();         // rows of a whole problem the register tail (sytrd_regtail.hpp) holds: stage 5 applies up to here
EigArenaView eigh_arena_view(gpcsd_ctx *c, const char *tag, int n, int count);
// tags of the two half-size classes of problem `slot` (0 / 1) of eigh_pair_device: [0] symmetric, [1] antisymmetric
const char *const *eigh_fold_tags(const gpcsd_ctx *c, int slot);     // (slot 1: the tag set of the context's current generation, gpcsd_ctx::tgen)
// fold of a PSD matrix (+ diagonal shift per replica) straight into the class arenas, scaled: see eigh.hip
void k_psd_fold_fill(gpcsd_ctx *c, const double *K, int n, long sK, int nrep, const double *shift, const SymDev &sy,
                     const EigArenaView &as, const EigArenaView &aa, int *status, int status_stride, hipStream_t s,
                     const HpDev *tab = nullptr,        // tab: replica r adds tab[r].jitter instead of shift[r] (any nrep)
                     bool tab_shifts_nonneg = false);   // ... all of which are >= 0 (the arenas then count as PSD: EigArenaView::psd)
// The temporal chain's input in ONE launch: the symmetric / antisymmetric fold of Kt = sum_c sigma2_c k_c(t_i - t_j) for
// `nrep` hyper-parameter sets, evaluated entry by entry from the time grid (the same expressions, in the same order, as
// k_temporal_gram followed by the eigensolver's fold: tests/test_fold_kernels.py holds the two to the same bits), divided by a power of two >= 2 sum_c sigma2_c (>= every entry of
// either block) and written where the tridiagonalisation reads it (eigh_arena_view of the two half-size classes), reflector
// storage zeroed, *amax set.  Replaces temporal Gram -> fold -> absmax -> scale/copy/zero (five dependent launches).
// Non-finite entries are zeroed and reported in status[r * status_stride] (4), as the scaling pass does.
struct TemporalSet {
    int ncomp;
    int kind[GPCSD_MAX_TEMPORAL];
    double ell[GPCSD_MAX_TEMPORAL], sigma2[GPCSD_MAX_TEMPORAL];
    __host__ __device__ double ell_of(int c) const { return ell[c]; }
    __host__ __device__ double sigma2_of(int c) const { return sigma2[c]; }
};
void k_temporal_fold_fill(gpcsd_ctx *c, const TemporalSet *sets, int nrep, const double *t, int n, const SymDev &sy,
                          const EigArenaView &as, const EigArenaView &aa, int *status, int status_stride, hipStream_t s);
// ... for B sets from a device table of hyper-parameters (scale formed on the device by the same rule)
void k_temporal_fold_fill_tab(gpcsd_ctx *c, const HpDev *tab, int B, const double *t, int n, const SymDev &sy,
                              const EigArenaView &as, const EigArenaView &aa, int *status, int status_stride, hipStream_t s,
                              bool variances_nonneg);   // every sigma2 of the table is >= 0: the blocks are PSD (EigArenaView::psd)
// flat problem index g -> (class, replica) from the prefix sums start[0..MAX_EIG_BATCH] (unused classes repeat the total)
__device__ __forceinline__ void class_of(const int *start, int g, int &cls, int &rep) {
    cls = (g >= start[1]) + (g >= start[2]) + (g >= start[3]);
    rep = g - start[cls];
}
// Two independent problems at once (Ks and Kt of one likelihood evaluation): every stage is batched so they share
// launches; with a known symmetry each splits into two half-size problems first.  Everything a solve depends on travels in the
// request (and from there into the graph key, eigh.hip): nothing is read from switches set around the call.
struct EighSide {
    double *A = nullptr;             // (n, n) per replica, destroyed; replicas n*n apart (eigenvalues n apart, eigenvectors n*n apart)
    int n = 0;                       // <= 0: the side is absent
    double *w = nullptr, *Z = nullptr;
    const SymDev *sym = nullptr;
    int count = 0;                   // replicas; < 1: one for side 0, as many as side 0 for side 1
    bool prefolded = false;          // the folded halves are in their class arenas already, scaled (EigArenaView); A is not read
};
// what stage 5 hangs on every finished block of columns of Q: out[:, block] = in Q[:, block] on the main stream -- in / out (M rows
// of ld), the parity blocks' first columns, the replica whose Q it is.  in == nullptr: Q only.
struct QPipeX {
    const double *in = nullptr;
    double *out = nullptr;
    int M = 0, ld = 0, c0[2] = {0, 0}, rep = 0;
};
struct EighCall {
    EighSide side[2];                // [0] the first / spatial slot, [1] the second / temporal slot
    int *status = nullptr;           // replica r reports numerical failure in status[r * status_stride] (stride 0: one shared word)
    int status_stride = 0;
    // false: a caller that stays in the folded basis (eigh_fold_view) skips the unfold + rank merge of folded problems
    bool need_merged = true;
    // 0 = the whole solve.  Staged (capi.hip: TChain -- the log-likelihood's shifted tridiagonal systems need the temporal side only
    // as far as A / amax = Q T Q^T), same request every time:
    //   1 = the tridiagonalisation (chain stream);
    //   3 = the T factors of its reflector panels and the orthogonal factor Q itself (eigh_Q_view; T in EigArenaView::d / e) -- on
    //       ANY stream behind stage 1: it reads the reflectors, which stages 2 and 4 leave alone;
    //   2 = the divide & conquer of the tridiagonal matrix (chain stream, behind stage 1);
    //   4 = the back-transformation (chain stream, behind stage 2 AND stage 3: it needs the T factors);
    //   5 = stage 3 panel by panel beside a running stage 1 that publishes its progress, each block of columns followed by `x`.
    // Staged solves need folded (prefolded or not), tridiagonalisation-path problems within the fused back-transformation's size
    // (eigh_stageable).
    int stage = 0;
    bool progress = false;           // stage 1: the register tails publish their progress panel by panel (a stage 5 follows)
    bool claim_psd = false;          // the caller vouches that its matrices are positive semi-definite (gpcsd_eigh_psd)
    QPipeX x;                        // stage 5 only
};
void eigh_pair_device(gpcsd_ctx *c, const EighCall &r, hipStream_t s);
bool eigh_stageable(const SymDev *sy, int n);
// Q of class `tag` after stage 3: (n, n) row-major per replica, replicas n*n apart
double *eigh_Q_view(gpcsd_ctx *c, const char *tag, int n, int count);
// Half-size results of a symmetry-folded problem, in fold order (see eigh.hip); on == false: the problem is not folded.
struct FoldView {
    bool on = false;
    int ns = 0, na = 0;
    double *w = nullptr, *U = nullptr;      // w = (ws | wa);  U = (Us, ns x ns | Ua, na x na), eigenvectors in columns
    long sw = 0, sU = 0;                    // replica strides of w (= n) and U (= ns^2 + na^2)
};
FoldView eigh_fold_view(gpcsd_ctx *c, int slot, const SymDev *sy, int n, int count = 1);
// fused compact-WY back-transformation (wy.hip): all panels of all problems in two launches
struct WyProb {
    const double *V, *tau;   // reflectors by rows ((n + 64) x n, zero padded), tau (n + 64)
    double *T, *Z;           // T factors (npanels x 64 x 64 workspace), eigenvector matrix updated in place
    int n, npanels, nrefl;
    double *w_scale = nullptr;       // optional: eigenvalues of the SCALED matrix, multiplied by *amax in the apply launch
    const double *amax = nullptr;    // (saves the separate rescale launch at the end of the dependent chain)
    long blk = 0, sZ = 0, sw = 0;    // replica strides: V / tau / T / amax live in the class arena (blk), Z and w_scale are the caller's
    int z_identity = 0;              // the apply launch starts from Z = I (and writes Q itself): Z is only written
};
struct WyBatch {
    WyProb p[MAX_EIG_BATCH];         // one entry per class
    int start[MAX_EIG_BATCH + 1];    // prefix sums of the replica counts (see class_of)
    unsigned long long *clk = nullptr;   // measurement aid (GPCSD_WY_CLK=1): wall-clock stamps of workgroup (0, 0) at its phase boundaries
    int *status = nullptr;               // stage 5 (wy_q_pipeline): a gate whose time ran out reports 7 here (a scheduling miss: the
                                         // collecting call evaluates again, unpipelined -- gpcsd_ctx::q_pipe_timeouts)
    unsigned long long gate_ticks = 20000000ull;   // the gate's patience, 100 MHz ticks; 0: give up at once (test aid)
};
__device__ __forceinline__ WyProb wy_resolve(const WyBatch &b, int g) {
    int cls, rep;
    class_of(b.start, g, cls, rep);
    WyProb P = b.p[cls];
    const long o = rep * P.blk;
    P.V += o; P.tau += o; P.T += o;
    if (P.amax) P.amax += o;
    P.Z += rep * P.sZ;
    if (P.w_scale) P.w_scale += rep * P.sw;
    return P;
}
bool wy_fused_supported(int nmax);
// prep_done: the T factors were already formed by the D&C leaf launch (stedc_batch_device with a WyBatch)
void wy_batch_device(gpcsd_ctx *c, const WyBatch &b, int nclass, hipStream_t s, bool prep_done = false);
void wy_prep_device(gpcsd_ctx *c, const WyBatch &b, int nclass, hipStream_t s);     // the T factors only
// Q panel by panel behind the progress words of a register tail that is still running (wy.hip); chunk: the caller's work on the
// columns [col0[i], col1[i]) of class i's Q that the panel just applied completes
void wy_q_pipeline(gpcsd_ctx *c, const WyBatch &b, int nclass, hipStream_t s,
                   const std::function<void(const int *col0, const int *col1)> &chunk, bool one_launch = false);
// stages of the large-n solver, exposed for tests / diagnostics.  stedc_device expects the scale the solver works at -- the
// tridiagonal of A / max|a|, largest entry of order 1: the deflation tolerance 8 eps max(|d|, |z|) (dlaed2's, behind dstedc's own
// scaling) compares poles with entries of unit vectors, and a tridiagonal far below 1 deflates whole (gpcsd_debug_stedc scales)
void sytrd_device(gpcsd_ctx *c, double *A, int n, double *d, double *e, double *V, double *tau, hipStream_t s);
void stedc_device(gpcsd_ctx *c, const double *d, const double *e, int n, double *w, double *Z, int *d_status,
                  hipStream_t s, const char *tag);

// ---------------------------------------------------------------- analytic gradient pieces (grad.hip)
// a_x = sum_i et_i/D_xi, b_i = sum_x es_x/D_xi, s1 = sum 1/D
// B > 1: B hyper-parameter sets, every array contiguous per set (D nx*nt, es nx, et nt, a nx, b nt apart), s1 s_s1 apart
void k_D_sums(gpcsd_ctx *c, const double *D, const double *es, const double *et, int nx, int nt, double *a, double *b,
              double *s1_out, hipStream_t s, int B = 1, long s_s1 = 0);
// Ghs[y][x] += -1/2 (sig_y - sig_x)/(es_x - es_y) Ssum[x][y] for x != y, |es_x - es_y| > tiny
// B > 1: per hyper-parameter set (Ghs, Ssum nx*nx apart, es and sig nx apart)
void k_siglist_eigvec_term(gpcsd_ctx *c, double *Ghs, const double *Ssum, const double *es, const double *sig, int nx,
                           double tiny, hipStream_t s, int B = 1);
// out[b] = sum_{x,i} alpha[(x*nb + b)*nt + i]^2 / D[x*nt + i]
void k_per_trial_quad(gpcsd_ctx *c, const double *alpha, const double *D, int nx, int nb, int nt, double *out, hipStream_t s);
// out[x] = sum_k B[x*rowlen + k]^2
void k_rowgroup_sumsq(gpcsd_ctx *c, const double *B, int nrows, long rowlen, double *out, hipStream_t s);
// out (n,n) = scale * sum_b in[b*stride + e] + dscale * diag(dvec)
// B > 1: per hyper-parameter set, inputs s_in apart, dvec s_dvec apart (default n), out s_out apart (default n*n)
void k_batch_reduce(gpcsd_ctx *c, const double *in, int nb, long stride, int n, double scale, const double *dvec, double dscale,
                    double *out, hipStream_t s, int B = 1, long s_in = 0, long s_dvec = -1, long s_out = -1);
// out[2c] = <Gt, dKt/d ell_c>, out[2c+1] = <Gt, dKt/d sigma2_c>
// with a table: B sets (Gt nt*nt apart, outputs s_out apart); hp still supplies n_temporal
void k_temporal_grad(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *Gt, const double *t, int nt, double *out2C,
                     hipStream_t s, const HpDev *tab = nullptr, int B = 1, long s_out = 0);
// out[b][i * R + r] = in[b * s_in + i], i < n, r < R, b < B
void k_repeat_rows(gpcsd_ctx *c, const double *in, long s_in, int n, int R, int B, double *out, hipStream_t s);
// out[k] = <Gt, dK_k> for nm matrices dK_k (n2 doubles each, contiguous): user-defined temporal covariances
void k_frob_inner(gpcsd_ctx *c, const double *Gt, const double *dK, long n2, int nm, double *out, hipStream_t s);
// out[0..1] = <M, dKgl/d ell_1>, <M, dKgl/d ell_2>   (ngl2 == 0: 1D, only out[0] meaningful)
// out2[set * s_out + q] = <P, T_q>, q = 0, 1: the two spatial length-scale derivatives in the Kronecker form (grad.hip)
void k_frob_pair(gpcsd_ctx *c, const double *P, const double *T1, const double *T2, long n, double *out2, hipStream_t s, int B,
                 long s_out);
void k_kgl_grad(gpcsd_ctx *c, const double *M, const double *Kgl, const double *gx1, const double *gx2, int G, int ngl2,
                double ell1, double ell2, double *out2, hipStream_t s, const HpDev *tab = nullptr, int B = 1, long s_out = 0);
// out[0] = 2 <S, dA/dR>
void k_fwdR_grad(gpcsd_ctx *c, const double *S, const double *x, int nx, const double *gx1, const double *gw1, const double *gx2,
                 const double *gw2, int G, int ngl2, double R, double eps, double *out1, hipStream_t s, const HpDev *tab = nullptr,
                 int B = 1, long s_out = 0);

// ---------------------------------------------------------------- Cholesky (chol.hip)
// In-place lower Cholesky of A (n,n) row-major; strictly-upper part zeroed.  d_status: 0 ok, k+1 = pivot k <= 0 or NaN (the first
// such k, whichever block or look-ahead step meets it).  Only the lower triangle of A is read: whatever lies above the diagonal,
// NaN included, leaves the factor's bits unchanged (tests/test_chol_kernels.py).
void potrf_device(gpcsd_ctx *c, double *A, int n, int *d_status, hipStream_t s);
void potrf_diag128_probe(gpcsd_ctx *c, double *A, int n, double *X, int *d_status, unsigned long long *clk_dev, hipStream_t s);
// X = L^{-1} B in place (B (n,nrhs) row-major).  Both solves read the lower triangle of L only.
void trsm_lower_device(gpcsd_ctx *c, const double *L, int n, double *B, int nrhs, hipStream_t s);
// X = L^{-T} B in place (the transposed solve of the same factor; B (n,nrhs) row-major)
void trsm_lower_trans_device(gpcsd_ctx *c, const double *L, int n, double *B, int nrhs, hipStream_t s);
void logdet_chol_device(gpcsd_ctx *c, const double *L, int n, double *out, hipStream_t s);
void sumsq_device(gpcsd_ctx *c, const double *x, long n, double *out, hipStream_t s);

// ---------------------------------------------------------------- trial-shift objective and gradient (shift.hip)
// The tables of a plan and the B points (trial_b, tau_b) of one evaluation.  mu [x][c][k], c = 0 the background and c = i + 1
// component i; slope [i][x][k], k < nt - 1; lfp [x][trial][k]; lo, dt [b][i][k]; every field [x][b][k] (the flat GEMM layout).
struct ShiftDesc {
    int nx = 0, nt = 0, ntrials = 0, nseg = 0, B = 0;
    const double *t = nullptr, *mu = nullptr, *slope = nullptr, *lfp = nullptr, *D = nullptr;
    const int *trial = nullptr;      // [B]
    const double *tau = nullptr;     // [B][nseg]
    int *lo = nullptr;
    double *dt = nullptr;
    double mutau = 0.0, sigtau = 1.0;
};
constexpr int SHIFT_MAX_NSEG = 32;   // (= GPCSD_MAX_SHIFT_NSEG) the gradient kernel keeps one partial sum per component in registers
// slope[i][x][k] = (y_i[x][k+1] - y_i[x][k]) / (t[k+1] - t[k])
void k_shift_slopes(gpcsd_ctx *c, const double *mu, const double *t, int nx, int nt, int nseg, double *slope, hipStream_t s);
// lo = clip(searchsorted_left(t, t_k + tau_i), 1, nt - 1) - 1 and dt = (t_k + tau_i) - t_lo for every (b, i, k)
void k_shift_locate(gpcsd_ctx *c, const ShiftDesc &d, hipStream_t s);
// R[x][b][k] = lfp[x][trial_b][k] - (mu_0[x][k] + sum_i y_i[x][lo] + slope_i[x][lo] dt)
void k_shift_resid(gpcsd_ctx *c, const ShiftDesc &d, double *R, hipStream_t s);
// workgroups per point of the two reducing kernels (slabs of electrodes; a function of nx alone): the length of a point's partials
int shift_slabs(int nx);
// beta = alpha / D (not stored when beta == nullptr), f[b] = 1/2 sum alpha beta + 1/2 sum_i ((tau_i - mutau) / sigtau)^2;
// part: B * shift_slabs(nx) doubles of scratch
void k_shift_quad(gpcsd_ctx *c, const ShiftDesc &d, const double *alpha, double *beta, double *part, double *f, hipStream_t s);
// g[b][i] = -sum_{x,k} Z[x][b][k] slope_i[x][lo(b,i,k)] + (tau_i - mutau) / sigtau^2; part: B * shift_slabs(nx) * nseg doubles
void k_shift_grad(gpcsd_ctx *c, const ShiftDesc &d, const double *Z, double *part, double *g, hipStream_t s);

// ---------------------------------------------------------------- posterior of linear functionals (fungram.hip)
// The long-K scaled Gram: out[p][j][k] = sum_b sum_i A_p[b][j][i] s[b][i] B[b][k][i], b < nb, i < K.  A (C, nb, J, K); plane p = C reads
// sum_c A_c, added in registers in index order; s (nb, K) or null; B (nb, N, K), or null for B = A_p: symmetric bit for bit.
// The range of b is cut into chunks of fun_gram_chunk(K), one partial tile per chunk in `part` (fun_gram_part_elems doubles), added
// in chunk order by a second launch: no atomics, the same bits on every call.
struct FunGramDesc {
    const double *A = nullptr;
    int C = 1, nb = 0, J = 0, K = 0;
    const double *s = nullptr;
    const double *B = nullptr;
    int N = 0;
    double *part = nullptr;
    double *list = nullptr;         // (C, J, N)
    double *sum = nullptr;          // (J, N): plane C
    const char *prof_name = "fun_gram";
};
int fun_gram_chunk(int K);          // b per chunk: a function of the contracted row length alone
size_t fun_gram_part_elems(int C, int nb, int J, int K, int N);
void k_fun_gram(gpcsd_ctx *c, const FunGramDesc &d, hipStream_t s);
void k_fun_relayout(gpcsd_ctx *c, const double *in, int J, int n1, int n2, double *out, hipStream_t s);      // (J, n1, n2) -> (n1, J, n2)
// prior[p] = both triangles of raw[p] (J, J) from its lower one, cov[p] = prior[p] - expl[p], p < planes
void k_fun_finish(gpcsd_ctx *c, const double *raw, const double *expl, int J, int planes, double *prior, double *cov, hipStream_t s);

// ---------------------------------------------------------------- hyper-parameter uncertainty (fisher.hip)
// The score product: quad[b][r] = sum over the entries (m, n) of trial r of (A_b B_b)[m][n] E[m][n] w[.], b < batch, with no C
// stored.  trial_in_col: N = R nt, the trial is n / nt and w = w[n % nt] (Ahat_p B); else M = nx R, the trial is m % R and
// w = w[m / R] (B Bhat_q).  Per-tile partial sums per column (row), added per trial in index order by a second launch: no
// atomics, and a trial's sum does not depend on R.
struct FisherScoreDesc {
    const double *A = nullptr;      // (M, K) row-major, batch entries sA apart
    long lda = 0, sA = 0;
    const double *B = nullptr;      // (K, N) row-major, batch entries sB apart
    long ldb = 0, sB = 0;
    const double *E = nullptr;      // (M, N) row-major
    long lde = 0;
    const double *w = nullptr;
    int M = 0, N = 0, K = 0, batch = 1;
    bool trial_in_col = true;
    int nt = 0, R = 0;
    double *quad = nullptr;         // (batch, R)
    const char *prof_name = "fisher_score";
};
void k_fisher_score(gpcsd_ctx *c, const FisherScoreDesc &d, hipStream_t s);
void k_fisher_trial_sumsq(gpcsd_ctx *c, const double *B, int nx, int R, int nt, double *quad, hipStream_t s);     // quad[r] = |B_r|^2, B [x][r][t]
// scores[r][i] = 1/2 quad[i][r] - 1/2 trace[i]
void k_fisher_scores(gpcsd_ctx *c, const double *quad, const double *trace, int R, int ng, double *scores, hipStream_t s);
// out[pair(a <= b)] = sum_e X_a[e] X_b[e] W[e] over nm matrices of n2 elements, pairs in the order (0,0), (0,1), .., (1,1), ..
void k_fisher_pairs(gpcsd_ctx *c, const double *X, const double *W, long n2, int nm, double *out, hipStream_t s);
// out[i] = sum sv_i[x] tv_i[t] U[x][t] (i < ng); out[ng + pair(i <= j)] = sum sv_i sv_j tv_i tv_j U^2; sv (ng, nx), tv (ng, nt)
void k_fisher_diag(gpcsd_ctx *c, const double *sv, const double *tv, const double *U, int nx, int nt, int ng, double *out, hipStream_t s);
// sv / tv of the nsp spatial directions (diag Ahat_p, et), the ntp temporal ones (es, diag Bhat_q) and the noise (1, 1); es2, et2
void k_fisher_weights(gpcsd_ctx *c, const double *Ah, const double *Bh, const double *es, const double *et, int nx, int nt, int nsp,
                      int ntp, double *sv, double *tv, double *es2, double *et2, hipStream_t s);
// dA/dR (nx, G) as a matrix (ngl2 == 0: 1D)
void k_fisher_dA_dR(gpcsd_ctx *c, const double *x, int nx, const double *gx1, const double *gw1, const double *gx2, const double *gw2,
                    int G, int ngl2, double R, double eps, double *out, hipStream_t s);
// out[2c] = dKt / d ell_c, out[2c + 1] = dKt / d sigma2_c, (nt, nt) each
void k_fisher_temporal_dgram(gpcsd_ctx *c, const TemporalSet &set, const double *t, int nt, double *out, hipStream_t s);

}  // namespace gpcsd
