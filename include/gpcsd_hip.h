/*
 * gpcsd_hip.h -- C ABI of libgpcsd_hip.so, the MI355X (gfx950) implementation of the
 * GPCSD covariance-assembly / Kronecker-eigen marginal-likelihood / posterior-predict
 * hot path.
 *
 * The reference (natalieklein/gpcsd) is pure Python and has no FFI; the boundary it
 * offers is its Python class + operator surface.  Every entry point below names the
 * reference function (file:line under /root/reference/) whose arithmetic it replaces;
 * the Python package `gpcsd_amd` mirrors the reference classes and calls these through
 * ctypes (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *   - All arrays are C-contiguous float64 HOST buffers owned by the caller unless a
 *     name ends in `_dev`.  The library never retains a host pointer past the call.
 *   - Every function returns int: 0 ok; >0 numerical failure (eigensolver did not
 *     converge, Cholesky pivot <= 0 at column k -> return k+1) which the Python shim
 *     turns into numpy.linalg.LinAlgError exactly where the reference would raise it
 *     (gpcsd1d.py:219, gpcsd2d.py:217,258); <0 usage / HIP runtime error.
 *     NaN/Inf in results are returned, not trapped (reference runs under
 *     np.seterr(all='ignore'), gpcsd1d.py:7).
 *   - One ctx = one device + its four HIP streams (main, temporal chain, spatial
 *     chain, side products: DESIGN.md 4.8) + the resident data; calls on one ctx must
 *     be serialised by the caller, different contexts may be used from different
 *     threads.  Contexts are created lazily by the Python layer (fork safety).
 */
#ifndef GPCSD_HIP_H
#define GPCSD_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPCSD_MAX_TEMPORAL 8
#define GPCSD_KIND_SE      0   /* covariances.py:257-271 */
#define GPCSD_KIND_MATERN  1   /* covariances.py:291-305 */
#define GPCSD_KIND_HOST    2   /* user-defined GPCSDTemporalCov subclass (covariances.py:235-238): its Gram matrices are
                                  evaluated by the caller's compute_Kt and handed over with gpcsd_set_host_temporal_gram */
/* The two kinds between Matern-1/2 (GPCSD_KIND_MATERN) and SE, evaluated on the device like those (no counterpart in the reference;
 * sigma2 (1 + a) exp(-a), a = sqrt(3) |d| / ell, and sigma2 (1 + a + a^2 / 3) exp(-a), a = sqrt(5) |d| / ell).  Accepted wherever
 * SE and MATERN are; every other value is rejected with rc -3 before anything is launched. */
#define GPCSD_KIND_MATERN32 3
#define GPCSD_KIND_MATERN52 4

/* Capacity limits of this build (no counterpart in the reference, which is bounded by host memory only).  Exceeding one
 * returns GPCSD_ERR_CAPACITY (-7), which the Python layer raises as gpcsd_amd.GPCSDCapacityError -- a RuntimeError, so
 * that fit()'s LinAlgError / ValueError handlers (gpcsd1d.py:219, gpcsd2d.py:217,258) do not swallow it.
 *   GPCSD_MAX_EIG_N           rows of one symmetric eigenproblem after symmetry folding (a mirror-symmetric grid of up
 *                           to 8192 points): nx and nt of the fused calls, n of gpcsd_eigh / gpcsd_eig_D
 *   GPCSD_MAX_GEMM_LD_KMAJOR  doubles in one row of a flat GEMM operand whose rows are the contracted index: ntrials * nt
 *                           of the resident block of trials (8.4 M: 16 777 trials of 500 samples, 25 GB of fp64 at 384
 *                           electrodes; shard trials over ranks beyond that)                                          */
#define GPCSD_MAX_EIG_N           4096
#define GPCSD_MAX_GEMM_LD_KMAJOR  (1L << 23)
/*   GPCSD_MAX_MISSING         missing samples of ONE trial in gpcsd_predict_masked / gpcsd_loglik_masked (m of gpcsd_masked_gram):
 *                           the Schur complement of the missing set is a dense m x m matrix, 512 MB of fp64 at the limit       */
#define GPCSD_MAX_MISSING         8192
/*   GPCSD_MAX_SHIFT_NSEG      shifted components of gpcsd_shift_plan (its gradient kernel keeps one partial sum per component in
 *                           registers; the reference's data has 10-20 per probe)                                                */
#define GPCSD_MAX_SHIFT_NSEG      32
/*   GPCSD_MAX_REGIONS         labelled regions J of gpcsd_region_features / gpcsd_sample_features (one row of workgroups per region
 *                           in the pass that folds a region's partial results)                                                   */
#define GPCSD_MAX_REGIONS         4096
/*   GPCSD_CV_MAX_FOLD         electrodes in one fold of gpcsd_cv_electrodes (the f x f block of a fold is factored by one lane: 136
 *                           doubles at the limit; gpcsd_predict_masked holds out larger sets)                                    */
#define GPCSD_CV_MAX_FOLD         16
#define GPCSD_ERR_CAPACITY      (-7)
/* values per region and column of gpcsd_region_features / gpcsd_sample_features */
#define GPCSD_NFEAT             10

#define GPCSD_PRED_CSD  1
#define GPCSD_PRED_LFP  2
#define GPCSD_PRED_BOTH 3

typedef struct gpcsd_ctx gpcsd_ctx;

/* Hyper-parameters read from the reference's mutable param dicts at every call
 * (gpcsd1d.py:53-62, gpcsd2d.py:67-79, covariances.py:48,174,254,288). */
typedef struct gpcsd_hparams {
    double R;                               /* forward-model radius                      */
    double eps;                             /* 2D singularity offset (ignored in 1D)     */
    double ell_s[2];                        /* spatial length scale(s): 1D uses [0]      */
    int    n_temporal;                      /* number of temporal components (<= 8)      */
    int    kind[GPCSD_MAX_TEMPORAL];        /* GPCSD_KIND_*                              */
    double ell_t[GPCSD_MAX_TEMPORAL];
    double sigma2_t[GPCSD_MAX_TEMPORAL];
    int    n_sig2n;                         /* 1 = scalar noise, nx = per-electrode list */
    const double *sig2n;                    /* host pointer, n_sig2n doubles             */
    double jitter;                          /* JITTER added to Ks in loglik (gpcsd1d.py:17, gpcsd2d.py:16) */
} gpcsd_hparams;

/* ---- context -------------------------------------------------------------------- */
int  gpcsd_ctx_create(int device, gpcsd_ctx **out);
int  gpcsd_ctx_destroy(gpcsd_ctx *ctx);
/* The HIP streams a context queues on, as integers (hipStream_t): which = 0 the main stream (every fused call's products and
 * results; an integrator orders its own HIP work against the library with an event on this one), 1 / 2 the temporal / spatial
 * eigen chains (utility_functions.py:58-59), 3 the side stream.  A closed context's four streams go back to a per-device pool and
 * the next context of the process takes them over (the stream -> hardware queue mapping is fixed when a stream is created: models
 * opened one after another run on the same queues); which = -1 / -2 (ctx may be NULL): stream sets created / taken over so far in
 * this process.  GPCSD_STREAM_POOL=0 switches the pool off. */
int  gpcsd_ctx_stream_handle(gpcsd_ctx *ctx, int which, unsigned long long *out);
const char *gpcsd_last_error(gpcsd_ctx *ctx);     /* ctx may be NULL: last global error */
int  gpcsd_version(void);
/* waits for everything queued on the context; also reports (rc > 0) a pending asynchronous gpcsd_predict_resident's failure */
int  gpcsd_device_synchronize(gpcsd_ctx *ctx);
/* Page-locked host blocks for result arrays (gpcsd2d.py:328-334 returns host arrays of (1+C)*nz*nt*ntrials doubles: 231 MB
 * at 384 x 500 x 50).  Outputs handed to gpcsd_predict / gpcsd_fetch / gpcsd_sample_prior may live in such a block, in which
 * case the device-to-host copy is a single DMA at link speed; any other host pointer still works (staged, slower). */
int  gpcsd_host_alloc(size_t bytes, void **out);
int  gpcsd_host_free(void *p);
/* PCI address of device `device` ("0000:c5:00.0", NUL-terminated into buf[len], len >= 16): what a host needs to find the
 * device's NUMA node (/sys/bus/pci/devices/<address>/numa_node) and keep its threads there.  On the two-socket hosts of the
 * MI355X pool a host process free to migrate between the sockets ran the queued step of bench.py at 1.12 .. 1.25 ms from run to
 * run, one kept on either socket's CPUs at 1.13 (gpcsd_amd._hip.bind_host_to_device_numa; `numactl`/`taskset` do the same from
 * outside).  No context needed. */
int  gpcsd_device_pci_bus_id(int device, char *buf, int len);

/* ---- resident data (copied; re-laid-out on device) ----------------------------- */
/* lfp is (nx, nt, ntrials) C-order as held by GPCSD{1,2}D.lfp (gpcsd1d.py:34, gpcsd2d.py:36);
 * stored on device electrode-major / trial / time so both projections are flat GEMMs. */
int gpcsd_set_lfp(gpcsd_ctx *ctx, const double *lfp, int nx, int nt, int ntrials);
/* GPCSD1DSpatialCov.__init__ state (covariances.py:12-27): electrodes + mapped GL rule */
int gpcsd_set_geometry_1d(gpcsd_ctx *ctx, const double *x, int nx,
                          const double *gl_x, const double *gl_w, int ngl);
/* GPCSD2DSpatialCov.__init__/reset_x state (covariances.py:99-137): xy is (nx,2) */
int gpcsd_set_geometry_2d(gpcsd_ctx *ctx, const double *xy, int nx,
                          const double *gl_x1, const double *gl_w1, int ngl1,
                          const double *gl_x2, const double *gl_w2, int ngl2);
int gpcsd_set_time(gpcsd_ctx *ctx, const double *t, int nt);   /* GPCSDTemporalCov.t */
/* User-defined temporal covariances (covariances.py:235-238; gpcsd1d.py:118-120 accepts any object with compute_Kt):
 * Kt = sum_c cov_c.compute_Kt() (nt, nt) and, for predict, Kt_cross[c] = cov_c.compute_Kt(tstar) (ncomp, ntstar, nt;
 * may be NULL for loglik), evaluated by the caller.  Copied; used by every later fused call whose hparams carry a
 * component of kind GPCSD_KIND_HOST, in place of the built-in Gram builders (the eigensolver, projections and predict
 * chain are unchanged; the reflection fold of the time axis is skipped since such a kernel need not be stationary).
 * Kt == NULL clears it.  gpcsd_loglik_grad needs the derivatives of such a Gram as well (gpcsd_set_host_temporal_dgram); without
 * them it refuses such hparams (-3). */
int gpcsd_set_host_temporal_gram(gpcsd_ctx *ctx, const double *Kt, int nt, const double *Kt_cross, int ncomp, int ntstar);
/* Derivatives of that Gram matrix with respect to the natural temporal hyper-parameters, evaluated by the caller (the
 * reference differentiates any GPCSDTemporalCov subclass by tracing it with autograd, gpcsd1d.py:211; here the class offers
 * compute_dKt(name)): dKt is (nmat, nt, nt) with nmat = 2 * n_temporal, ordered (d/d ell_c, d/d sigma2_c) per component.
 * Copied; belongs to the Gram handed over last (a new gpcsd_set_host_temporal_gram clears it).  With it gpcsd_loglik_grad
 * accepts GPCSD_KIND_HOST components: its temporal entries are <Gt, dKt_k>, one evaluation per gradient.  dKt == NULL clears. */
int gpcsd_set_host_temporal_dgram(gpcsd_ctx *ctx, const double *dKt, int nt, int nmat);

/* ---- operator surface (stand-alone; host in / host out) ------------------------- */
/* b_fwd_1d(r, R)                        forward_models.py:9-17   (elementwise, n values) */
int gpcsd_b_fwd_1d(gpcsd_ctx *ctx, const double *r, long n, double R, double *out);
/* predictcsd_trad_1d / _2d  predict_csd.py:3-16 / :19-31: minus the second difference along the electrode axis of host data
 * viewed as (n_outer, n_axis, n_inner) -- 1-D: (1, nx, nt*ntrials), ends of the axis -0.0 (edge_nan = 0); 2-D, column-wise on
 * gridded data: (nx1, nx2, nt*ntrials), first and last column NaN (edge_nan = 1).  out has the shape of lfp. */
int gpcsd_trad_csd(gpcsd_ctx *ctx, const double *lfp, long n_outer, long n_axis, long n_inner, int edge_nan, double *out);
/* b_fwd_2d(delta1, delta2, R, eps, w)   forward_models.py:42-54  (w != NULL -> d1,d2 ignored) */
int gpcsd_b_fwd_2d(gpcsd_ctx *ctx, const double *d1, const double *d2, const double *w, long n,
                   double R, double eps, double *out);
/* GPCSDTemporalCov{SE,Matern,Matern32,Matern52}.compute_Kt(t, tprime)   covariances.py:257-271 / :291-305; out (n, m).
 * kind: any GPCSD_KIND_* but HOST (rc -3 otherwise). */
int gpcsd_gram_temporal(gpcsd_ctx *ctx, int kind, const double *t, int n, const double *tp, int m,
                        double ell, double sigma2, double *out);
/* GPCSD1DSpatialCovSE.compute_Ks        covariances.py:50-56 ; out (nx, nx) */
int gpcsd_ks_csd_1d(gpcsd_ctx *ctx, const double *x, int nx, double ell, double *out);
/* GPCSD2DSpatialCovSE.compute_Ks        covariances.py:177-186 */
int gpcsd_ks_csd_2d(gpcsd_ctx *ctx, const double *xy, int nx, double ell1, double ell2, double *out);
/* compKphi_1d(R, xp)                    covariances.py:74-96 ; out (nx, nxp); xp NULL -> x */
int gpcsd_kphi_1d(gpcsd_ctx *ctx, const double *x, int nx, const double *gl_x, const double *gl_w, int ngl,
                  double R, double ell, const double *xp, int nxp, double *out);
/* compKphig_1d(z, R)                    covariances.py:58-72 ; out (nx, nz) */
int gpcsd_kphig_1d(gpcsd_ctx *ctx, const double *x, int nx, const double *gl_x, const double *gl_w, int ngl,
                   const double *z, int nz, double R, double ell, double *out);
/* compKphi_2d(R, eps, xp)               covariances.py:204-232 ; xy (nx,2), xp (nxp,2) or NULL */
int gpcsd_kphi_2d(gpcsd_ctx *ctx, const double *xy, int nx,
                  const double *gl_x1, const double *gl_w1, int ngl1,
                  const double *gl_x2, const double *gl_w2, int ngl2,
                  double R, double eps, double ell1, double ell2,
                  const double *xp, int nxp, double *out);
/* compKphig_2d(z, R, eps)               covariances.py:188-202 ; z (nz,2) */
int gpcsd_kphig_2d(gpcsd_ctx *ctx, const double *xy, int nx,
                   const double *gl_x1, const double *gl_w1, int ngl1,
                   const double *gl_x2, const double *gl_w2, int ngl2,
                   const double *z, int nz, double R, double eps, double ell1, double ell2, double *out);
/* numpy.linalg.eigh as used by comp_eig_D (utility_functions.py:58-59): ascending evals, evecs in columns */
int gpcsd_eigh(gpcsd_ctx *ctx, const double *A, int n, double *evals, double *evecs);
/* the same for a matrix the caller vouches is positive semi-definite (a Gram matrix such as Ks, Kt handed to comp_eig_D,
 * utility_functions.py:44-64): it may take the rank-revealing early exit of gpcsd_tail_early_exit (orders <= 192) */
int gpcsd_eigh_psd(gpcsd_ctx *ctx, const double *A, int n, double *evals, double *evecs);
/* `count` matrices of the same order through one shared chain of launches (batched hyper-parameter evaluations decompose
 * all their Gram matrices this way): A (count,n,n) -> evals (count,n), evecs (count,n,n); status[i] > 0: matrix i failed. */
int gpcsd_eigh_batch(gpcsd_ctx *ctx, const double *A, int n, int count, double *evals, double *evecs, int *status);
/* Diagnostics for the large-n eigensolver stages (no reference counterpart; LAPACK does these inside dsyevd):
 * Householder tridiagonalisation A = Q T Q^T: d (n), e (n, last unused), reflectors V (n,n) by rows, tau (n) */
int gpcsd_debug_sytrd(gpcsd_ctx *ctx, const double *A, int n, double *d, double *e, double *V, double *tau);
/* divide & conquer eigen-decomposition of tridiag(d (n), e (n-1)): w ascending, Z (n,n) eigenvectors in columns */
int gpcsd_debug_stedc(gpcsd_ctx *ctx, const double *d, const double *e, int n, double *w, double *Z);
/* Diagnostics for the shifted-tridiagonal kernels of the default step (no reference counterpart): item (x', p) is the system
 * A = es[x'] m_p T_p + sig2 I with T_p = tridiag(d_p (np_p), e_p (np_p - 1)); W (nx, R, nt) holds its right-hand sides in the
 * columns [c0_p, c0_p + np_p) of the rows [x'][r].  variant: 0 the library's choice, 1 serial pivots, 2 pivot scan (-3 for a
 * block of more than 256 columns).  partials (4 nx): w^T A^-1 w summed over r per item (2 x' + p), then log det A per item;
 * sums (2): the totals of the two halves as the step forms them (quadratic forms, log-determinants). */
int gpcsd_debug_ll_tridiag(gpcsd_ctx *ctx, const double *W, const double *es, int nx, int R, int nt,
                           const double *d0, const double *e0, double m0, int np0, int c00,
                           const double *d1, const double *e1, double m1, int np1, int c01,
                           double sig2, int variant, double *partials, double *sums);
/* the same systems solved: B (nx, R, nt) = W with the blocks' columns replaced by A^-1 w, every other column untouched.
 * pass: trials per pass of the kernel, 0 the library's choice, 32 or 64.  -3 for R < 16 or a block of more than 256 columns. */
int gpcsd_debug_tridiag_solve(gpcsd_ctx *ctx, const double *W, const double *es, int nx, int R, int nt,
                              const double *d0, const double *e0, double m0, int np0, int c00,
                              const double *d1, const double *e1, double m1, int np1, int c01,
                              double sig2, int pass, double *B);
/* Diagnostics for the fp64 MFMA GEMM core (no reference counterpart): one launch of the core with the whole descriptor in the
 * caller's hands.  The fields mirror GemmDesc (csrc/kernels.hpp: layouts, epilogues, both batch levels, dyn, lower); every
 * operand is a host array with its length in doubles (ints for dyn) and is uploaded exactly as given.  C, C2, C3 and quad_out
 * are in/out: their contents are the buffers' initial contents and come back whole, padding included.  The furthest element
 * every operand can address is computed from the sizes, strides and batch counts and compared with its length before
 * anything is uploaded: -3 for an operand that is missing, too short or laid out below the minimum leading dimension. */
typedef struct gpcsd_debug_gemm_args {
    int M, N, K, transA, transB;
    int cfg, epi;                        /* cfg 0 (automatic), 1, 2, 3, 5; epi: enum Epi */
    int rdiv, batch, batch2;
    int lower, lower_shift;
    long lda, ldb, ldc, ldd;
    long sA, sB, sC, sD, sColscale, sKscale;                                  /* strides of the inner batch level */
    long sA2, sB2, sC2, sD2, sColscale2, sRowscale2, sDyn2, sQuad2, sKscale2; /* ... of the outer one */
    double alpha;
    const double *A, *B;
    long nA, nB;
    double *C, *C2, *C3;                 /* C2 / C3 (EPI_GRAD, optional) have C's length and layout */
    long nC;
    const double *D, *colscale, *rowscale, *kscale;
    long nD, nColscale, nRowscale, nKscale;
    const int *dyn;                      /* optional: effective N = K of batch entry (z2, z1) at dyn[z2 * sDyn2 + z1] */
    long nDyn;
    double *quad_out;                    /* EPI_QUAD: one sum per outer entry at z2 * sQuad2, EPI_GRAD: two */
    long nQuad;
} gpcsd_debug_gemm_args;
int gpcsd_debug_gemm(gpcsd_ctx *ctx, gpcsd_debug_gemm_args *args);
/* Diagnostics for the analytic gradient's contraction kernels (csrc/grad.hip; no reference counterpart: they replace the autograd
 * tape): ONE of the k_* launchers on the context's main stream, host arrays in and out, nothing else between the caller and the
 * kernels.  in[k] / out[k] are host arrays with their lengths in doubles in nin[k] / nout[k]; the furthest element the launcher
 * can address is compared with every length before anything is uploaded.  B: hyper-parameter sets (1 where an op has none);
 * table != 0: the scalars come from a device table of the B sets in hp (built as the gradient evaluation builds it), else from
 * hp[0] / s[] by value (then B must be 1).  s_out (l[3]): distance of the sets' outputs in out[0] (the evaluation uses 64).
 *   op  launcher                n[]                  l[]            s[]            in[]                              out[]
 *   0   k_temporal_grad         nt                   -, -, -, s_out -              Gt (B nt nt), t (nt)              (B s_out): 2 ncomp each
 *   1   k_frob_inner            nm                   n2             -              Gt (n2), dK (nm n2)               (nm)
 *   2   k_kgl_grad              G, ngl2 (0: 1D)      -, -, -, s_out ell1, ell2     M, Kgl (B G G), gx1, gx2          (B s_out): 1 or 2 each
 *   3   k_frob_pair             -                    n, -, -, s_out -              P, T1, T2 (B n)                   (B s_out): 2 each
 *   4   k_fwdR_grad             nx, G, ngl2 (0: 1D)  -, -, -, s_out R, eps         S (B nx G), x, gx1, gw1, gx2, gw2 (B s_out): 1 each
 *   5   k_D_sums                nx, nt               -, -, -, s_out -              D (B nx nt), es (B nx), et (B nt) a (B nx), b (B nt), sum 1/D
 *                                                                                                                    (B s_out), row sums of 1/D (B nx)
 *   6   k_batch_reduce          nb, n                stride, s_in,  scale, dscale  in, dvec                          (B s_out) [s_out >= n n]
 *                                                    s_dvec, s_out
 *   7   k_siglist_eigvec_term   nx                   -              tiny           Ghs, Ssum (B nx nx), es, sig (B nx)  Ghs updated (B nx nx)
 *   8   k_rowgroup_sumsq        nrows                rowlen         -              B (nrows rowlen)                  (nrows)
 *   9   k_per_trial_quad        nx, nb, nt           -              -              alpha (nx nb nt), D (nx nt)       (nb)
 * Table form of op 0: 2 hp[0].n_temporal values are summed for every set (as in an evaluation, whose sets share it), so it
 * must be the largest of the sets'.  rc -3: an unknown op, a null or short operand, a non-positive size, n_temporal outside
 * [1, GPCSD_MAX_TEMPORAL], a kind the device does not evaluate (GPCSD_KIND_HOST, unknown values), nm outside [1, 2 GPCSD_MAX_TEMPORAL], B > 1 without a table where
 * the scalars come by value; nothing has been launched then. */
typedef struct gpcsd_debug_grad_args {
    int op, B, table;
    int n[4];
    long l[4];
    double s[4];
    const gpcsd_hparams *hp;             /* B sets (ops 0, 2, 4 with a table; op 0 always) */
    const double *in[6];
    long nin[6];
    double *out[4];
    long nout[4];
} gpcsd_debug_grad_args;
int gpcsd_debug_grad_op(gpcsd_ctx *ctx, gpcsd_debug_grad_args *args);
/* Diagnostics for the folded-basis and relayout kernels (csrc/gram.hip, csrc/eigh.hip; no reference counterpart): ONE of the k_*
 * launchers on the context's main stream, host arrays in and out, nothing else between the caller and the kernels.  An orbit table
 * comes from the caller as an involution perm[k] of nperm[k] points (perm[perm[i]] == i; the identity is accepted: no pair, every
 * point its own orbit) and is built by the routine the grids' own symmetries go through: pairs in the order of their first
 * members, then the fixed points (ns orbits, na pairs).  in[k] / out[k] are host arrays with their lengths in doubles in nin[k] /
 * nout[k]; the furthest element the launcher can address is compared with every length before anything is uploaded.  Every output
 * starts on the device as the bit pattern `fill` and comes back whole: what no kernel wrote still holds it (an output may be longer
 * than its launcher's reach, at least one double).  list != 0: ops 1 and 5 also write the per-component list.
 *   op  launcher                 perm[]            n[]                l[]                 in[]                 out[]
 *   0   k_swap_last2             -                 n0, n1, n2         -                   in (n0 n1 n2)        out (n0 n2 n1)
 *   1   k_swap_last2_sum         -                 n0, n1, n2, C      list_stride         in (n0 n1 C n2)      sum (n0 n2 n1), list
 *   2   k_sym_fold_rect          rows, columns     -                  ldk                 K (rows ldk apart)   ss (ns_r ns_c), aa (na_r na_c)
 *   3   k_sym_unfold_mat         matrix            -                  s_in                Gf (B sets s_in apart: ss, aa)   out (B n n)
 *   4   k_fold_lfp               electrodes, time  R                  -                   Y (nx R nt)          out (nx R nt)
 *   5   k_unfold_swap_sum        sites, time       R, C, nsP, naP     list_stride, ldin   in (nz R rows)       sum (nz nt R), list
 *   6   k_temporal_fold_fill     time grid         -                  -                   t (nt)               A0s (B ns ns), A0a (B na na), V, tau, amax
 *       (table: _tab)
 *   7   k_psd_fold_fill          grid              -                  sK                  K (B or 1 of n n)    the same
 * Op 5: nsP, naP, ldin = 0 are the launcher's defaults (unpadded blocks).  Ops 6 and 7 write where the tridiagonalisation reads
 * (the class arenas of the temporal / spatial chain) and return, per set: both scaled blocks; V = the (ns + 64) ns words of the
 * symmetric class's reflector storage and the word behind them, then the same for the antisymmetric class; tau = ns + 66 words and
 * the word behind them, then na + 67; amax = the two scale words; status[set] (ints).  Op 6 takes B sets from hp: 1 or 2 by value,
 * any number with table != 0, and honours gpcsd_set_gram_precision.  Op 7 adds s[set] to the diagonals (1 or 2 sets; sK = 0: one
 * source) or, with table != 0, hp[set].jitter.  Both need a pair (na >= 1).  They drop whatever an earlier call left for reuse in
 * those arenas (decomposition cache, positive-semi-definite marks): a model call afterwards decomposes again and returns the bits
 * it returned before.
 * rc -3: an unknown op, a null or short operand, a permutation that is no involution, a non-positive size, a stride or padded
 * width below its minimum, a table or sets where an op has none; nothing has been launched then. */
typedef struct gpcsd_debug_fold_args {
    int op, B, table, list;
    int n[4];
    long l[4];
    double s[4];
    double fill;
    const gpcsd_hparams *hp;             /* B sets (op 6; op 7 with a table) */
    const int *perm[2];
    int nperm[2];
    const double *in[2];
    long nin[2];
    double *out[5];
    long nout[5];
    int *status;                         /* ops 6 and 7: at least B words */
    int nstatus;
} gpcsd_debug_fold_args;
int gpcsd_debug_fold_op(gpcsd_ctx *ctx, gpcsd_debug_fold_args *args);
/* comp_eig_D(Ks, Kt, sig2n)            utility_functions.py:44-64 ; Dvec has nx*nt entries */
int gpcsd_eig_D(gpcsd_ctx *ctx, const double *Ks, int nx, const double *Kt, int nt,
                const double *sig2n, int n_sig, double *Qs, double *Qt, double *Dvec);
/* numpy.linalg.cholesky (gpcsd1d.py:303-304, gpcsd2d.py:343-350): lower factor, upper part zeroed */
int gpcsd_potrf(gpcsd_ctx *ctx, const double *A, int n, double *L);
/* sum(log(diag(L))) * 2 = log det(A) for A = L L^T */
int gpcsd_logdet_chol(gpcsd_ctx *ctx, const double *L, int n, double *out);
/* solve L X = B (lower, non-transposed), B and X are (n, nrhs) */
int gpcsd_trsm_lower(gpcsd_ctx *ctx, const double *L, int n, const double *B, int nrhs, double *X);
/* C(M,N) = op(A) op(B), row-major; transA: A stored (K,M); transB: B stored (N,K).  The fp64 MFMA core. */
int gpcsd_gemm(gpcsd_ctx *ctx, int transA, int transB, int M, int N, int K,
               const double *A, const double *B, double *C);
/* dense cross-check path (scalar sig2n): chol(kron(Ks,Kt)+sig2n I) log-det + triangular solves.
 * lfp (nx,nt,ntrials) host.  Not a reference code path; see DESIGN.md. */
int gpcsd_loglik_dense_chol(gpcsd_ctx *ctx, const double *Ks, int nx, const double *Kt, int nt, double sig2n,
                            const double *lfp, int ntrials, double *out);

/* ---- fused hot calls on resident data ------------------------------------------- */
/* GPCSD1D.loglik() gpcsd1d.py:113-128 / GPCSD2D.loglik() gpcsd2d.py:136-151 */
int gpcsd_loglik(gpcsd_ctx *ctx, const gpcsd_hparams *hp, double *out);
/* Sharded form: out[0] = sum(log D) (identical on every shard), out[1] = sum_r sum alpha^2/D over the
 * resident trials; loglik = -0.5*R_total*out[0] - 0.5*sum_over_shards(out[1]) */
int gpcsd_loglik_parts(gpcsd_ctx *ctx, const gpcsd_hparams *hp, double *out2);
/* The same evaluation split in two: _async validates its arguments, queues the work and returns; _wait blocks until that
 * evaluation (and only that: not whatever was queued behind it) has finished and returns its out2 / rc.  Between the two
 * the caller may queue further calls on the context -- a gpcsd_predict_resident at the same hyper-parameters, say -- whose
 * eigen-chains then run beside this evaluation's GEMMs instead of after the host has come back for the result.  Up to
 * four evaluations may be outstanding per context (rc -3 beyond that); _wait collects them oldest first.  hp is read during
 * the _async call only.  rc > 0 from _wait:
 * numerical failure of this evaluation or of an earlier asynchronous call nobody has collected yet (status is sticky until
 * a synchronising call -- gpcsd_device_synchronize, any call that returns values -- has reported it).  A _wait that reports
 * a failure drains the context and clears the status, so evaluations queued AFTER it returned start clean; evaluations that
 * were already outstanding copied the status as it stood and report the failure too (a failed wait poisons those), and
 * the decomposition cache forgets both sides (a retry with the same hp re-solves). */
int gpcsd_loglik_parts_async(gpcsd_ctx *ctx, const gpcsd_hparams *hp);
int gpcsd_loglik_parts_wait(gpcsd_ctx *ctx, double *out2);
/* gpcsd_loglik_parts_async(hp_loglik) followed by gpcsd_predict_resident(hp_predict, ...) as ONE queued call: same results
 * bit for bit, collected the same way (gpcsd_loglik_parts_wait, gpcsd_fetch), but the two temporal eigenproblems go through
 * one chain of launches as two replicas and the two spatial ones through another -- replicas inside a chain are nearly free
 * on this GPU, independent chains are not.  The usual pair is one hyper-parameter set with and without the
 * jitter (GPCSD1D.loglik gpcsd1d.py:113-128 adds it, predict gpcsd1d.py:258 does not); any two sets are accepted.  Every
 * decomposition is still computed, unless the decomposition cache is on and the temporal hyper-parameters of the two sets
 * coincide: then that side is solved once, exactly as the cache would serve the second of two separate calls.  Falls back
 * to the two calls in sequence where the folded-basis path does not apply (per-electrode noise lists, user-defined temporal
 * covariances, grids or prediction sites without the mirror symmetry). */
int gpcsd_loglik_predict_async(gpcsd_ctx *ctx, const gpcsd_hparams *hp_loglik, const gpcsd_hparams *hp_predict,
                               const double *z, int nz, const double *tstar, int ntstar, int type, int want_lists);
/* Announce the NEXT gpcsd_loglik_predict_async.  A caller that knows the hyper-parameters of its next paired evaluation before
 * the current one has been collected -- a grid or a chain of proposals fixed in advance, a benchmark loop; NOT an optimiser, whose
 * next point depends on the value it is waiting for (gpcsd1d.py:211) -- passes them here right after queueing the current call:
 * the two decomposition chains of the next call (utility_functions.py:58-59 for Kt and Ks) are queued at once and start as soon as
 * their streams are free, i.e. under the current call's products instead of behind the host's collection of its log-likelihood.
 * The next gpcsd_loglik_predict_async with the same hyper-parameters, sites and times takes them over (same launches, same
 * buffers, same bits); any other evaluation on the context in between drops them (they have then run for nothing).
 * Returns 1 when queued, 0 when the paired form does not apply to these arguments (nothing queued), < 0 on error. */
int gpcsd_prefetch_pair(gpcsd_ctx *ctx, const gpcsd_hparams *hp_loglik, const gpcsd_hparams *hp_predict, const double *z, int nz,
                        const double *tstar, int ntstar);
/* how many front halves gpcsd_prefetch_pair queued, and how many of them a paired call took over */
int gpcsd_prefetch_stats(gpcsd_ctx *ctx, long *queued, long *taken);
/* Local log-likelihood pieces and the gradient of  L_loc = -0.5*ntrials_resident*out2[0] - 0.5*out2[1]  with respect
 * to the natural hyper-parameters [R, ell_s (dim), (ell_t, sigma2_t) per component, sig2n]; with a per-electrode
 * noise list (hp->n_sig2n == nx, indexed by eigen-row as utility_functions.py:54-63) the tail holds nx entries and the
 * spatial entries include the eigenvector-rotation term (the objective is then not a function of Ks alone).
 * Replaces the autograd tape of gpcsd1d.py:211 / gpcsd2d.py:250.  Both L_loc and grad are sums over trials plus a
 * term linear in the resident trial count, so shards combine by plain summation over ranks. */
int gpcsd_loglik_grad(gpcsd_ctx *ctx, const gpcsd_hparams *hp, double *out2, double *grad, int ngrad);
/* The same evaluation for `nsets` hyper-parameter sets in ONE chain of launches -- the restarts of fit() (gpcsd1d.py:193-220,
 * gpcsd2d.py:230-262) are independent optimiser chains whose evaluations are latency-bound, so sets evaluated together
 * share every launch.  out2 is (nsets, 2), grad (nsets, ngrad); status[i] > 0 reports a numerical failure of set i alone
 * (the others are valid).  Every set gets exactly the bits a gpcsd_loglik_grad call of its own returns.  All sets must have
 * the same temporal kernel kinds and the same number of noise entries: a scalar sig2n each, or (round 5) a per-electrode list
 * of nx entries each -- the restarts of auditory_lfp/fit_gpcsd_baseline.py:85-101, evaluated on the merged-order path with the
 * eigenvector-rotation term per set. */
int gpcsd_loglik_grad_batch(gpcsd_ctx *ctx, const gpcsd_hparams *hp, int nsets, double *out2, double *grad, int ngrad,
                            int *status);
/* GPCSD{1,2}D.predict(z, t, type) gpcsd1d.py:248-293 / gpcsd2d.py:289-334.
 * z (nz, dim), tstar (ntstar) with ntstar == nt (the reference raises ValueError otherwise -> rc -22).
 * Outputs (any may be NULL): *_list is (n_temporal, nz, ntstar, ntrials), sums are (nz, ntstar, ntrials). */
int gpcsd_predict(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                  const double *tstar, int ntstar, int type,
                  double *csd_list, double *csd, double *lfp_list, double *lfp);
/* Same computation, results left in ctx-owned device buffers in the output layout (z, t, trial); nothing crosses
 * PCIe.  Buffers: "pred_out_csd", "pred_out_lfp" (nz*ntstar*ntrials) and, when want_lists,
 * "pred_out_csd_list", "pred_out_lfp_list" (n_temporal times that).  Read them back with gpcsd_fetch.
 * ASYNCHRONOUS on the symmetric-grid (folded) path: the call validates its arguments, queues the work and returns 0 with
 * the GEMM tail still in flight; any later call on the context is ordered behind it (the next call's temporal
 * eigen-chain runs beside that tail, which is the point).  A numerical failure (rc > 0) of such a call is reported by the
 * next call on the context that synchronises: gpcsd_fetch, gpcsd_device_synchronize, or any call that returns values
 * (gpcsd_loglik*, gpcsd_predict, ...).  Argument errors (rc < 0) are still reported by the call itself. */
int gpcsd_predict_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                           const double *tstar, int ntstar, int type, int want_lists);
/* Posterior mean at ARBITRARY prediction times: out_c[z, j, r] = sum_{x,i} Kcross[x, z] InvY_r[x, i] k_c(t*_j, t_i) with
 * k_c(t*_j, t_i) = cov_c.compute_Kt(tstar)[j, i], the TRAINING axis i contracted; ntstar is any positive count (up-sampling, a
 * window, times shifted against the grid).  NO REFERENCE COUNTERPART: the reference's predict reshapes compute_Kt(tstar) as if it
 * were (nt, ntstar) (gpcsd1d.py:277-279), so it needs ntstar == nt and contracts the test axis of the cross Gram with the training
 * axis of InvY -- a GP prediction only when tstar is the training grid, where Kt is symmetric.  gpcsd_predict reproduces that
 * quirk bit for bit and keeps it; this call is the prediction itself, and equals gpcsd_predict (to rounding) when tstar == t.
 * Arguments, `type`, NULL outputs and return codes as gpcsd_predict, except that no length is refused with -22; a capacity limit
 * (ntrials * ntstar or n_temporal * ntstar >= GPCSD_MAX_GEMM_LD_KMAJOR) returns GPCSD_ERR_CAPACITY before tstar is read.
 * Outputs: *_list (n_temporal, nz, ntstar, ntrials), sums (nz, ntstar, ntrials).  User-defined temporal covariances
 * (GPCSD_KIND_HOST): hand compute_Kt(tstar) per component, (ncomp, ntstar, nt), to gpcsd_set_host_temporal_gram first. */
int gpcsd_predict_at(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                     const double *tstar, int ntstar, int type,
                     double *csd_list, double *csd, double *lfp_list, double *lfp);
/* Same computation, results left in the named device buffers of gpcsd_predict_resident ("pred_out_csd", "pred_out_lfp":
 * nz*ntstar*ntrials; "pred_out_csd_list", "pred_out_lfp_list": n_temporal times that, when want_lists) for gpcsd_fetch /
 * gpcsd_device_buffer.  This call waits for its own work: a numerical failure (rc > 0) is returned by the call itself. */
int gpcsd_predict_at_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                              const double *tstar, int ntstar, int type, int want_lists);
/* Posterior VARIANCE of the CSD / LFP at sites z and ARBITRARY times tstar -- the diagonal of the posterior covariance of the model
 * whose mean gpcsd_predict_at returns (no jitter; a per-electrode noise list on the eigen-index as utility_functions.py:54-63).  NO
 * REFERENCE COUNTERPART: the reference has no predictive variance.  Per component c and for the component sum,
 *   var_c[z, j]   = prior_s[z] sigma2_c       - k_c^T (Ks (x) Kt + sig2n I)^-1 k_c,      k_c = Kcross[:, z] (x) k_c(t*_j, t),
 *   var_sum[z, j] = prior_s[z] sum_c sigma2_c - (sum_c k_c)^T (..)^-1 (sum_c k_c)         (NOT sum_c var_c: the components are
 *                                                                                         correlated a posteriori),
 * with prior_s = 1 for the CSD (the diagonal of compute_Ks, covariances.py:50-56, 177-186) and the diagonal of compKphi at the sites
 * (covariances.py:74-96, 204-232) for the LFP, whose variance is that of the noise-free potential (no sig2n added).  Values are
 * returned UNCLAMPED: where var << prior the subtraction may leave a slightly negative entry.  Reads no trial data (gpcsd_set_lfp
 * must have fixed nx and nt); the cost does not depend on ntrials.  Arguments and `type` as gpcsd_predict_at; outputs (any may be
 * NULL): *_var_list (n_temporal, nz, ntstar), *_var (nz, ntstar).  Capacity (n_temporal * ntstar >= GPCSD_MAX_GEMM_LD_KMAJOR) returns
 * GPCSD_ERR_CAPACITY before tstar is read.  A user-defined temporal covariance (GPCSD_KIND_HOST) has no prior diagonal on the
 * device: rc -3. */
int gpcsd_predict_var(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                      const double *tstar, int ntstar, int type,
                      double *csd_var_list, double *csd_var, double *lfp_var_list, double *lfp_var);
/* Same computation (no reference counterpart), results left in the named device buffers "pred_var_csd", "pred_var_lfp" (nz*ntstar)
 * and "pred_var_csd_list", "pred_var_lfp_list" (n_temporal times that) for gpcsd_fetch / gpcsd_device_buffer.  Waits for its own
 * work: a numerical failure (rc > 0) is returned by the call itself.  The buffers of the posterior means are left alone. */
int gpcsd_predict_var_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                               const double *tstar, int ntstar, int type);
/* The last product of gpcsd_predict_var alone, on host arrays (no reference counterpart; upload, one launch, download): G (nz, K)
 * and P (K, C * nts) -- component c in the columns [c * nts, (c + 1) * nts) --, prior_s (nz), kd (C) -> out (C + 1, nz, nts):
 *   out[c][z][j] = prior_s[z] kd[c]       - sum_k G[z][k] P[k][c * nts + j]^2             c < C
 *   out[C][z][j] = prior_s[z] sum_c kd[c] - sum_k G[z][k] (sum_c P[k][c * nts + j])^2
 * P is squared on its way to the multiplier; prior_s kd - sum is one fused multiply-add. */
int gpcsd_var_contract(gpcsd_ctx *ctx, const double *G, int nz, int K, const double *P, int C, int nts,
                       const double *prior_s, const double *kd, double *out);
/* Leave-one-out cross-validation of the fitted Gaussian process, in closed form and without a refit (Rasmussen & Williams, Gaussian
 * Processes for Machine Learning, 5.4.2).  NO REFERENCE COUNTERPART: the reference would need the diagonal of the inverse of the
 * (nx nt)^2 covariance.  K is the covariance of the data exactly as gpcsd_loglik sees it: K = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T
 * with Ks + hp->jitter I = Qs diag(es) Qs^T, Kt = Qt diag(et) Qt^T, D[x', i'] = es[x'] et[i'] + sig2n -- a per-electrode noise list
 * on the eigen-index x' as utility_functions.py:54-63; a user-defined temporal Gram (GPCSD_KIND_HOST) is allowed.  For sample (x, t)
 * of trial r, with c = diag(K^-1) (trial-independent) and beta_r = K^-1 y_r:
 *   loo_var[x, t]     = 1 / c[x, t]                      predictive variance of the NOISY sample given all others
 *   loo_mean[x, t, r] = y_r[x, t] - beta_r[x, t] / c[x, t]
 *   lpd_r[x, t]       = 1/2 log c - 1/2 beta_r^2 / c - 1/2 log(2 pi)      (a density per sample: unlike gpcsd_loglik it KEEPS the
 *                                                                           2 pi constant, to be compared across models and sizes)
 * Outputs (any may be NULL; mean == NULL also skips its stores on the device): var (nx, nt); mean (nx, nt, ntrials), the layout of
 * the data; lpd and sse (nx, ntrials) = the sums over t of lpd_r and of the squared residual (beta_r / c)^2.  The sums are formed in
 * a fixed order without atomics: the same call returns the same bits.  Capacity (ntrials * nt >= GPCSD_MAX_GEMM_LD_KMAJOR or
 * nx * ntrials >= 2^31) returns GPCSD_ERR_CAPACITY before anything is read; rc -4 without resident data. */
int gpcsd_loo(gpcsd_ctx *ctx, const gpcsd_hparams *hp, double *var, double *mean, double *lpd, double *sse);
/* Same computation (no reference counterpart), results left in the named device buffers "loo_var" (nx*nt), "loo_lpd" and "loo_sse"
 * (nx*ntrials each) and, when want_mean != 0, "loo_mean" (nx*nt*ntrials) for gpcsd_fetch / gpcsd_device_buffer.  Waits for its own
 * work: a numerical failure (rc > 0) is returned by the call itself.  The buffers of the predictions are left alone. */
int gpcsd_loo_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, int want_mean);
/* Leave-electrodes-out cross-validation in closed form (no reference counterpart): the model of gpcsd_loo, but whole ELECTRODES are
 * held out -- every sample of the fold's electrodes at once, so that the prediction rests on the spatial model (the forward model,
 * R, ell_s) and not on the electrode's own neighbours in time.  Folds in CSR form: fold i holds the electrodes
 * fold_idx[fold_ptr[i] .. fold_ptr[i + 1]), 1 to GPCSD_CV_MAX_FOLD of them, all folds disjoint, indices in [0, nx); electrodes in
 * no fold are allowed.  For a fold F of f electrodes (K^-1)_FF = Qt blockdiag_j(G_j) Qt^T with one f x f matrix per temporal
 * eigen-index j,
 *   G_j[a][b] = sum_x' Qs[a][x'] Qs[b][x'] / D[x'][j],   u_j,r = (Qs ((Qs^T Y_r Qt) / D))[F][j],   e_j,r = G_j^-1 u_j,r
 * (e: the held-out residual y - yhat in the temporal eigen-basis), and
 *   lpd[F][r]    = 1/2 sum_j log det G_j - 1/2 sum_j u_j,r^T e_j,r - 1/2 f nt log(2 pi)   joint log predictive density of the block
 *   sse[a][r]    = sum_j e_j,r[a]^2           = sum_t (y - yhat)^2 of electrode a (Qt is orthogonal)
 *   var[a][t]    = sum_j Qt[t][j]^2 (G_j^-1)[a][a]              predictive variance of the NOISY held-out sample
 *   mean[a][t][r] = y - sum_j Qt[t][j] e_j,r[a]
 * Outputs (any may be NULL; mean == NULL also skips its stores and its product on the device, with the same bits for the rest):
 * var (nx, nt); mean (nx, nt, ntrials); lpd (nfolds, ntrials); sse (nx, ntrials); status (nfolds) ints, 1 = some G_j of the fold
 * lost positive definiteness (its outputs are NaN).  Rows of electrodes in no fold are NaN.  All sums are formed in a fixed order
 * without atomics: the same call returns the same bits, and a fold's outputs depend neither on the other folds of the call nor on
 * their order.  rc -3: null hp / fold arrays, nfolds <= 0, an empty fold, an index out of range, a repeated electrode; rc -4: no
 * resident trials; GPCSD_ERR_CAPACITY: a fold above GPCSD_CV_MAX_FOLD, or the row capacities of gpcsd_loo -- all returned before
 * anything is read or launched, and the context stays usable. */
int gpcsd_cv_electrodes(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const int *fold_ptr, const int *fold_idx, int nfolds, double *var,
                        double *mean, double *lpd, double *sse, int *status);
/* Same computation (no reference counterpart), results left in the named device buffers "cv_var" (nx*nt), "cv_lpd" (nfolds*ntrials),
 * "cv_sse" (nx*ntrials), "cv_status" (nfolds ints) and, when want_mean != 0, "cv_mean" (nx*nt*ntrials). */
int gpcsd_cv_electrodes_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const int *fold_ptr, const int *fold_idx, int nfolds,
                                 int want_mean);
/* The kernels of gpcsd_cv_electrodes alone, on host arrays (no reference counterpart; upload, the Gram product, factor and solve,
 * the ordered sums, download): A (nx, K), W (K, nt) > 0 and V (nx, R, nt) give G_j[a][b] = sum_k A[a][k] A[b][k] W[k][j] per fold
 * and e = G_j^-1 V[F][r][j]; outputs E (nx, R, nt) (may be NULL), pdiag (nx, nt) with pdiag[a][j] = (G_j^-1)[a][a], lpd (nfolds, R),
 * sse (nx, R), status (nfolds).  Rows of electrodes in no fold are NaN.  Return codes as gpcsd_cv_electrodes (no -4). */
int gpcsd_efold_contract(gpcsd_ctx *ctx, const double *A, const double *W, const double *V, int nx, int K, int nt, int R,
                         const int *fold_ptr, const int *fold_idx, int nfolds, double *E, double *pdiag, double *lpd, double *sse,
                         int *status);
/* Hyper-parameter uncertainty.  NO REFERENCE COUNTERPART: fit() (gpcsd1d.py:193-220, gpcsd2d.py:232-259) returns a point estimate
 * and stops; tr(K^-1 d_i K K^-1 d_j K) on the (nx nt)^2 covariance is out of its reach.  Extends gpcsd_loglik_grad: the same model
 * (Ks + hp->jitter I, a user-defined temporal Gram with its derivative matrices from gpcsd_set_host_temporal_dgram allowed), the
 * same NATURAL parameters in the same order, ng = 1 + dim + 2 n_temporal + 1: [R, ell_s (dim), (ell_t, sigma2_t) per component,
 * sig2n].  Scalar sig2n only: a per-electrode list (n_sig2n == nx) ties the noise to the eigen-index of Ks
 * (utility_functions.py:54-63), so that model is not a function of Ks alone -- rc -3.
 *   gpcsd_fisher        info (ng, ng): the expected Fisher information of ONE trial, I_ij = 1/2 tr(K^-1 d_i K K^-1 d_j K), symmetric bit
 *                       for bit.  Reads no trial data and needs none resident (geometry and time grid only).
 *   gpcsd_trial_scores  scores (ntrials, ng): s[r][i] = d log p(y_r) / d theta_i = 1/2 y_r^T K^-1 d_i K K^-1 y_r - 1/2 tr(K^-1 d_i K) of
 *                       the resident trials; their sum over r is the gradient of gpcsd_loglik_grad.  rc -4 without resident data.
 * All sums are formed in a fixed order without atomics: the same call returns the same bits, and a trial's scores do not depend on
 * which other trials are resident.  rc -3: bad ng, a noise list, a GPCSD_KIND_HOST component without its derivative matrices;
 * rc > 0: numerical failure of an eigensolver; GPCSD_ERR_CAPACITY as gpcsd_loo. */
int gpcsd_fisher(gpcsd_ctx *ctx, const gpcsd_hparams *hp, double *info, int ng);
int gpcsd_trial_scores(gpcsd_ctx *ctx, const gpcsd_hparams *hp, double *scores, int ng);
/* Same computation, the scores left in the named device buffer "trial_scores" (ntrials*ng) for gpcsd_fetch / gpcsd_device_buffer.
 * Waits for its own work: a numerical failure (rc > 0) is returned by the call itself. */
int gpcsd_trial_scores_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, int ng);
/* The last product of gpcsd_loo alone, on host arrays (no reference counterpart; upload, the launch and its reduce, download):
 * V (nx * R, K) and Qt (nt, K) give beta[(x, r)][t] = sum_k V[(x, r)][k] Qt[t][k], which is never stored; with c (nx, nt) > 0 and
 * Y (nx * R, nt): e = beta / c, mean[x][t][r] = Y[(x, r)][t] - e (mean may be NULL), lpd[(x, r)] = sum_t 1/2 log c - 1/2 beta e -
 * 1/2 log(2 pi), sse[(x, r)] = sum_t e^2.  K is the contracted length (nt in gpcsd_loo).  Capacity as gpcsd_loo, checked before
 * anything is read. */
int gpcsd_loo_contract(gpcsd_ctx *ctx, const double *V, const double *Qt, const double *c, const double *Y, int nx, int R, int nt,
                       int K, double *mean, double *lpd, double *sse);
/* Band phase of a field along time: the analytic signal under a complex operator A = A_re + i A_im (nsel, nts) -- a zero-phase
 * band-pass (filtfilt / sosfiltfilt) followed by the Hilbert transform along an axis of fixed length is ONE such matrix, keeping a
 * few times keeps those rows (gpcsd_amd.utility_functions.analytic_operator builds it; filter design stays the caller's) -- and its
 * amplitude, phase and unit phasor.  NO REFERENCE COUNTERPART in the package; usage note: it replaces the filtfilt + hilbert +
 * np.angle passes over csd_pred that the reference's analysis scripts end with (auditory_lfp/fit_gpcsd_baseline.py:303-334,
 * neuropixels/fit_gpcsd2d.py:147-159).  x (nz, nts, M), M innermost (the trials, or (trial, draw) flattened):
 *   Re[z, j, m] = sum_t A_re[j, t] x[z, t, m],   Im likewise from A_im                      (one fp64 MFMA product, never stored)
 *   amp = hypot(Re, Im),   phase = atan2(Im, Re),   (u_re, u_im) = (Re, Im) / amp;          amp == 0: phase 0, phasor (1, 0)
 * Outputs (nz, nsel, M) each; any may be NULL and is then neither computed into memory nor touched.  Host arrays: upload, one
 * launch, download.  rc -3: NULL inputs or an empty shape; GPCSD_ERR_CAPACITY (before anything is read): M >=
 * GPCSD_MAX_GEMM_LD_KMAJOR, nts >= 2^22, nz * M >= 2^31. */
int gpcsd_analytic(gpcsd_ctx *ctx, const double *x, int nz, int nts, long M, const double *A_re, const double *A_im, int nsel,
                   double *phase, double *amp, double *u_re, double *u_im);
/* Same computation (no reference counterpart; usage note as gpcsd_analytic) on a field that is ALREADY in HBM: the named ctx-owned
 * device buffer src_name ("pred_out_csd", "pred_out_lfp", their "_list" forms, "post_sample_csd", "post_sample_lfp", ...) from
 * src_offset doubles on (component c of a "_list" buffer: c * nz * nts * M), read as (nz, nts, M).  want_mask: bit 0 phase -> "phase_out",
 * bit 1 amp -> "phase_amp", bit 2 u_re -> "phasor_re", bit 3 u_im -> "phasor_im" (nz * nsel * M doubles each, for gpcsd_fetch /
 * gpcsd_device_buffer / gpcsd_plv_resident); outputs not asked for are not stored.  Collects a queued prediction's deferred status
 * first (rc > 0 as gpcsd_fetch), waits for its own work and leaves every other buffer alone.  rc -2: no buffer of that name; rc -3:
 * bad arguments, the source is one of the outputs, or it holds fewer than src_offset + nz * nts * M doubles; capacity as
 * gpcsd_analytic. */
int gpcsd_analytic_resident(gpcsd_ctx *ctx, const char *src_name, long src_offset, int nz, int nts, long M, const double *A_re,
                            const double *A_im, int nsel, int want_mask);
/* Phase-locking value of ALL site pairs over the trials, from unit phasors u = u_re + i u_im (nz, nsel, R, S): R trials, S draws per
 * trial with the draw index innermost (S = 1 for posterior means; gpcsd_sample_posterior's layout otherwise).  NO REFERENCE
 * COUNTERPART in the package; usage note: one launch in place of the Python loop over site pairs of
 * auditory_lfp/fit_gpcsd_baseline.py:303-334.  For every draw s and kept time j,
 *   c_re[s, j, a, b] = 1/R sum_r (u_re[a] u_re[b] + u_im[a] u_im[b])            the complex mean resultant of exp(i (phi_a - phi_b)):
 *   c_im[s, j, a, b] = 1/R sum_r (u_im[a] u_re[b] - u_re[a] u_im[b])            its angle is the mean phase difference, and the
 *   plv[s, j, a, b]  = hypot(c_re, c_im)                                         ranks of a trial-sharded job add R c
 * Outputs (S, nsel, nz, nz) each, any may be NULL.  Only the tiles on or below the diagonal are computed and their mirror images are
 * written from the same registers: plv and c_re are symmetric, c_im antisymmetric BIT FOR BIT, the diagonal of c_im is 0.  The sums
 * run in a fixed order without atomics: the same call returns the same bits.  Host arrays: upload, one launch, download.  rc -3: NULL
 * inputs or an empty shape; GPCSD_ERR_CAPACITY (before anything is read): R * S >= GPCSD_MAX_GEMM_LD_KMAJOR, nz >= 2^21, or 2^31 tiles. */
int gpcsd_plv(gpcsd_ctx *ctx, const double *u_re, const double *u_im, int nz, int nsel, int R, int S, double *c_re, double *c_im,
              double *plv);
/* Same computation (no reference counterpart; usage note as gpcsd_plv) on the unit phasors gpcsd_analytic_resident left in
 * "phasor_re" / "phasor_im", read as (nz, nsel, R, S); results in the named device buffers "plv_re", "plv_im", "plv_abs"
 * (S * nsel * nz * nz doubles each).  Waits for its own work and leaves every other buffer alone.  rc -4 unless the last
 * gpcsd_analytic_resident call stored both halves of the phasors with nz, nsel and M = R * S as given here. */
int gpcsd_plv_resident(gpcsd_ctx *ctx, int nz, int nsel, int R, int S);
/* Power spectrum of a field along time, averaged over the trials.  Every step of a periodogram of fixed length but the final modulus
 * is linear -- window, detrend, zero-padded FFT, scaling -- so it is ONE complex matrix A = A_re + i A_im (nrow, nts), keeping a
 * frequency keeps a row (gpcsd_amd.utility_functions.spectral_operator builds it).  NO REFERENCE COUNTERPART in the package; usage
 * note: it replaces the scipy.signal.periodogram(..., detrend=False, axis=1) calls on csd_pred, csd_pred_list, the LFP forms and the
 * recording and the mean over the trials that follows (auditory_lfp/fit_gpcsd_baseline.py:189-195, neuropixels/fit_gpcsd2d.py:120-128).
 * x (nz, nts, R, S): R trials, S draws per trial with the draw index innermost (S = 1 for posterior means; gpcsd_sample_posterior's
 * layout otherwise), m = r S + s:
 *   X[z, j, m] = sum_t A[j, t] x[z, t, m]                                    (one fp64 MFMA product for both parts)
 *   power[z, j, r, s] = Re X^2 + Im X^2,     psd[z, j, s] = 1/R sum_r power[z, j, r, s]
 * psd (nz, nrow, S) is required; power, X_re, X_im (nz, nrow, R, S each) may be NULL and are then neither stored on the device nor
 * touched.  The sum over the trials runs in a fixed order (per column tile in trial order, then over the tiles of a site) without
 * atomics: the same call returns the same bits, and psd has the same bits whichever optional outputs are asked for.  Host arrays:
 * upload, two launches, download.  rc -3: NULL inputs or an empty shape; GPCSD_ERR_CAPACITY (before anything is read): R * S >=
 * GPCSD_MAX_GEMM_LD_KMAJOR, nts >= 2^22, nz * R * S >= 2^31, nrow * nts >= 2^28. */
int gpcsd_power_spectrum(gpcsd_ctx *ctx, const double *x, int nz, int nts, int R, int S, const double *A_re, const double *A_im, int nrow,
                         double *psd, double *power, double *X_re, double *X_im);
/* Same computation (NO REFERENCE COUNTERPART in the package; usage note as gpcsd_power_spectrum: auditory_lfp/fit_gpcsd_baseline.py:189-195,
 * neuropixels/fit_gpcsd2d.py:120-128) on a field that is ALREADY in HBM: the named ctx-owned device buffer src_name from src_offset
 * doubles on (as gpcsd_analytic_resident), read as (nz, nts, R, S).  psd -> "spec_psd" (nz * nrow * S doubles) always; want_mask: bit 0
 * power -> "spec_power", bit 1 X_re -> "spec_re", bit 2 X_im -> "spec_im" (nz * nrow * R * S doubles each, for gpcsd_fetch /
 * gpcsd_device_buffer / gpcsd_cross_spectrum_resident); outputs not asked for are not stored.  Collects a queued prediction's
 * deferred status first (rc > 0 as gpcsd_fetch), waits for its own work and leaves every other buffer alone (the prediction, phase
 * and PLV buffers among them).  rc -2: no buffer of that name; rc -3: bad arguments, the source is one of the call's buffers, or it
 * holds fewer than src_offset + nz * nts * R * S doubles; capacity as gpcsd_power_spectrum. */
int gpcsd_power_spectrum_resident(gpcsd_ctx *ctx, const char *src_name, long src_offset, int nz, int nts, int R, int S, const double *A_re,
                                  const double *A_im, int nrow, int want_mask);
/* Cross-spectral matrix and magnitude-squared coherence of ALL site pairs from the coefficients X = X_re + i X_im (nz, nrow, R, S) of
 * gpcsd_power_spectrum.  NO REFERENCE COUNTERPART in the package; usage note: the amplitude-weighted companion of gpcsd_plv for the
 * spectra of auditory_lfp/fit_gpcsd_baseline.py:189-195 and neuropixels/fit_gpcsd2d.py:120-128.  For every draw s and kept row j,
 *   s_re + i s_im [s, j, a, b] = 1/R sum_r X[a] conj(X[b])         = scipy.signal.csd(x_b, x_a) averaged over the trials (SciPy
 *   coh[s, j, a, b] = (s_re^2 + s_im^2) / (s_re[a, a] s_re[b, b])    conjugates its FIRST argument): the orientation of gpcsd_plv
 * in the scaling of the operator that made X; the ranks of a trial-sharded job add R (s_re + i s_im) and form coh after the sum.  coh
 * is 0 where its denominator is 0 (an all-zero site).  Outputs (S, nrow, nz, nz) each, any may be NULL.  The matrix is gpcsd_plv's
 * kernel on X: s_re and coh are symmetric, s_im antisymmetric BIT FOR BIT, the diagonal of s_im is 0 and that of coh 1 (or 0); fixed
 * summation order, no atomics.  rc -3: NULL inputs or an empty shape; capacity as gpcsd_plv. */
int gpcsd_cross_spectrum(gpcsd_ctx *ctx, const double *X_re, const double *X_im, int nz, int nrow, int R, int S, double *s_re, double *s_im,
                         double *coh);
/* Same computation (NO REFERENCE COUNTERPART in the package; usage note as gpcsd_cross_spectrum: auditory_lfp/fit_gpcsd_baseline.py:189-195,
 * neuropixels/fit_gpcsd2d.py:120-128) on the coefficients gpcsd_power_spectrum_resident left in "spec_re" / "spec_im"; results in the
 * named device buffers "xspec_re", "xspec_im", "xspec_coh" (S * nrow * nz * nz doubles each).  Waits for its own work and leaves every
 * other buffer alone.  rc -4 unless the last gpcsd_power_spectrum_resident call stored both halves of the coefficients with nz, nrow,
 * R and S as given here. */
int gpcsd_cross_spectrum_resident(gpcsd_ctx *ctx, int nz, int nrow, int R, int S);
/* Solve L^T X = B with the lower Cholesky factor L (n, n): the transposed companion of gpcsd_trsm_lower, same inverted-diagonal-block
 * + GEMM scheme, host arrays, B and X (n, nrhs); L is not modified.  No reference counterpart in the package; it serves
 * gpcsd_torus_graph (auditory_lfp/torus_graph_fit.py, neuropixels/fit_torus_graph.py: phi = L^-T L^-1 H). */
int gpcsd_trsm_lower_trans(gpcsd_ctx *ctx, const double *L, int n, const double *B, int nrhs, double *X);
/* Phase-difference torus graph by score matching, for B weighted replicates of the trials (bootstrap resamples as multiplicity
 * vectors).  No reference counterpart in the package; usage note: it replaces the torusGraphs(X, selMode=(False, True, False)) fit and
 * the bootstrap loop around it that the reference's analyses end with (auditory_lfp/torus_graph_fit.py,
 * neuropixels/fit_torus_graph.py), which call a package that is not part of the reference.  Unit phasors u = u_re + i u_im (d, N) of d
 * nodes over N trials; pairs p = (i, j), i < j, in the order of np.triu_indices(d, 1), P = d (d - 1) / 2, m = 2 P.  Per trial
 * c_p = cos(x_i - x_j) = re_i re_j + im_i im_j, s_p = sin(x_i - x_j) = im_i re_j - re_i im_j, S = (c_0, s_0, c_1, s_1, ...), and the
 * m x d Jacobian D with D[2p][i] = -s_p, D[2p][j] = s_p, D[2p+1][i] = c_p, D[2p+1][j] = -c_p.  With weights w[b][n] >= 0 (B, N) and
 * W_b their row sums (weights == NULL with B == 1: all ones),
 *   Gamma_b = 1/W_b sum_n w[b][n] D_n D_n^T,   H_b = 2/W_b sum_n w[b][n] S_n,   phi_b = Gamma_b^-1 H_b        (dense Cholesky, fp64 MFMA)
 * and for replicate 0 only  r_n = D_n (D_n^T phi_0) - 2 S_n,  Sigma = Gamma_0^-1 (1/W_0 sum_n w[0][n] r_n r_n^T) Gamma_0^-1 / W_0,
 * chi2[p] = phi_p^T (Sigma_pp)^-1 phi_p with the 2 x 2 diagonal block of Sigma (the p-value is exp(-chi2 / 2)).
 * Outputs: phi (B, P, 2); status (B): 0, or 1 + the failing pivot of that replicate's factorisation (a pivot of rounding size counts
 * as failing) -- that replicate's phi is NaN, the others are unaffected; optional (NULL skips the work) and of replicate 0: chi2 (P),
 * gamma0 (m, m) symmetric bit for bit with exact zeros between pairs that share no node, h0 (m).  Fixed summation order, no atomics:
 * the same call returns the same bits, however the replicates are chunked (GPCSD_TORUS_CHUNK_MB megabytes of Gamma and node blocks
 * per chunk, default 256, read per call).  rc 0 when the work ran (failures are in status); rc -3: NULL arguments or B < 1; rc -22:
 * d < 2, N < 1, a negative or non-finite weight, a zero row sum; GPCSD_ERR_CAPACITY: d > 128 (or N >= 2^22), before anything is read. */
int gpcsd_torus_graph(gpcsd_ctx *ctx, const double *u_re, const double *u_im, int d, int N, const double *weights, int B,
                      double *phi, int *status, double *chi2, double *gamma0, double *h0);
/* Same computation (no reference counterpart in the package; usage note as gpcsd_torus_graph: auditory_lfp/torus_graph_fit.py,
 * neuropixels/fit_torus_graph.py) on the unit phasors gpcsd_analytic_resident left in "phasor_re" / "phasor_im", read as
 * (nz, nsel, R): the nodes are the rows sites[0..d) at kept time j, gathered on the device, the R trials are N.  The results are small
 * and come back to the host; every named device buffer of other calls is left alone.  rc -4 unless the last gpcsd_analytic_resident
 * call stored both halves of the phasors with nz, nsel and M = R as given here (posterior draws, S > 1, and trial-sharded contexts
 * are out of scope: fetch the phasors and use gpcsd_torus_graph); rc -3 also for j or a site out of range. */
int gpcsd_torus_graph_resident(gpcsd_ctx *ctx, const int *sites, int d, int j, int nz, int nsel, int R, const double *weights, int B,
                               double *phi, int *status, double *chi2);
/* Kernel CSD in one dimension with Gaussian sources.  No reference counterpart in the package; usage note: these four
 * calls replace the KCSD1D class of the external kcsd package that the reference's comparisons construct, cross-validate and evaluate
 * (simulation_studies/sim_from_gp_1D.py:14,112-127, simple_template_1D.py:99-105, sim_from_gp_1D_mismatch.py,
 * auditory_lfp/fit_mean_function.py:31,112-115).  This is the project's closed-form statement of the method, not that package's
 * table-interpolated one.
 *
 * One basis: out (M, npts) row-major.  which == 1, the source basis (the b_src_matrix of sim_from_gp_1D.py:114's constructor):
 *   out[j][p] = g(pts[p] - src[j]),  g(u) = exp(-u^2 / (2 sb^2)) / (sqrt(2 pi) sb),  sb = R / 3  (not truncated at |u| = R).
 * which == 0, the potential basis (its b_pot_matrix):
 *   out[j][p] = 1 / (2 varsigma) int_{-R}^{R} [sqrt((u - d)^2 + h^2) - |u - d|] g(u) du,   d = pts[p] - src[j],
 * by Gauss-Legendre with the caller's ngl nodes gl_x / weights gl_w on [-1, 1] (as gpcsd_kphi_1d) on each of the two panels
 * [-R, c], [c, R], c = clip(d, -R, R) -- the integrand has a kink at u = d; the bracket is evaluated as h^2 / (sqrt(v^2 + h^2) + v),
 * v = |u - d|; the 2 ngl terms are added in node order.  Accurate to ~1e-13 of the largest entry for h / R >= 0.05 at ngl = 48; the
 * rule degrades below that.  rc -3: NULL or empty operands, non-finite input, R <= 0, h <= 0, varsigma <= 0, M < 1, ngl < 2, which
 * not 0 / 1; GPCSD_ERR_CAPACITY: M npts >= 2^31. */
int gpcsd_kcsd_basis_1d(gpcsd_ctx *ctx, const double *src, int M, const double *pts, int npts, double R, double h, double varsigma,
                        const double *gl_x, const double *gl_w, int ngl, int which, double *out);
/* The leave-one-electrode-out table of the scan in sim_from_gp_1D.py:115 (cross_validate: one refit per held-out electrode, basis
 * width and ridge) from eigen-decompositions K_r = U_r diag(s_r) U_r^T, in closed form: with d_k = 1 / (max(s_k, 0) + lambda),
 * beta = U diag(d) W, W = U^T V, a_i = sum_k U_ik^2 d_k = ((K + lambda I)^-1)_ii, the residual of electrode i predicted without it is
 * beta_i / a_i, and err[r][l] = sum_i || beta_i / a_i ||_2.  U (nR, n, n) eigenvectors in columns, s (nR, n), W (nR, n, T), lambdas
 * (nlam); err and status (nR, nlam).  A pair with s_min + lambda < n 2^-52 s_max (or not positive) is numerically singular: err =
 * +inf, status = 1, and the other pairs keep their bits.  beta is formed tile by tile on the matrix cores and never stored; fixed
 * summation order, no atomics: the same call returns the same bits, and an entry does not depend on which other lambda values the call
 * holds.  rc -3: NULL or empty operands, non-finite input, lambda < 0; GPCSD_ERR_CAPACITY (before anything is read): n >
 * GPCSD_MAX_EIG_N, nR nlam > 65535, T >= GPCSD_MAX_GEMM_LD_KMAJOR. */
int gpcsd_kcsd_cv(gpcsd_ctx *ctx, const double *U, const double *s, const double *W, int n, int T, int nR, const double *lambdas, int nlam,
                  double *err, int *status);
/* The whole of sim_from_gp_1D.py:114-118 on the device: bases for every R, K = B_pot^T B_pot / M and K~ = B_src^T B_pot / M, one batched
 * eigen-decomposition (negative eigenvalues set to 0), W = U^T V, the table of the kernel-CSD cross-validation, its argmin (best[0] = R
 * index, best[1] = lambda index; on ties the smallest R index, then the smallest lambda index; singular pairs are never selected) and,
 * where an output is not NULL, for the selected pair: csd (n_est, T) = K~ (K + lambda I)^-1 V, pot (n, T) = K (K + lambda I)^-1 V,
 * k_pot (n, n) = K, k_cross (n_est, n) = K~.  ele (n), V (n, T), src (M), est (n_est), Rs (nR), lambdas (nlam).  Only V, the table and
 * the requested outputs cross the bus.  rc 1: every pair is singular (err and status are written), or an eigen-decomposition failed;
 * rc -3 and GPCSD_ERR_CAPACITY as the two calls above (also M, n_est >= 2^22). */
int gpcsd_kcsd_cross_validate(gpcsd_ctx *ctx, const double *ele, int n, const double *V, int T, const double *src, int M, const double *est,
                              int n_est, double h, double varsigma, const double *gl_x, const double *gl_w, int ngl, const double *Rs,
                              int nR, const double *lambdas, int nlam, double *err, int *status, int *best, double *csd, double *pot,
                              double *k_pot, double *k_cross);
/* The estimate of sim_from_gp_1D.py:122-124 (a KCSD1D with given R_init and lambd, then values()) for one pair (R, lambda): the same
 * chain without the table.  rc 1: K + lambda I is numerically singular. */
int gpcsd_kcsd_estimate(gpcsd_ctx *ctx, const double *ele, int n, const double *V, int T, const double *src, int M, const double *est,
                        int n_est, double h, double varsigma, const double *gl_x, const double *gl_w, int ngl, double R, double lambda,
                        double *csd, double *pot, double *k_pot, double *k_cross);
/* copy `count` doubles of the named ctx-owned device buffer to host; rc -2 if the name is unknown; rc > 0 if the
 * asynchronous gpcsd_predict_resident that produced the buffer failed numerically */
int gpcsd_fetch(gpcsd_ctx *ctx, const char *name, double *host, long count);
/* Bytes this context has moved between the caller's PAGEABLE host memory and the device through its own page-locked bounce blocks.
 * The library never passes pageable caller memory to the HIP runtime: the runtime would register those pages with the driver and
 * keep the registration cached, and when the pages are later freed or moved the driver evicts every queue of the process for
 * 10-30 ms (measured: one such stall in every second later step loop of a process, none with this in place).  Arrays in
 * page-locked memory (gpcsd_host_alloc; the class API's results) are copied directly.  No reference counterpart (NumPy arrays
 * in, NumPy arrays out: gpcsd1d.py:21-62). */
int gpcsd_bounce_stats(gpcsd_ctx *ctx, long *bytes);
/* The device address and size in bytes of the same named buffer, for callers that go on working on the GPU instead of copying out:
 * the posterior means gpcsd_predict_resident leaves in HBM ("pred_out_csd", "pred_out_csd_list", "pred_out_lfp",
 * "pred_out_lfp_list": gpcsd1d.py:286-293 / gpcsd2d.py:327-334, layout (nz, nt, ntrials) / (C, nz, nt, ntrials)) gathered over the
 * ranks of a trial-sharded job by an RCCL all-gather (gpcsd_amd/dist.py), or handed to another library (__cuda_array_interface__,
 * DLPack).  Collects a queued prediction's deferred status (rc > 0 as gpcsd_fetch) and drains the context's streams first: the
 * buffer is complete on return and stays valid until the next call that writes it; the library keeps ownership. */
int gpcsd_device_buffer(gpcsd_ctx *ctx, const char *name, unsigned long long *dev_ptr, unsigned long long *bytes);
/* sample_prior with host-supplied standard normals (nx, nt, ntrials): Ls Z_r Lt^T
 * gpcsd1d.py:295-309 / gpcsd2d.py:336-360.  which: GPCSD_PRED_CSD (compute_Ks) or GPCSD_PRED_LFP (compKphi) */
int gpcsd_sample_prior(gpcsd_ctx *ctx, const gpcsd_hparams *hp, int which,
                       const double *normals, int ntrials, double *out);

/* Standard normals from the device generator (no reference counterpart: the reference draws with numpy.random on the host,
 * gpcsd1d.py:300, gpcsd2d.py:341): out[k] = normal number first + k of stream `stream` under `seed`, k < count.  Philox4x32-10
 * (Random123) + Box-Muller in fp64: pair i has counter (lo32(i), hi32(i), stream, 0) and key (lo32(seed), hi32(seed)); with the
 * output words w0..w3, u1 = ((w1 >> 5) 2^26 + (w0 >> 6) + 1/2) 2^-53, u2 likewise from (w3, w2),
 * normal[2 i] = sqrt(-2 ln u1) cos(2 pi u2), normal[2 i + 1] = sqrt(-2 ln u1) sin(2 pi u2).  Every value is a function of
 * (seed, stream, index) alone: ranges split differently give the same bits.  One launch, one download; no upload. */
int gpcsd_normals(gpcsd_ctx *ctx, unsigned long long seed, unsigned stream, unsigned long long first, long count, double *out);
/* The global index of the first resident trial: a rank of a trial-sharded job (gpcsd_shard_block) passes its block's `first`, and
 * gpcsd_sample_posterior then draws for its trials the normals the unsharded job draws for them.  gpcsd_set_lfp resets it to 0
 * (call this after it); gpcsd_dist_set_lfp with replicate = 0 sets every device's to its block's `first`. */
int gpcsd_set_trial_offset(gpcsd_ctx *ctx, long first);
/* Joint draws from the POSTERIOR of the CSD / LFP at sites z and ARBITRARY times tstar, nsamples per resident trial -- of the model
 * whose mean gpcsd_predict_at and whose variance gpcsd_predict_var return (no jitter; a per-electrode noise list on the eigen-index
 * as utility_functions.py:54-63; the LFP is the noise-free potential).  NO REFERENCE COUNTERPART: the reference has sample_prior only
 * (gpcsd1d.py:295-309, gpcsd2d.py:336-360).  Matheron's rule: sample = f_prior + P (y_r - phi - eps) with (f_prior, phi) a joint
 * prior draw Fs Xi Ft^T of the stacked rows [CSD(z) if type & 1; LFP(z) if type & 2; LFP(x)] (ns rows) over the stacked times
 * [t*; t] (ntt = ntstar + nt columns), eps = Qs diag(sqrt(sig2n)) E a noise draw, P the linear map of gpcsd_predict_at.  The factors
 * Fs, Ft come from the symmetric eigensolver (negative eigenvalues of rounding size count as zero; the joint covariances are singular
 * whenever z holds electrodes or t* training times), the spatial one after equilibration to a unit diagonal.  Each draw has the mean
 * of gpcsd_predict_at and the full posterior covariance; the component SUM only (a joint draw does not identify the components).
 * Outputs (either may be NULL): (nz, ntstar, ntrials, nsamples), C order.
 * normals_xi (ntrials, nsamples, ns, ntt) and normals_eps (ntrials, nsamples, nx, nt): host-supplied standard normals -- both or
 * neither (rc -3).  Both NULL: the device generator (gpcsd_normals) with `seed`, stream 0 for Xi and stream 1 for E, the index of
 * an entry its C-order index in those arrays with the GLOBAL trial index (gpcsd_set_trial_offset): the same seed gives the same
 * draws however the call is chunked or sharded.  The draws are processed in chunks of pseudo-trials (trial, draw) whose scratch fits
 * GPCSD_SAMPLE_SCRATCH_MB megabytes (default 2048; read per call).
 * rc -3: bad arguments, nsamples < 1, a user-defined temporal covariance (GPCSD_KIND_HOST: no joint Gram over [t*; t] on the
 * device); GPCSD_ERR_CAPACITY: ns or ntt beyond GPCSD_MAX_EIG_N (checked before z or tstar is read); rc -4 without resident data. */
int gpcsd_sample_posterior(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                           const double *tstar, int ntstar, int type, int nsamples, unsigned long long seed,
                           const double *normals_xi, const double *normals_eps, double *csd, double *lfp);
/* Same computation (no reference counterpart), results left in the named device buffers "post_sample_csd", "post_sample_lfp"
 * (nz*ntstar*ntrials*nsamples each) for gpcsd_fetch / gpcsd_device_buffer.  Waits for its own work: a numerical failure (rc > 0) is
 * returned by the call itself.  The buffers of the posterior means, variances and leave-one-out scores are left alone. */
int gpcsd_sample_posterior_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                                    const double *tstar, int ntstar, int type, int nsamples, unsigned long long seed,
                                    const double *normals_xi, const double *normals_eps);
/* REGION FEATURES of a field x (nz, nts, M), C order, the column m innermost -- a prediction (M = ntrials) or posterior draws
 * (M = ntrials * nsamples, gpcsd_sample_posterior's layout): per labelled region of the (z, t) plane and per column the extrema, where
 * and when they occur, the sums that give the centre of mass, and the largest standardised deviation from a mean.  NO REFERENCE
 * COUNTERPART as a routine: the reference's analysis segments ONE evoked field into labelled regions on the host and takes
 * scipy.ndimage.center_of_mass of each (auditory_lfp/fit_mean_function.py:350-353); these are the same reductions for every column,
 * taken where the field lies.  labels (nz, nts) int32 with values 0..J, 0 the background (ignored); tau (nts) and zeta (nz, dim),
 * dim 1 or 2, the coordinates; mean (nz, nts, R) and isd (nz, nts), both or neither, with M = R * S and column m of trial m / S.
 * feat (J, GPCSD_NFEAT, M), for region j = 1..J (row j - 1) and column m, over the region's points (i, k):
 *   slot 0, 1   max of x and the flat index i * nts + k of its FIRST occurrence in row-major (z, t) order (a double, exact)
 *   slot 2, 3   min of x and the flat index of its first occurrence
 *   slot 4, 5   sum x, sum |x|
 *   slot 6      sum |x| tau[k]
 *   slot 7, 8   sum |x| zeta[i][0], sum |x| zeta[i][1] (0 when dim = 1)
 *   slot 9      max |x - mean[i][k][m / S]| isd[i][k]; NaN when mean / isd are NULL
 * A region without a point gives -inf, -1, +inf, -1, zeros, and -inf in slot 9 when it is asked for.  NaN inputs are NOT supported
 * and nothing checks for them.  Sums are taken in a fixed order that depends on the label map alone, without atomics: the same call
 * returns the same bits, and a column's result does not depend on which other columns are in the call.  Extrema are replaced on
 * strict comparisons in point order.  One upload, three launches, one download.
 * rc -3: NULL or empty arguments, J < 1, a label outside [0, J], mean without isd, R * S != M; GPCSD_ERR_CAPACITY (before anything
 * is read on the device): J > GPCSD_MAX_REGIONS, nz * nts >= 2^31, J * GPCSD_NFEAT * M >= 2^31, M >= 64 * 65535. */
int gpcsd_region_features(gpcsd_ctx *ctx, const double *x, int nz, int nts, long M, const int *labels, int J, const double *tau,
                          const double *zeta, int dim, const double *mean, const double *isd, int R, int S, double *feat);
/* Same computation (no reference counterpart) on a named device buffer from `src_offset` doubles on (as gpcsd_analytic_resident
 * takes its source), read as (nz, nts, M); the features are left in "feat_out" (J * GPCSD_NFEAT * M doubles).  rc -2: no such
 * buffer; -3 also when the buffer is too small or is "feat_out" itself. */
int gpcsd_region_features_resident(gpcsd_ctx *ctx, const char *src_name, long src_offset, int nz, int nts, long M, const int *labels,
                                   int J, const double *tau, const double *zeta, int dim, const double *mean, const double *isd,
                                   int R, int S);
/* The region features of gpcsd_sample_posterior's draws, reduced chunk by chunk INSIDE the sampler (no reference counterpart; the
 * centre of mass as auditory_lfp/fit_mean_function.py:350-353 takes it of one field): arguments, model, normals and chunking of
 * gpcsd_sample_posterior, then labels (nz, ntstar) and J as gpcsd_region_features, tau = tstar and zeta = z.  feat_csd / feat_lfp
 * (J, GPCSD_NFEAT, ntrials * nsamples), column p = r * nsamples + s; either may be NULL.  After the combine pass of a chunk the
 * features of its columns are written to columns [p0, p0 + np) of the result, so nothing but the result grows with nsamples:
 * with keep_draws = 0 a chunk's draws live in a chunk-sized scratch and "post_sample_csd" / "post_sample_lfp" are neither allocated
 * nor touched (csd and lfp must then be NULL, rc -3); with keep_draws != 0 the draws are kept and returned as
 * gpcsd_sample_posterior returns them.  The chunk length counts that scratch either way: both settings form the same draws and so
 * the same features, bit for bit (a chunk may be shorter than gpcsd_sample_posterior's own).
 * with_band != 0 fills slot 9 with the supremum over the region of |draw - mean| / sd: the call first forms the mean of
 * gpcsd_predict_at and the variance of gpcsd_predict_var at the same sites and times, through those calls' internals, into buffers of
 * its own ("feat_mean_csd" / "feat_mean_lfp" (nz, ntstar, ntrials), "feat_var_*" and "feat_isd_*" (nz, ntstar)): "pred_out_*" and
 * "pred_var_*" are not touched.  1 / sd = 1 / sqrt(var) where var > floor * max(var), 0 elsewhere (floor in [0, 1), 1e-10 by
 * convention; points below it drop out of the supremum).  The quantile over the draws of slot 9 is the half-width, in standard
 * deviations, of a simultaneous band over the region.
 * rc -3: as gpcsd_sample_posterior, J < 1, a label outside [0, J], a floor outside [0, 1); GPCSD_ERR_CAPACITY: as
 * gpcsd_sample_posterior and gpcsd_region_features with M = ntrials * nsamples, with_band also as gpcsd_predict_at; everything is
 * checked before any device work. */
int gpcsd_sample_features(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar, int type,
                          int nsamples, unsigned long long seed, const double *normals_xi, const double *normals_eps,
                          const int *labels, int J, int with_band, double floor, int keep_draws, double *feat_csd, double *feat_lfp,
                          double *csd, double *lfp);
/* Same computation (no reference counterpart), the features left in "feat_csd" / "feat_lfp" and, with keep_draws != 0, the draws
 * in "post_sample_csd" / "post_sample_lfp". */
int gpcsd_sample_features_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                                   int type, int nsamples, unsigned long long seed, const double *normals_xi,
                                   const double *normals_eps, const int *labels, int J, int with_band, double floor, int keep_draws);
/* Posterior mean and covariance of J LINEAR FUNCTIONALS <W_j, f> = sum_{z,s} W_j[z, s] f(z, t*_s) of the CSD / LFP field at the sites
 * z and times tstar of gpcsd_predict_at -- a layer and window average, a sink-minus-source contrast, a component's amplitude -- of the
 * model whose mean that call returns (no jitter; a per-electrode noise list on the eigen-index; the LFP is the noise-free potential).
 * NO REFERENCE COUNTERPART.  W (J, nz, ntstar), C order.  With alpha_j^c = (Qs (x) Qt)^T (Kcross (x) k_c(t, t*)) vec(W_j), one
 * (nx, nt) array per functional and temporal component c, and alpha_j^C = sum_c alpha_j^c for the component sum (plane p = C),
 *   mean_p[j, r]  = <alpha_j^p, (Qs^T y_r Qt) / D>
 *   prior_p[j, k] = <W_j, Kzz W_k Ktt_p>,     Kzz the prior spatial covariance at the sites, Ktt_p = k_p(t*, t*), Ktt_C = sum_c Ktt_c
 *   cov_p[j, k]   = prior_p[j, k] - <alpha_j^p, alpha_k^p / D>       (plane C is NOT sum_c cov_c: the components are correlated a
 *                                                                      posteriori)
 * gpcsd_predict_var / gpcsd_predict_at are the special case of point-mass weights.  The covariances are returned UNCLAMPED, are
 * symmetric bit for bit, and read no trial data.  Outputs per quantity (any may be NULL): *_mean_list (n_temporal, J, ntrials),
 * *_mean (J, ntrials), *_cov_list / *_prior_list (n_temporal, J, J), *_cov / *_prior (J, J).  Every sum is formed in a fixed order:
 * the same call returns the same bits.  The scratch -- alpha is n_temporal * J * nx * nt doubles -- is bounded by
 * GPCSD_FUN_SCRATCH_MB megabytes (default 2048; read per call; J = 64 at 384 x 500 with two components, z = x and t* = t needs about 810):
 * GPCSD_ERR_CAPACITY beyond it, or when J > 65535 or a row of J * nt, J * ntstar, ntrials * nt or n_temporal * ntstar doubles
 * reaches 2^22, before z, tstar or W is read.  rc -3: bad arguments, a user-defined temporal covariance (GPCSD_KIND_HOST: no
 * k_c(t*, t*) on the device); rc -4 without resident data. */
int gpcsd_predict_functionals(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                              const double *tstar, int ntstar, const double *W, int J, int type,
                              double *csd_mean_list, double *csd_mean, double *csd_cov_list, double *csd_cov,
                              double *csd_prior_list, double *csd_prior,
                              double *lfp_mean_list, double *lfp_mean, double *lfp_cov_list, double *lfp_cov,
                              double *lfp_prior_list, double *lfp_prior);
/* Same computation (no reference counterpart), results left in the named device buffers "fun_mean_csd" (J*ntrials), "fun_cov_csd",
 * "fun_prior_csd" (J*J), their "_list" forms (n_temporal times that) and the "lfp" ones for gpcsd_fetch / gpcsd_device_buffer.  Waits
 * for its own work: a numerical failure (rc > 0) is returned by the call itself.  The buffers of the posterior means, variances,
 * leave-one-out scores and draws are left alone. */
int gpcsd_predict_functionals_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const double *z, int nz,
                                       const double *tstar, int ntstar, const double *W, int J, int type);
/* The Gram kernel of gpcsd_predict_functionals alone, on host arrays (no reference counterpart; fungram.hip: upload, two launches,
 * download): A (C, nb, J, K), s (nb, K) or NULL, B (nb, N, K) or NULL -> out (C + 1, J, N), N = J when B is NULL,
 *   out[p][j][k] = sum_b sum_i A_p[b][j][i] s[b][i] B[b][k][i],      A_C = sum_c A_c (added in index order, never stored).
 * B NULL: B = A_p, and out[p] is symmetric bit for bit.  The range of b is cut into chunks of gpcsd_fun_gram_chunk(K) whose
 * partial products are added in chunk order: the same call returns the same bits.  rc -3: bad arguments, C outside
 * [1, GPCSD_MAX_TEMPORAL]; GPCSD_ERR_CAPACITY: more than 65535 chunks. */
int gpcsd_fun_gram(gpcsd_ctx *ctx, const double *A, int C, int nb, int J, int K, const double *s, const double *B, int N,
                   double *out);
/* Values of b per chunk of gpcsd_fun_gram: a function of the contracted row length K alone (-3 for K < 1). */
int gpcsd_fun_gram_chunk(int K);

/* Posterior means with MISSING SAMPLES: gpcsd_predict_at of the model conditioned on the observed samples only.  NO REFERENCE
 * COUNTERPART: the reference needs the full (electrode, time, trial) grid.  mask: bytes in the data's layout (nx, nt, mask_trials),
 * C order, non-zero = observed; mask_trials == ntrials, or 1 for one (nx, nt) mask shared by all trials.  Exact, no iteration: with
 * A = Ks (x) Kt + sig2n I of a full trial (no jitter; a noise list on the eigen-index), M the m missing samples of a trial, y~ the
 * trial with zeros on M, c = (A^-1 y~)_M and G = (A^-1)_MM (dense, SPD, one per DISTINCT mask),
 *   A_OO^-1 y_O = [A^-1 (y~ + E_M u)]_O,  u = -G^-1 c,
 * i.e. the full-grid solve of gpcsd_predict_at on the data with u imputed.  The zeros are a SELECTION: a masked-out value is never an
 * arithmetic operand, NaN / Inf there change no bit of any output.  A trial without an observed sample predicts 0.  The same call
 * returns the same bits.  G is assembled in chunks whose scratch fits GPCSD_MASKED_SCRATCH_MB megabytes (default 256; read per call).
 * z, tstar, `type`, outputs and their layouts as gpcsd_predict_at.  rc -3: bad arguments, mask_trials not in {1, ntrials}, a
 * user-defined temporal covariance (GPCSD_KIND_HOST); GPCSD_ERR_CAPACITY, before any data is read: a trial with more than
 * GPCSD_MAX_MISSING missing samples (unless none is observed), or gpcsd_predict_at's limits; rc > 0: numerical failure, a G that is
 * not positive definite included; rc -4 without resident data. */
int gpcsd_predict_masked(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials,
                         const double *z, int nz, const double *tstar, int ntstar, int type,
                         double *csd_list, double *csd, double *lfp_list, double *lfp);
/* Same computation (no reference counterpart), results left in the named device buffers of gpcsd_predict_at_resident.  Waits for its
 * own work: a numerical failure (rc > 0) is returned by the call itself. */
int gpcsd_predict_masked_resident(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials,
                                  const double *z, int nz, const double *tstar, int ntstar, int type, int want_lists);
/* Log-likelihood of the OBSERVED samples under the model of gpcsd_predict_masked (no jitter).  NO REFERENCE COUNTERPART.  mask and
 * mask_trials as gpcsd_predict_masked.  out2 = {sum_r (log det A + log det G_r), sum_r (y~_r^T A^-1 y~_r - c_r^T G_r^-1 c_r)} =
 * {sum_r log det A_OO, sum_r y_O^T A_OO^-1 y_O}; the value is -1/2 out2[0] - 1/2 out2[1], loglik()'s convention without a 2 pi
 * term -- *n_obs (may be NULL) receives the number of observed samples over all trials so that a caller comparing masks can add
 * -1/2 n_obs log(2 pi).  per_trial (ntrials, 2), C order, may be NULL: the two terms of every trial; a trial without an observed
 * sample contributes (0, 0).  Fixed summation orders: the same call returns the same bits.  Return codes as gpcsd_predict_masked. */
int gpcsd_loglik_masked(gpcsd_ctx *ctx, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials, double *out2,
                        double *per_trial, long *n_obs);
/* The Schur complement's assembly alone, on host arrays (no reference counterpart; masked.hip): Qs (nx, nx) and Qt (nt, nt), C order,
 * eigen-index in columns; D (nx, nt) > 0; samples (xi[p], ti[p]), p < m, in any order.  G (m, m), C order, in the caller's order:
 *   G[p][q] = sum_{a,b} Qs[xi[p]][a] Qs[xi[q]][a] Qt[ti[p]][b] Qt[ti[q]][b] / D[a][b]
 * as sum_a Qs[xi[p]][a] Qs[xi[q]][a] H_a[j(p)][j(q)], H_a = Qt_u diag(1 / D[a, :]) Qt_u^T over the distinct times.  Symmetric bit for
 * bit; the same call returns the same bits.  rc -3: NULL or empty arguments, a sample outside the grid; GPCSD_ERR_CAPACITY (before
 * anything is read): m > GPCSD_MAX_MISSING. */
int gpcsd_masked_gram(gpcsd_ctx *ctx, const double *Qs, int nx, const double *Qt, int nt, const double *D,
                      const int *xi, const int *ti, int m, double *G);

/* Per-trial whitened quadratic forms  out[b] = sum( (Qs^T resid_b Qt)^2 / Dvec )  for nb residual matrices at once, given a
 * cached decomposition (Qs, Qt, Dvec) from gpcsd_eig_D.  resid is (nx, nt, nb) C-order like lfp.  This is the projection
 * kernel of loglik (gpcsd1d.py:124-127) exposed for downstream per-trial consumers, e.g. the shift-optimisation objective
 * of auditory_lfp/fit_mean_function.py:311-321 (alpha = Qs^T resid Qt; quad = -0.5 * sum(alpha^2 / Dvec)). */
int gpcsd_whitened_quad(gpcsd_ctx *ctx, const double *Qs, int nx, const double *Qt, int nt, const double *Dvec,
                        const double *resid, int nb, double *out);

/* The trial-shift objective of auditory_lfp/fit_mean_function.py:306-321 and its analytic gradient, with everything resident: a PLAN
 * (this call) uploads once the decomposition (Qs, Qt, Dvec of gpcsd_eig_D, Dvec taken as given), the trials lfp (nx, nt, ntrials), the
 * means mu (nx, nt, nseg + 1) -- background in [..., 0], component i in [..., i + 1] -- and the strictly increasing time grid t (nt),
 * which need not be uniform; it stores the trials as (x, trial, t) and forms the slope tables s_i[x][k] = (y_i[x][k+1] - y_i[x][k]) /
 * (t[k+1] - t[k]).  One plan per context, in the named buffers "shift_*"; a new plan replaces it.  rc -3: NULL inputs, an empty
 * shape, nt < 2, or a t that is not finite and strictly increasing (the previous plan stays); GPCSD_ERR_CAPACITY (before anything is
 * read): nseg > GPCSD_MAX_SHIFT_NSEG, nx > 65535, nt >= 2^22. */
int gpcsd_shift_plan(gpcsd_ctx *ctx, const double *Qs, int nx, const double *Qt, int nt, const double *Dvec, const double *lfp,
                     int ntrials, const double *mu, int nseg, const double *t);
/* B points (trial_idx[b], tau[b][0..nseg)) of the plan's objective (auditory_lfp/fit_mean_function.py:306-321) in one batch:
 *   mean[x][k] = mu_0[x][k] + sum_i y_i[x][lo] + s_i[x][lo] ((t_k + tau_i) - t_lo),  lo = clip(searchsorted_left(t, t_k + tau_i), 1, nt-1) - 1
 *   (scipy.interpolate.interp1d, linear, fill_value="extrapolate": a sample on a knot takes the segment to its left, samples outside
 *   the grid extend the end segments),  r = lfp[:, :, trial] - mean,  alpha = Qs^T r Qt,  beta = alpha / Dvec,  Z = Qs beta Qt^T,
 *   f_out[b] = 1/2 sum alpha beta + 1/2 sum_i ((tau_i - mutau) / sigtau)^2,
 *   g_out[b][i] = -sum_{x,k} Z[x][k] s_i[x][lo(i,k)] + (tau_i - mutau) / sigtau^2   (the derivative on the segments in use: the LEFT
 *   derivative where a sample sits on a knot, tau = 0 included).
 * Only trial_idx, tau, f_out and g_out cross PCIe.  g_out may be NULL: the back-projection and the gradient kernel are then skipped
 * and f_out has the same bits.  Fixed summation order, no atomics: the same call gives the same bits, and the kernels of this path do
 * not see which other points share the batch (the four products are the library's GEMM, whose tile configuration follows the batch's
 * size).  rc -2: no plan; rc -3 (nothing is launched): NULL inputs, B < 1, a trial index outside [0, ntrials), a tau that is
 * not finite, sigtau <= 0; GPCSD_ERR_CAPACITY (nothing is launched): B * nt >= GPCSD_MAX_GEMM_LD_KMAJOR, nx * B or B * nseg * nt >=
 * 2^31 -- evaluate in chunks of B, as the Python layer does. */
int gpcsd_shift_eval(gpcsd_ctx *ctx, const int *trial_idx, const double *tau, int B, double mutau, double sigtau, double *f_out,
                     double *g_out);

/* Precision of the Gram builders (temporal SE / Matern, spatial SE, forward-model weights; covariances.py:50-96,177-232,
 * 257-305): bits = 64 (default) evaluates them exactly as the reference does; bits = 32 is the "fp32 kernel build + fp64
 * factor" variant of the fit benchmark: coordinates and hyper-parameters are rounded to float, exp/log/sqrt are
 * single precision, the result is widened and every later stage (GEMMs, eigensolver, likelihood, gradient) stays fp64.
 * Applies to the operator entry points and to the fused calls of this context. */
int gpcsd_set_gram_precision(gpcsd_ctx *ctx, int bits);

/* Folded-basis GEMMs: with mirror-symmetric electrode and time grids (detected in set_geometry / set_time) loglik and predict
 * run their projections (gpcsd1d.py:124-127, 262-279) as half-size products in the symmetric / antisymmetric basis; same
 * results to rounding, half the flops.  on = 0 / 1 switches the path for this context (default 1; GPCSD_NO_FOLD_GEMM=1 in
 * the environment disables it process-wide), on < 0 only queries.  *calls (optional) receives how many loglik / predict
 * calls of this context have taken the folded path so far. */
/* Multi-GPU from C (one process per GPU): trials are independent, every rank recomputes the (deterministic)
 * decompositions and owns a contiguous block of trials.  gpcsd_shard_block gives rank `rank` of `world` its block
 * [first, first+count) of `ntrials`; the rank uploads lfp[:, :, first:first+count] with gpcsd_set_lfp, calls
 * gpcsd_loglik_parts -> (sum log D, partial quad), sums the partial quad over ranks with the collective of its choice
 * (RCCL / MPI all-reduce of one double) and gpcsd_combine_loglik forms -R/2 sum log D - 1/2 quad (gpcsd1d.py:122,127-128).
 * predict / gpcsd_loglik_grad work on the rank's block the same way (gradient entries and L_loc add over ranks). */
int gpcsd_shard_block(int ntrials, int rank, int world, int *first, int *count);
int gpcsd_combine_loglik(int ntrials_total, double sumlog, double quad_sum_over_ranks, double *out);

/* Decomposition cache: a fused call whose spatial and / or temporal hyper-parameters, grids and precision equal those of
 * the previous fused call on this context reuses that side's eigendecomposition instead of repeating it (predict() right
 * after loglik() / fit(): neuropixels/fit_gpcsd2d.py:101-107; repeated predict() calls).  Kernels are deterministic, so the
 * results are bit-identical either way.  on = 1 / 0 switches it (default on), -1 only queries; *hits counts reused sides. */
int gpcsd_decomposition_cache(gpcsd_ctx *ctx, int on, long *hits);
int gpcsd_fold_gemm(gpcsd_ctx *ctx, int on, long *calls);
/* The paired call gpcsd_loglik_predict_async (loglik gpcsd2d.py:136-151 + predict :289-334 of one step) with EQUAL temporal
 * hyper-parameters in both sets -- the case of every loglik -> predict pair, whose only difference is the spatial jitter -- forms
 * the product X = Y~ Q of the resident data with the temporal basis once and lets the prediction read the log-likelihood's copy:
 * the two replicas of the temporal problem are the same matrix reduced by the same deterministic launches, so the second product
 * would recompute the same bits.  on = 1 / 0 switches it (default 1; GPCSD_PAIR_SHARE_X=0 for new contexts), < 0 only queries;
 * *calls counts the paired calls that shared the product.  Results are bit-identical either way. */
int gpcsd_pair_share_x(gpcsd_ctx *ctx, int on, long *calls);
/* ... and ONE spatial decomposition for the pair when the two sets have equal spatial hyper-parameters and differ by the jitter
 * only -- every loglik -> predict pair: the reference adds jitter * I to Ks in loglik (gpcsd1d.py:116, gpcsd2d.py:139) and not in
 * predict (gpcsd1d.py:258, gpcsd2d.py:296).  eigh(Ks + j I) has the eigenvectors of eigh(Ks) and its spectrum shifted by j
 * (utility_functions.py:58-59 applied to either), so the prediction takes the log-likelihood's eigenvectors, its spectrum minus j
 * and -- with X shared as well -- its projected data.  Exact in exact arithmetic; in floating point the prediction then differs from
 * the separately decomposed one by the eigensolver's own backward error (1e-13 relative at 384 x 500, tests/test_pair_share_s.py).
 * on = 1 / 0 switches it (default 0: it saves a large product and 154 MB of traffic per 384 x 500 x 50 step, but the step measured
 * slower, DESIGN 4.13, and the pair then differs from its fenced calls in the last bits; GPCSD_PAIR_SHARE_S=1 for new contexts),
 * < 0 only queries; *calls counts the pairs that took it. */
int gpcsd_pair_share_s(gpcsd_ctx *ctx, int on, long *calls);
/* Pipelined orthogonal factor (round 5).  The tridiagonal forms (gpcsd_ll_tridiag below) need Q of Kt = Q T Q^T
 * (utility_functions.py:58) and X = Y~ Q before anything else of their tails can start, and both used to wait for the END of the
 * tridiagonalisation -- the longest launch of a step.  Column j of Q only depends on the reflectors in front of it, so the
 * single-workgroup reduction publishes its progress every 64 reflectors and the T factor of that panel, the 64 finished columns of Q
 * and the matching 64 columns of X follow on another stream while the reduction is still at work on the next panel; behind it only
 * the last panel's share is left.  Same reflectors, same T factors; Q and X agree with the unpipelined form to rounding (the products
 * are summed in another order).  Applies to temporal blocks of at most 256 rows after symmetry folding.
 * on = 1 / 0 switches it (default 1; GPCSD_Q_PIPE=0 for new contexts -- cheaper under a profiler that serialises kernels, where a
 * launch that waits for a running one cannot make progress: gpcsd_q_pipeline_stats below), < 0 only queries;
 * *calls counts the temporal chains that took it. */
int gpcsd_q_pipeline(gpcsd_ctx *ctx, int on, long *calls);
/* The one place where a launch waits for a RUNNING kernel of another stream is bounded (0.2 s).  A wait that runs out is a
 * scheduling miss, not a numerical failure (kernels serialised by a profiler or a debugger, an oversubscribed card): the launch
 * leaves the unfinished reflectors alone, and the call that collects the evaluation -- the synchronous call itself,
 * gpcsd_loglik_parts_wait, or whichever call next synchronises behind a gpcsd_predict_resident -- switches the pipeline off for
 * the context (latched), evaluates again behind the end of the reduction (same T, Q, X as with on = 0) and returns that result.
 * *on: the switch as it stands; *timeouts: evaluations repeated for this reason; gate_ticks >= 0 sets the bound in 100 MHz ticks
 * (0: every wait gives up at once -- the test aid that drives the repeat path; GPCSD_QPIPE_GATE_TICKS for new contexts), < 0
 * leaves it.  No reference counterpart (utility_functions.py:58-59 is one LAPACK call). */
int gpcsd_q_pipeline_stats(gpcsd_ctx *ctx, int *on, long *timeouts, long long gate_ticks);
/* gpcsd_predict with host outputs (what the class API's predict() returns, gpcsd1d.py:286-293 / gpcsd2d.py:327-334): the last
 * product of a folded prediction is launched in chunks of prediction sites and every chunk's finished output rows are copied to
 * the caller's arrays while the next chunk computes (231 MB per call at 384 x 500 x 50: the copy is 4 of the call's 5 ms and no
 * longer waits for the whole product).  Applies to outputs of at least 32 MB through the fused last product; same bits.
 * on = 1 / 0 switches it (default 1; GPCSD_PRED_CHUNKED=0 for new contexts), < 0 only queries; *calls counts the calls that took it. */
int gpcsd_predict_chunked_copy(gpcsd_ctx *ctx, int on, long *calls);
/* The log-likelihood of the folded path in the basis U (x) Q instead of U (x) V.  With Kt = m Q T Q^T from the
 * tridiagonalisation alone (Q orthogonal, T tridiagonal) and the spatial side fully decomposed, Ks (x) Kt + sig2 I is a set of
 * SHIFTED TRIDIAGONAL matrices es[x'] m T + sig2 I: sum log D is the sum of the logs of their LDL^T pivots and the quadratic
 * form one forward recurrence per (x', trial) row of U^T Y Q -- exact algebra (gpcsd1d.py:113-128), no temporal eigenvectors, so
 * the log-likelihood does not wait for the temporal divide & conquer (which a prediction still needs and the chain still runs).
 * Same results to rounding (1e-15 relative on the log-likelihood at 384 x 500).  mode: 0 = off (the eigenvector form always),
 * 1 = on wherever it applies (mirror-symmetric time grid with halves beyond the Jacobi size, scalar noise, folded path),
 * 2 = on while max(nx, 64) * nt * ntrials <= 11 * 2^20 (the default: above that the step is bound by its GEMMs and the form
 *     costs 2-10 %),
 * < 0 only queries; GPCSD_LL_TRIDIAG=0|1|2 sets the mode of new contexts.  *calls counts the log-likelihoods evaluated this
 * way.  DESIGN.md 9. */
/* Late status words.  A temporal chain all of whose consumers take the tridiagonal form (a log-likelihood in this form; the
 * paired call when its prediction is in that form too, the default) runs its tridiagonalisation, T factors and Q only: the
 * divide & conquer and the back-transformation are not queued, and the context is idle behind every value-returning call.  Only
 * the paired call gpcsd_loglik_predict_async with an EIGENVECTOR-form prediction (GPCSD_PRED_TRIDIAG=0, or shapes the solve
 * kernel does not take) queues those two stages behind a log-likelihood that does not wait for them; they report into status
 * words of their own, which the call that JOINS that chain collects (the prediction's wait / gpcsd_device_synchronize): a failure
 * there is that call's rc > 0, never the log-likelihood's (whose value does not depend on them) and never an unrelated later
 * call's. */
int gpcsd_ll_tridiag(gpcsd_ctx *ctx, int on, long *calls);
/* Rank-revealing early exit of the tridiagonalisation (no reference counterpart -- numpy.linalg.eigh,
 * utility_functions.py:58-59, reduces every column): for matrices the LIBRARY's own Gram fills announce as positive
 * semi-definite (Ks, Kt of the model with non-negative variances and jitter; never a caller's matrix handed to gpcsd_eigh /
 * gpcsd_eig_D / gpcsd_set_host_temporal_gram) of at most 192 rows after folding, the Householder reduction stops once the trace
 * still to be reduced is below 64 unit roundoffs of the matrix's trace (backward error <= that trace).  on = 1 / 0 switches it
 * for this context (default 1; GPCSD_TAIL_EARLY_EXIT=0 for new contexts), < 0 only queries; *previous receives the setting
 * before the call.  Both settings are tested against each other (tests/test_hip_fullsize.py::test_tail_early_exit_*). */
int gpcsd_tail_early_exit(gpcsd_ctx *ctx, int on, int *previous);
/* Test aid, off by default and never read from the environment: with on = 1 the divide & conquer stage of a staged temporal
 * chain reports numerical failure 3 for every replica (drives the late status words above). */
int gpcsd_debug_fault_stage2(gpcsd_ctx *ctx, int on);

/* ---- several devices from ONE process ------------------------------------------------------- */
/* SURVEY 8(b)'s gpcsd_dist_*: one context per device, driven by one host process (the Python layer uses one process per GPU
 * over torch.distributed / RCCL instead: gpcsd_amd/dist.py).  The path has no device-to-device exchange: trials
 * are independent, every device recomputes the deterministic decompositions, and what is combined is one double per device --
 * summed on the host in device order.  devices == NULL: ordinals 0..ndev-1 (an ordinal may repeat: two contexts on one GPU). */
typedef struct gpcsd_dist gpcsd_dist;
int gpcsd_dist_create(int ndev, const int *devices, gpcsd_dist **out);
int gpcsd_dist_destroy(gpcsd_dist *dist);
int gpcsd_dist_size(gpcsd_dist *dist);
int gpcsd_dist_ctx(gpcsd_dist *dist, int i, gpcsd_ctx **ctx);          /* the i-th context, for the per-context knobs */
const char *gpcsd_dist_last_error(gpcsd_dist *dist);
/* the gpcsd_set_* calls on every device */
int gpcsd_dist_set_geometry_1d(gpcsd_dist *dist, const double *x, int nx, const double *gl_x, const double *gl_w, int ngl);
int gpcsd_dist_set_geometry_2d(gpcsd_dist *dist, const double *xy, int nx, const double *gl_x1, const double *gl_w1, int ngl1,
                               const double *gl_x2, const double *gl_w2, int ngl2);
int gpcsd_dist_set_time(gpcsd_dist *dist, const double *t, int nt);
/* lfp (nx, nt, ntrials).  replicate = 0: device i gets the block of trials gpcsd_shard_block gives rank i (trial sharding,
 * BASELINE cfg4); replicate = 1: every device gets all trials (restart sharding, BASELINE cfg5) */
int gpcsd_dist_set_lfp(gpcsd_dist *dist, const double *lfp, int nx, int nt, int ntrials, int replicate);
/* loglik() over all trials  gpcsd1d.py:113-128 / gpcsd2d.py:136-151: queued on every device, partial sums added in device order */
int gpcsd_dist_loglik(gpcsd_dist *dist, const gpcsd_hparams *hp, double *out);
/* as gpcsd_loglik_grad, summed over the devices' blocks of trials */
int gpcsd_dist_loglik_grad(gpcsd_dist *dist, const gpcsd_hparams *hp, double *out2, double *grad, int ngrad);
/* the restarts of fit()  gpcsd1d.py:193-220: set k evaluated on device k mod ndev (needs replicate = 1); arguments as
 * gpcsd_loglik_grad_batch */
int gpcsd_dist_loglik_grad_batch(gpcsd_dist *dist, const gpcsd_hparams *hps, int nsets, double *out2, double *grad, int ngrad,
                                 int *status);
/* predict() over all trials  gpcsd1d.py:248-293 / gpcsd2d.py:289-334: outputs as gpcsd_predict, assembled from the devices' blocks */
int gpcsd_dist_predict(gpcsd_dist *dist, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                       int type, double *csd_list, double *csd, double *lfp_list, double *lfp);

/* ---- measurement --------------------------------------------------------------- */
/* When enabled, every launch of a named hot kernel (or kernel family) is bracketed by hipEvents on the stream it runs on.
 * on = 0 off; 1 fenced: every fused call synchronises, asynchronous / paired calls are evaluated one by one, chains run
 * eagerly; 2 asynchronous: events only, queued and paired calls stay queued and paired (what bench.py's timed step does),
 * chains run eagerly so the scopes inside them see their kernels; 3 as 2 with the chains replayed as hipGraphs (only the
 * scopes around whole chains and the GEMMs record).  gpcsd_prof_get waits for the recorded events. */
int gpcsd_prof_enable(gpcsd_ctx *ctx, int on);
/* Modes 2 / 3: duration (ms) of the last launch of the single-workgroup tridiagonalisation tail -- the kernel with the
 * largest share of GPU time -- in a chain (region 0: temporal, 1: spatial, 2: other), from wall-clock stamps its workgroups
 * write themselves: the one way to time it inside a replayed hipGraph.  Valid once that chain has finished. */
int gpcsd_prof_tail_clock(gpcsd_ctx *ctx, int region, double *ms, int *nwg, double *flops);
int gpcsd_prof_reset(gpcsd_ctx *ctx);
/* total ms, launch count and algorithmic flops accumulated under `name`; rc -2 if unknown */
int gpcsd_prof_get(gpcsd_ctx *ctx, const char *name, double *ms, long *count, double *flops);
/* names, ';'-separated, into buf */
int gpcsd_prof_names(gpcsd_ctx *ctx, char *buf, int buflen);
/* back-to-back v_mfma_f64_16x16x4_f64 microbenchmark: measured TFLOP/s */
int gpcsd_mfma_f64_peak(gpcsd_ctx *ctx, double *tflops);
/* average ms per launch of the fp64 MFMA GEMM on device-resident pseudo-random operands; cfg 0 = automatic tile
 * configuration, 1, 2, 3 or 5 = forced (tuning aid) */
int gpcsd_gemm_bench(gpcsd_ctx *ctx, int transA, int transB, int M, int N, int K, int cfg, int reps, double *ms_out);
/* average ms of the blocked Cholesky (numpy.linalg.cholesky of gpcsd1d.py:303-304 / gpcsd2d.py:343-350; the dense cross-check's
 * factor at N = nx * nt) on a device-resident, device-generated SPD test matrix of order n; events on the call's own stream
 * around the factorisation alone.  Kernel split through the profiling scopes (potrf_*). */
int gpcsd_potrf_bench(gpcsd_ctx *ctx, int n, int reps, double *ms_out);
/* how many of the factorisation's gate launches (the one-wave launches that hold the trailing update back until the next diagonal
 * block's workgroup is resident, numpy.linalg.cholesky at gpcsd1d.py:303-304) gave up waiting since the context was created:
 * the gates steer the order of execution only, so this is a performance counter, never an error */
int gpcsd_potrf_gate_timeouts(gpcsd_ctx *ctx, long *count);
/* phase split (us) of the one-workgroup 128 x 128 factor + invert launch inside that Cholesky: {load, serial panels, rank-16
 * MFMA updates, store L, diagonal-block inverses, doubling levels 16 / 32 / 64, store X, total} -- a tuning aid */
int gpcsd_potrf_diag_probe(gpcsd_ctx *ctx, double *out10);
/* streaming copy microbenchmark over `bytes` bytes: measured GB/s (read+write counted) */
int gpcsd_hbm_copy_peak(gpcsd_ctx *ctx, long bytes, double *gbs);
/* the device generator of gpcsd_normals alone: `count` normals into a device buffer, `reps` launches between two events, nothing
 * copied out; measured GB/s of normals WRITTEN (the copy peak above counts its reads too: compare with half of it) */
int gpcsd_normals_bench(gpcsd_ctx *ctx, long count, int reps, double *gbs);

#ifdef __cplusplus
}
#endif
#endif /* GPCSD_HIP_H */
