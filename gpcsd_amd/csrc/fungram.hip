// The long-K scaled Gram of gpcsd_predict_functionals (gfx950), FunGramDesc in kernels.hpp:
//
//   out[p][j][k] = sum_b sum_i A_p[b][j][i] s[b][i] B[b][k][i]            b < nb, i < K, p = 0 .. C
//
// A is (C, nb, J, K); plane p = C reads the sum over c of the C operand tiles, added in registers in index order between the
// global load and the LDS store -- no summed copy of A exists in memory (gemm_var_kernel's treatment of its component-sum plane).
// s (nb, K) or null scales the A tile once per element on its way to LDS (one rounded product, as GemmDesc::kscale).  B is A_p
// itself (the symmetric form: only tiles on or below the diagonal run, and every entry above the diagonal is the entry below it,
// bit for bit) or a separate (nb, N, K) operand shared by all planes.  Both operands are K-contiguous.
//
// J and N are tens to a few hundred, the contracted length nb K is long (192 000 at 384 x 500): one 64 x 64 tile per workgroup
// would leave the machine idle, so the range of b is cut into chunks of fun_gram_chunk(K) -- a function of K alone -- and
//
//   fun_gram_kernel      grid (tiles, chunks, C + 1): one partial tile per chunk into `part` [plane][chunk][J][N]
//   fun_reduce_kernel    out[p][j][k] = the partials added in chunk order; symmetric form: the entry (max(j,k), min(j,k)) for both
//
// No atomics, and a partial depends on its chunk alone: the same bits on every call.  The kernel is bound by the HBM reads of A
// (each element once per plane that uses it), not by MFMA.
//
// Conventions of masked.hip / gemm_f64.hip: 256 threads = four waves of 2 x 2 fragments of 16 x 16 (v_mfma_f64_16x16x4_f64), K
// tiles of 16, [o][k] operand tiles with a row stride of BK + 1, the next tile's global loads in flight under the current tile's
// MFMAs.  Edges: a row past J (N) reads the last valid row -- its accumulators are never stored --, an index past K reads the last
// valid one and is zeroed on its way to LDS.  Fragment maps: A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15],
// C/D lane l reg r holds C[(l >> 4) + 4 r][l & 15].
#include <algorithm>

#include "kernels.hpp"

namespace gpcsd {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef const volatile double __attribute__((address_space(3))) *lds_frag_ptr;
#define LDS_FRAG(p) (*(lds_frag_ptr)(p))

namespace {
constexpr int NT = 256, BO = 64, BK = 16, LDK = BK + 1;
constexpr int T_ELEMS = BO * LDK;
constexpr int PER = BO * BK / NT;          // 4 consecutive k of one row per thread and operand
constexpr int FUN_CHUNK_LEN = 512;         // contracted elements per chunk, rounded down to whole b (at least one)

struct FunK {
    const double *A;             // (C, nb, J, K)
    const double *s;             // (nb, K) or nullptr
    const double *B;             // (nb, N, K) or nullptr: B = A_p
    int C, nb, J, K, N;
    int cb, nchunk;              // b per chunk, chunks
    int tiles_n;                 // column tiles (separate B)
    double *part;                // [plane][chunk][J][N]
};
}  // namespace

int fun_gram_chunk(int K) { return std::max(1, FUN_CHUNK_LEN / std::max(K, 1)); }

__global__ __launch_bounds__(256) void fun_gram_kernel(FunK g) {
    __shared__ double lds[2 * T_ELEMS];
    double *const lA = lds, *const lB = lds + T_ELEMS;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const bool self = g.B == nullptr;
    int tm, tn;                                                // wave-uniform
    if (self) {                                                // tile t of the lower triangle, row by row
        tm = 0;
        while ((tm + 1) * (tm + 2) / 2 <= (int)blockIdx.x) ++tm;
        tn = (int)blockIdx.x - tm * (tm + 1) / 2;
    } else {
        tm = blockIdx.x / g.tiles_n;
        tn = blockIdx.x % g.tiles_n;
    }
    const bool diag = self && tm == tn;                        // one load serves both operands
    const int chunk = blockIdx.y, plane = blockIdx.z;
    const bool all = plane == g.C;                             // the plane of the component sum
    const int ncomp = all ? g.C : 1;
    const int N = self ? g.J : g.N;
    const int b0 = chunk * g.cb, b1 = min(g.nb, b0 + g.cb);
    const int K = g.K, nkt = (K + BK - 1) / BK;
    const int ntile = (b1 - b0) * nkt;

    // this thread's slot of an operand tile: row lr, k = lk .. lk + 3
    const int lr = tid >> 2, lk = (tid & 3) * PER;
    const int rowA = min(tm * BO + lr, g.J - 1), rowB = min(tn * BO + lr, N - 1);
    const long JK = (long)g.J * K, planeA = (long)g.nb * JK;
    const double *const baseA = g.A + (all ? 0L : (long)plane * planeA) + (long)rowA * K;
    const double *const baseB = self ? g.A + (all ? 0L : (long)plane * planeA) + (long)rowB * K : g.B + (long)rowB * K;
    const long strideB = self ? JK : (long)g.N * K;            // from one b to the next
    const int compB = self ? ncomp : 1;

    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

    double ra[PER], rb[PER], rs[PER];
    auto load = [&](int t) {                                   // tile t of the chunk: b = b0 + t / nkt, k0 = (t % nkt) * BK
        const int b = b0 + t / nkt, k0 = (t % nkt) * BK + lk;
        int kk[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) kk[i] = min(k0 + i, K - 1);
        const double *pa = baseA + (long)b * JK;
#pragma unroll
        for (int i = 0; i < PER; ++i) ra[i] = pa[kk[i]];
        for (int cc = 1; cc < ncomp; ++cc) {                   // (wave-uniform: the sum plane only)
            pa += planeA;
#pragma unroll
            for (int i = 0; i < PER; ++i) ra[i] += pa[kk[i]];
        }
        if (!diag) {
            const double *pb = baseB + (long)b * strideB;
#pragma unroll
            for (int i = 0; i < PER; ++i) rb[i] = pb[kk[i]];
            for (int cc = 1; cc < compB; ++cc) {
                pb += planeA;
#pragma unroll
                for (int i = 0; i < PER; ++i) rb[i] += pb[kk[i]];
            }
        }
        if (g.s) {
            const double *ps = g.s + (long)b * K;
#pragma unroll
            for (int i = 0; i < PER; ++i) rs[i] = ps[kk[i]];
        }
    };
    auto store = [&](int t) {
        const int k0 = (t % nkt) * BK + lk;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const bool in = k0 + i < K;
            const double a = ra[i], b = diag ? a : rb[i];
            lA[lr * LDK + lk + i] = in ? (g.s ? a * rs[i] : a) : 0.0;
            lB[lr * LDK + lk + i] = in ? b : 0.0;
        }
    };
    const double *const srA = lA + (wr * 32 + fr) * LDK + fq;
    const double *const srB = lB + (wc * 32 + fr) * LDK + fq;

    if (ntile > 0) load(0);
    for (int t = 0; t < ntile; ++t) {
        store(t);
        __syncthreads();
        if (t + 1 < ntile) load(t + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = LDS_FRAG(srA + i * 16 * LDK + ks * 4);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = LDS_FRAG(srB + j * 16 * LDK + ks * 4);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    double *const out = g.part + ((long)plane * g.nchunk + chunk) * g.J * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int row = tm * BO + wr * 32 + i * 16 + fq + 4 * r4;
            if (row >= g.J) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = tn * BO + wc * 32 + j * 16 + fr;
                if (col >= N) continue;
                out[(long)row * N + col] = acc[i][j][r4];
            }
        }
}

// list[p][j][k] (p < C) and sum[j][k] (p = C) = the chunks' partials in chunk order; sym: both (j, k) and (k, j) from the partials
// of the entry on or below the diagonal
__global__ __launch_bounds__(256) void fun_reduce_kernel(const double *__restrict__ part, int nchunk, int C, int J, int N, int sym,
                                                         double *__restrict__ list, double *__restrict__ sum) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, JN = (long)J * N;
    const int plane = blockIdx.y;
    if (e >= JN) return;
    int j = (int)(e / N), k = (int)(e % N);
    if (sym && k > j) {
        const int tmp = j;
        j = k;
        k = tmp;
    }
    const double *p = part + (long)plane * nchunk * JN + (long)j * N + k;
    double v = 0.0;
    int c = 0;
    for (; c + 16 <= nchunk; c += 16) {                        // sixteen loads in flight, added in chunk order
        double x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = p[(long)(c + u) * JN];
#pragma unroll
        for (int u = 0; u < 16; ++u) v += x[u];
    }
    for (; c < nchunk; ++c) v += p[(long)c * JN];
    double *const out = plane == C ? sum : list + (long)plane * JN;
    out[e] = v;
}

void k_fun_gram(gpcsd_ctx *c, const FunGramDesc &d, hipStream_t s) {
    GP_REQUIRE(d.A && d.part && d.list && d.sum && d.C >= 1 && d.C <= GPCSD_MAX_TEMPORAL && d.nb > 0 && d.J > 0 && d.K > 0 &&
                   (d.B == nullptr || d.N > 0),
               -3, "fun_gram: bad problem");
    const int N = d.B ? d.N : d.J;
    FunK k;
    k.A = d.A; k.s = d.s; k.B = d.B;
    k.C = d.C; k.nb = d.nb; k.J = d.J; k.K = d.K; k.N = N;
    k.cb = fun_gram_chunk(d.K);
    k.nchunk = ceil_div(d.nb, k.cb);
    k.tiles_n = ceil_div(N, BO);
    k.part = d.part;
    const long tm = ceil_div(d.J, BO);
    const long tiles = d.B ? tm * k.tiles_n : tm * (tm + 1) / 2;
    GP_REQUIRE(k.nchunk <= 65535 && tiles < (1L << 31) && (long)d.J * N < (1L << 31), GPCSD_ERR_CAPACITY,
               "fun_gram: %d chunks of the contracted range (at most 65535) or %ld output tiles exceed one launch", k.nchunk, tiles);
    ProfScope ps(c, d.prof_name, 2.0 * (double)d.J * N * (double)d.nb * d.K * (d.C + 1), s);
    hipLaunchKernelGGL(fun_gram_kernel, dim3((unsigned)tiles, (unsigned)k.nchunk, (unsigned)(d.C + 1)), dim3(NT), 0, s, k);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fun_reduce_kernel, dim3((unsigned)ceil_div((long)d.J * N, 256), (unsigned)(d.C + 1)), dim3(256), 0, s,
                       (const double *)d.part, k.nchunk, d.C, d.J, N, d.B ? 0 : 1, d.list, d.sum);
    GP_HIP(hipGetLastError());
}

size_t fun_gram_part_elems(int C, int nb, int J, int K, int N) {
    return (size_t)(C + 1) * ceil_div(nb, fun_gram_chunk(K)) * (size_t)J * N;
}

// in (J, n1, n2) -> out (n1, J, n2)
__global__ __launch_bounds__(256) void fun_relayout_kernel(const double *__restrict__ in, int J, int n1, int n2, double *__restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, tot = (long)J * n1 * n2;
    if (e >= tot) return;
    const int i2 = (int)(e % n2);
    const long r = e / n2;
    const int j = (int)(r % J), i1 = (int)(r / J);
    out[e] = in[((long)j * n1 + i1) * n2 + i2];
}
void k_fun_relayout(gpcsd_ctx *c, const double *in, int J, int n1, int n2, double *out, hipStream_t s) {
    const long tot = (long)J * n1 * n2;
    GP_REQUIRE(tot > 0 && tot < (1L << 31) * 256, GPCSD_ERR_CAPACITY, "fun_relayout: too many elements");
    ProfScope ps(c, "fun_relayout", 0.0, s);
    hipLaunchKernelGGL(fun_relayout_kernel, dim3((unsigned)ceil_div(tot, 256)), dim3(256), 0, s, in, J, n1, n2, out);
    GP_HIP(hipGetLastError());
}

// prior[p][j][k] = raw[p][max(j,k)][min(j,k)] (both triangles from the lower one), cov = prior - expl, p < planes
__global__ __launch_bounds__(256) void fun_finish_kernel(const double *__restrict__ raw, const double *__restrict__ expl, int J,
                                                         double *__restrict__ prior, double *__restrict__ cov) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x, JJ = (long)J * J;
    if (e >= JJ) return;
    const long o = (long)blockIdx.y * JJ;
    const int j = (int)(e / J), k = (int)(e % J);
    const double p = raw[o + (long)max(j, k) * J + min(j, k)];
    prior[o + e] = p;
    cov[o + e] = p - expl[o + e];
}
void k_fun_finish(gpcsd_ctx *c, const double *raw, const double *expl, int J, int planes, double *prior, double *cov, hipStream_t s) {
    GP_REQUIRE(raw && expl && prior && cov && J > 0 && planes > 0 && (long)J * J < (1L << 31), -3, "fun_finish: bad problem");
    ProfScope ps(c, "fun_finish", 0.0, s);
    hipLaunchKernelGGL(fun_finish_kernel, dim3((unsigned)ceil_div((long)J * J, 256), (unsigned)planes), dim3(256), 0, s, raw, expl, J,
                       prior, cov);
    GP_HIP(hipGetLastError());
}

}  // namespace gpcsd
