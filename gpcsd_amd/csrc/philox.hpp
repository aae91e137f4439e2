// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and the
// fp64 Box-Muller pair on top of it.  Counter-based: every output is a function of (seed, stream, index) alone, so a value does not
// depend on the grid that produced it, on how a range was split into launches, or on which rank drew it.  Host and device compile the
// same text.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPCSD_HD __host__ __device__ __forceinline__
#else
#define GPCSD_HD inline
#endif

namespace gpcsd {

struct Philox4 {
    uint32_t w[4];
};

// ten rounds on counter c with key k: p0 = M0 c0, p1 = M1 c2 (64-bit products), c <- (hi(p1)^c1^k0, lo(p1), hi(p0)^c3^k1, lo(p0)),
// then the key is bumped by the Weyl constants
GPCSD_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// 53 bits of two words, centred: ((hi >> 5) 2^26 + (lo >> 6) + 1/2) 2^-53.  The integer part is exact; adding the half rounds to
// even above 2^52, so the value lies in (0, 1] and is never 0: the logarithm below is finite.
GPCSD_HD double philox_u53(uint32_t lo, uint32_t hi) {
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * 0x1p-53;
}

// pair i of stream `stream` under `seed`: normal[2 i] = n0, normal[2 i + 1] = n1
GPCSD_HD void philox_normal_pair(uint64_t seed, uint32_t stream, uint64_t i, double &n0, double &n1) {
    const Philox4 p = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = philox_u53(p.w[0], p.w[1]), u2 = philox_u53(p.w[2], p.w[3]);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586476925 * u2, &sn, &cs);
    n0 = r * cs;
    n1 = r * sn;
}

}  // namespace gpcsd
