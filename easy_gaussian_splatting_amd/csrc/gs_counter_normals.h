// gs_counter_normals.h -- the counter-based draw of the budget noise (gs_mcmc.hip; DESIGN.md "Training to a budget"): Philox4x32-10,
// the two elementary functions the Box-Muller step needs, and the normals of one Gaussian.  Plain C++ that compiles for the device
// and for the host alike: tests/test_counter_normals_host.py builds it with the host compiler and drives every function over
// chosen arguments (the edge words 0 and 2^32 - 1, the quadrant boundaries) that a Philox output reaches once in 2^32 draws.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD static inline
#endif

namespace gs {

// Philox4x32-10 (Salmon et al. 2011): counter (n lo, n hi, t lo, t hi), key (seed lo, seed hi) -- the draws of Gaussian n at
// optimizer step t are a pure function of (seed, t, n): a step the guard skipped draws the same normals when it is replayed.
GS_HD void philox4x32_10(uint64_t n, uint64_t t, uint64_t seed, uint32_t x[4]) {
    uint32_t c0 = (uint32_t)n, c1 = (uint32_t)(n >> 32), c2 = (uint32_t)t, c3 = (uint32_t)(t >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;   // (one 32 x 32 -> 64 multiply each)
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0; c1 = (uint32_t)p1; c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// ln(x) for a normal x in (0, 1) and sin / cos of 0 < a < 2 pi + 1e-9, as fdlibm evaluates them (e_log.c, k_sin.c, k_cos.c: below one
// fp64 ulp) without what the draw never needs -- zero, infinities, NaN, subnormals, and the reduction of a large argument: the
// library's forms compile to 404 fp64 instructions per Gaussian of the draw, these to 160 (the move: 215).
GS_HD double log_unit(double x) {
    int k;
    double m = frexp(x, &k);                                   // m in [0.5, 1)
    if (m < 0.70710678118654752440) { m *= 2.0; k -= 1; }      // m in [sqrt(1/2), sqrt(2))
    const double f = m - 1.0, s = f / (2.0 + f), z = s * s, w = z * z, dk = (double)k;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double hfsq = 0.5 * f * f;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + (t2 + t1)) + dk * 1.90821492927058770002e-10)) - f);
}

GS_HD void sincos_turn(double a, double* sn, double* cs) {
    const double kd = rint(a * 6.36619772367581382433e-01);   // quadrant, 0 .. 4
    double r = fma(-kd, 1.57079632679489655800e+00, a);        // exact: both are multiples of 2^-52 and the difference is below 1
    r = fma(-kd, 6.12323399573676603587e-17, r);               // |r| <= pi / 4
    const double z = r * r;
    const double sp = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double cp = (1.0 - 0.5 * z) + z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const int q = (int)kd;
    const double ss = (q & 1) ? cp : sp, cc = (q & 1) ? sp : cp;
    *sn = (q & 2) ? -ss : ss;
    *cs = ((q + 1) & 2) ? -cc : cc;
}

// The three float32 standard normals of Gaussian n at step t: u_i = (x_i + 0.5) 2^-32 in (0, 1), Box-Muller in fp64 on (u0, u1)
// and (u2, u3), each z rounded to float32 once -- the z that gs_mcmc_noise is documented to take.
GS_HD void normals_of_words(const uint32_t x[4], float z[3]) {
    const double u0 = ((double)x[0] + 0.5) * 0x1p-32, u1 = ((double)x[1] + 0.5) * 0x1p-32;
    const double u2 = ((double)x[2] + 0.5) * 0x1p-32, u3 = ((double)x[3] + 0.5) * 0x1p-32;
    const double two_pi = 6.283185307179586476925286766559;
    const double r01 = sqrt(-2.0 * log_unit(u0)), r23 = sqrt(-2.0 * log_unit(u2));
    double s01, c01, s23, c23;
    sincos_turn(two_pi * u1, &s01, &c01);
    sincos_turn(two_pi * u3, &s23, &c23);
    z[0] = (float)(r01 * c01);
    z[1] = (float)(r01 * s01);
    z[2] = (float)(r23 * c23);
}

GS_HD void counter_normals(uint64_t n, uint64_t t, uint64_t seed, float z[3]) {
    uint32_t x[4];
    philox4x32_10(n, t, seed, x);
    normals_of_words(x, z);
}

}  // namespace gs
