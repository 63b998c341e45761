// gs_mcmc.hip -- training under a Gaussian budget: the densification of "3D Gaussian Splatting as Markov Chain Monte Carlo"
// (Kheradmand et al., 2024) on the flat optim.FusedAdam buffers -- relocate dead Gaussians onto live ones drawn in proportion to
// opacity, grow by drawing new rows the same way, perturb the means after every step.  DESIGN.md, "Training to a budget".
//
//   mcmc_weights_kernel      per Gaussian: opacity in fp64, dead flag, integer weight floor(o 2^24) (0 when dead, else >= 1)
//   mcmc_cdf_*_kernel        inclusive prefix sum of the uint32 weights into int64: per-block sums, one block over the block
//                            sums, per-block rescan + base.  Integers: the sum does not depend on the order of the blocks.
//   mcmc_sample_kernel       compaction of the dead indices (dst), and per draw j: t = mulhi64(bits[j], total),
//                            src[j] = min{i : cdf[i] > t} by binary search, counts[src[j]] += 1.  The number of draws is read
//                            on the device (relocate: the dead total of the scan) -- no host read sizes anything.
//   mcmc_values_kernel       every drawn Gaussian: new opacity and scales (fp64), Adam moments of its six rows to zero
//   mcmc_copy_kernel         every draw: the six parameter rows src[j] -> dst[j], moments of the destination to zero
//   mcmc_noise_kernel        means += strength g(o) R diag(s^2) R^T z in fp64, four Gaussians per thread, 16-byte accesses
//   mcmc_normals_kernel      z[n][3] = the float32 normals of (seed, step, Gaussian): one Philox4x32-10 block each, Box-Muller in fp64
//   mcmc_step_inputs_kernel  {strength, step, seed} of the step about to run into a device record (values travel as kernel arguments)
//   mcmc_noise_step_kernel   mcmc_noise_kernel with the normals drawn in the kernel from that record; honours the step guard
//
// Everything that decides (weights, opacities against min_opacity, the new values) is formed in fp64 from the fp32 parameters
// and rounded once at the store, as the projection's covariance chain is.
#include "gs_common.h"
#include "gs_counter_normals.h"

namespace gs {

constexpr int kMcmcThreads = 256;
constexpr int kCdfPer = 8, kCdfChunk = kMcmcThreads * kCdfPer;
constexpr int kMaxRatio = 51;   // the paper's (and gsplat's) n_max: the binomial expansion is cut there

__device__ __forceinline__ double sigmoid64(float l) { return 1.0 / (1.0 + exp(-(double)l)); }

// (a) ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMcmcThreads) void mcmc_weights_kernel(int64_t n, const float* __restrict__ logit, double min_opacity,
                                                                    int grow, uint32_t* __restrict__ w, int32_t* __restrict__ dead) {
    const int64_t i = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x;
    if (i >= n) return;
    const double o = sigmoid64(logit[i]);
    const bool d = !grow && !(o > min_opacity);   // (a NaN opacity is dead: relocation heals it)
    const double f = floor(o * 16777216.0);
    w[i] = d ? 0u : (f >= 1.0 ? (uint32_t)f : 1u);
    dead[i] = d ? 1 : 0;
}

// (b) ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMcmcThreads) void mcmc_cdf_partial_kernel(int64_t n, const uint32_t* __restrict__ w,
                                                                        int64_t* __restrict__ block_sums) {
    __shared__ int64_t red[kMcmcThreads / 64];
    const int64_t first = (int64_t)blockIdx.x * kCdfChunk + (int64_t)threadIdx.x * kCdfPer;
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < kCdfPer; ++k) s += first + k < n ? (int64_t)w[first + k] : 0;
    s = wave_reduce_add(s);
    if (lane_id() == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
#pragma unroll
        for (int i = 0; i < kMcmcThreads / 64; ++i) t += red[i];
        block_sums[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kMcmcThreads) void mcmc_cdf_blocksums_kernel(int64_t nb, int64_t* __restrict__ block_sums) {
    __shared__ int64_t scratch[17];
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += kMcmcThreads) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < nb ? block_sums[i] : 0;
        int64_t total;
        const int64_t ex = block_excl_scan_add(v, scratch, &total);
        if (i < nb) block_sums[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kMcmcThreads) void mcmc_cdf_final_kernel(int64_t n, const uint32_t* __restrict__ w,
                                                                      const int64_t* __restrict__ block_sums, int64_t* __restrict__ cdf) {
    __shared__ int64_t scratch[17];
    const int64_t first = (int64_t)blockIdx.x * kCdfChunk + (int64_t)threadIdx.x * kCdfPer;
    uint32_t v[kCdfPer];
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < kCdfPer; ++k) { v[k] = first + k < n ? w[first + k] : 0u; s += (int64_t)v[k]; }
    int64_t total;
    int64_t run = block_sums[blockIdx.x] + block_excl_scan_add(s, scratch, &total);
#pragma unroll
    for (int k = 0; k < kCdfPer; ++k) {
        run += (int64_t)v[k];
        if (first + k < n) cdf[first + k] = run;
    }
}

// (c) ------------------------------------------------------------------------------------------------------------------------
// Relocate (dead_incl given): the draws are the dead Gaussians, dst = their indices in index order.  Grow (dead_incl null): the
// host-known n_draws_host draws, dst = n + j.  No draws when every weight is zero.
__global__ __launch_bounds__(kMcmcThreads) void mcmc_sample_kernel(int64_t n, int64_t n_slots, const int64_t* __restrict__ cdf,
                                                                   const int64_t* __restrict__ bits, const int32_t* __restrict__ dead,
                                                                   const int32_t* __restrict__ dead_incl, int64_t n_draws_host,
                                                                   int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                                   int32_t* __restrict__ counts, int64_t* __restrict__ n_draws_dev) {
    const int64_t j = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x;
    const int64_t total = cdf[n - 1];
    int64_t nd = dead_incl ? (int64_t)dead_incl[n - 1] : n_draws_host;
    if (total <= 0) nd = 0;
    if (nd > n_slots) nd = n_slots;
    if (j == 0) *n_draws_dev = nd;
    if (dead_incl) {
        if (j < n && dead[j]) {
            const int64_t r = (int64_t)dead_incl[j] - 1;
            if (r >= 0 && r < n_slots) dst[r] = (int32_t)j;
        }
    } else if (j < nd) {
        dst[j] = (int32_t)(n + j);
    }
    if (j >= nd) return;
    const uint64_t t = __umul64hi((uint64_t)bits[j], (uint64_t)total);   // in [0, total)
    int64_t lo = 0, hi = n - 1;   // cdf[n-1] = total > t: the answer exists
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    src[j] = (int32_t)lo;
    atomicAdd(counts + lo, 1);
}

// (d) ------------------------------------------------------------------------------------------------------------------------
// Opacity and scale of a Gaussian that R copies replace (the paper's eq. 9): o' = 1 - (1 - o)^(1/R) and s' = s o / D with
//   D = sum_{i=1..R} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)  =  sum_{k=0..R-1} C(R, k+1) (-1)^k o'^(k+1) / sqrt(k+1)
// (the sum over i of C(i-1, k) is C(R, k+1)): R terms, the coefficient by the row recurrence c <- c (R-1-k) / (k+2), no table.
// o' through log1p / expm1: 1 - (1 - o)^(1/R) as written loses o' to cancellation when o is small.  *ratio = o / D.
__device__ __forceinline__ void relocation(double o, int R, double* o_new, double* ratio) {
    const double on = -expm1(log1p(-o) / (double)R);
    double c = (double)R, pw = on, D = 0.0;
    for (int k = 0; k < R; ++k) {
        const double term = c * pw / sqrt((double)(k + 1));
        D += (k & 1) ? -term : term;
        c = c * (double)(R - 1 - k) / (double)(k + 2);
        pw *= on;
    }
    *o_new = on;
    *ratio = D > 0.0 ? o / D : 1.0;   // (o = 0: nothing to share out, the scales stay)
}

__device__ __forceinline__ int clamp_ratio(int r) { return r < 1 ? 1 : (r > kMaxRatio ? kMaxRatio : r); }

__global__ __launch_bounds__(kMcmcThreads) void mcmc_relocation_values_kernel(int64_t n, const float* __restrict__ opac,
                                                                              const float* __restrict__ scales, const int32_t* __restrict__ ratio,
                                                                              float* __restrict__ new_opac, float* __restrict__ new_scales) {
    const int64_t i = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x;
    if (i >= n) return;
    double on, q;
    relocation((double)opac[i], clamp_ratio(ratio[i]), &on, &q);
    new_opac[i] = (float)on;
#pragma unroll
    for (int a = 0; a < 3; ++a) new_scales[3 * i + a] = (float)((double)scales[3 * i + a] * q);
}

struct McmcApplyArgs {
    int64_t n, n_rows, max_draws;
    float *p, *m, *v;
    int64_t off[6];
    int width[6];
    int row_floats;
    double min_opacity;
    const int32_t *src, *dst, *counts;
    const int64_t* n_draws;
};

// tensor order of param_names: 0 means, 1 log_scales, 2 quats, 3 sh_0, 4 sh_rest, 5 logit_opacities
__global__ __launch_bounds__(kMcmcThreads) void mcmc_values_kernel(const McmcApplyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x;
    if (i >= a.n) return;
    const int c = a.counts[i];
    if (c <= 0) return;
    float* lo = a.p + a.off[5] + i;
    float* ls = a.p + a.off[1] + 3 * i;
    const double o = sigmoid64(*lo);
    double on, q;
    relocation(o, clamp_ratio(c + 1), &on, &q);
#pragma unroll
    for (int k = 0; k < 3; ++k) ls[k] = (float)log(exp((double)ls[k]) * q);
    on = fmin(fmax(on, a.min_opacity), 1.0 - 0x1p-23);
    *lo = (float)log(on / (1.0 - on));
    for (int t = 0; t < 6; ++t) {
        const int w = a.width[t];
        const int64_t base = a.off[t] + i * w;
        for (int k = 0; k < w; ++k) { a.m[base + k] = 0.f; a.v[base + k] = 0.f; }
    }
}

__global__ __launch_bounds__(kMcmcThreads) void mcmc_copy_kernel(const McmcApplyArgs a) {
    int64_t nd = *a.n_draws;
    if (nd > a.max_draws) nd = a.max_draws;
    const int W = a.row_floats;
    const int64_t total = nd * W;
    for (int64_t idx = (int64_t)blockIdx.x * kMcmcThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kMcmcThreads) {
        const int64_t j = idx / W;
        const int c = (int)(idx - j * W);
        const int64_t s = a.src[j], d = a.dst[j];
        if (s < 0 || s >= a.n || d < 0 || d >= a.n_rows) continue;
        int t, col;
        if (c < 3) { t = 0; col = c; }
        else if (c < 6) { t = 1; col = c - 3; }
        else if (c < 10) { t = 2; col = c - 6; }
        else if (c < 13) { t = 3; col = c - 10; }
        else if (c < W - 1) { t = 4; col = c - 13; }
        else { t = 5; col = 0; }
        const int w = a.width[t];
        const int64_t from = a.off[t] + s * w + col, to = a.off[t] + d * w + col;
        a.p[to] = a.p[from];
        a.m[to] = 0.f;
        a.v[to] = 0.f;
    }
}

// (e) ------------------------------------------------------------------------------------------------------------------------
// One Gaussian's move: mu += strength g(o) R diag(s^2) R^T z in fp64, one rounding per component (both noise kernels call this).
__device__ __forceinline__ void noise_move(const float* __restrict__ q, const float* __restrict__ ls, float lg, const float* __restrict__ z,
                                           double strength, float* __restrict__ mu) {
    double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double inv = 1.0 / fmax(sqrt(qw * qw + qx * qx + qy * qy + qz * qz), 1e-12);
    qw *= inv; qx *= inv; qy *= inv; qz *= inv;
    const double r00 = 1.0 - 2.0 * (qy * qy + qz * qz), r01 = 2.0 * (qx * qy - qw * qz), r02 = 2.0 * (qx * qz + qw * qy);
    const double r10 = 2.0 * (qx * qy + qw * qz), r11 = 1.0 - 2.0 * (qx * qx + qz * qz), r12 = 2.0 * (qy * qz - qw * qx);
    const double r20 = 2.0 * (qx * qz - qw * qy), r21 = 2.0 * (qy * qz + qw * qx), r22 = 1.0 - 2.0 * (qx * qx + qy * qy);
    const double z0 = z[0], z1 = z[1], z2 = z[2];
    const double s0 = exp((double)ls[0]), s1 = exp((double)ls[1]), s2 = exp((double)ls[2]);
    // R diag(s^2) R^T z
    const double y0 = s0 * s0 * (r00 * z0 + r10 * z1 + r20 * z2);
    const double y1 = s1 * s1 * (r01 * z0 + r11 * z1 + r21 * z2);
    const double y2 = s2 * s2 * (r02 * z0 + r12 * z1 + r22 * z2);
    const double o = sigmoid64(lg);
    const double gate = strength / (1.0 + exp(-100.0 * ((1.0 - o) - 0.995)));
    mu[0] = (float)((double)mu[0] + gate * (r00 * y0 + r01 * y1 + r02 * y2));
    mu[1] = (float)((double)mu[1] + gate * (r10 * y0 + r11 * y1 + r12 * y2));
    mu[2] = (float)((double)mu[2] + gate * (r20 * y0 + r21 * y1 + r22 * y2));
}

// Four Gaussians per thread: their means, log-scales and normals are three float4 each, their quaternions four, their logits
// one.  Every pointer is 16-byte aligned (the flat buffers' segments are; the entry refuses anything else); the last, ragged
// group goes element by element.
__global__ __launch_bounds__(kMcmcThreads) void mcmc_noise_kernel(int64_t n, double strength, const float* __restrict__ log_scales,
                                                                  const float* __restrict__ quats, const float* __restrict__ logit,
                                                                  const float* __restrict__ z, float* means) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * kMcmcThreads + threadIdx.x);
    if (i0 >= n) return;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    float mu[12], ls[12], zz[12], qq[16], lg[4];
    const bool vec = cnt == 4;
    if (vec) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 a = reinterpret_cast<const float4*>(means + 3 * i0)[k];
            const float4 b = reinterpret_cast<const float4*>(log_scales + 3 * i0)[k];
            const float4 c = reinterpret_cast<const float4*>(z + 3 * i0)[k];
            mu[4 * k] = a.x; mu[4 * k + 1] = a.y; mu[4 * k + 2] = a.z; mu[4 * k + 3] = a.w;
            ls[4 * k] = b.x; ls[4 * k + 1] = b.y; ls[4 * k + 2] = b.z; ls[4 * k + 3] = b.w;
            zz[4 * k] = c.x; zz[4 * k + 1] = c.y; zz[4 * k + 2] = c.z; zz[4 * k + 3] = c.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 a = reinterpret_cast<const float4*>(quats + 4 * i0)[k];
            qq[4 * k] = a.x; qq[4 * k + 1] = a.y; qq[4 * k + 2] = a.z; qq[4 * k + 3] = a.w;
        }
        const float4 a = *reinterpret_cast<const float4*>(logit + i0);
        lg[0] = a.x; lg[1] = a.y; lg[2] = a.z; lg[3] = a.w;
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bool in = g < cnt;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mu[3 * g + k] = in ? means[3 * (i0 + g) + k] : 0.f;
                ls[3 * g + k] = in ? log_scales[3 * (i0 + g) + k] : 0.f;
                zz[3 * g + k] = in ? z[3 * (i0 + g) + k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) qq[4 * g + k] = in ? quats[4 * (i0 + g) + k] : (k == 0 ? 1.f : 0.f);
            lg[g] = in ? logit[i0 + g] : 0.f;
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) noise_move(qq + 4 * g, ls + 3 * g, lg[g], zz + 3 * g, strength, mu + 3 * g);
    if (vec) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<float4*>(means + 3 * i0)[k] = make_float4(mu[4 * k], mu[4 * k + 1], mu[4 * k + 2], mu[4 * k + 3]);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g < cnt) {
#pragma unroll
                for (int k = 0; k < 3; ++k) means[3 * (i0 + g) + k] = mu[3 * g + k];
            }
        }
    }
}

// (f) ------------------------------------------------------------------------------------------------------------------------
// Same four Gaussians per thread as mcmc_noise_kernel, for the store of the normals: three float4 per full group.
__global__ __launch_bounds__(kMcmcThreads) void mcmc_normals_kernel(int64_t n, uint64_t step, uint64_t seed, float* __restrict__ z) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * kMcmcThreads + threadIdx.x);
    if (i0 >= n) return;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    float zz[12];
#pragma unroll
    for (int g = 0; g < 4; ++g) counter_normals((uint64_t)(i0 + g), step, seed, zz + 3 * g);
    if (cnt == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<float4*>(z + 3 * i0)[k] = make_float4(zz[4 * k], zz[4 * k + 1], zz[4 * k + 2], zz[4 * k + 3]);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g < cnt) {
#pragma unroll
                for (int k = 0; k < 3; ++k) z[3 * (i0 + g) + k] = zz[3 * g + k];
            }
        }
    }
}

// The record gs_mcmc_noise_step reads: GS_MCMC_REC_WORDS int64 = {strength (the bits of a double), step, seed, 0}.
struct McmcStepRec { int64_t w[GS_MCMC_REC_WORDS]; };
__global__ void mcmc_step_inputs_kernel(const McmcStepRec r, int64_t* __restrict__ rec) {
    if (threadIdx.x < (unsigned)GS_MCMC_REC_WORDS) rec[threadIdx.x] = r.w[threadIdx.x];
}

// mcmc_noise_kernel without the z array: every thread draws its four Gaussians' normals (counter_normals) from the record's
// {step, seed} and applies the record's strength -- 12 bytes per Gaussian less than randn + mcmc_noise_kernel, and no launch
// between them.  Under the step guard a skipped step moves nothing.
__global__ __launch_bounds__(kMcmcThreads) void mcmc_noise_step_kernel(int64_t n, const int64_t* __restrict__ rec, const int64_t* guard,
                                                                       const float* __restrict__ log_scales, const float* __restrict__ quats,
                                                                       const float* __restrict__ logit, float* means) {
    if (guard_tripped(guard)) return;
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * kMcmcThreads + threadIdx.x);
    if (i0 >= n) return;
    const double strength = __longlong_as_double(rec[0]);
    const uint64_t step = (uint64_t)rec[1], seed = (uint64_t)rec[2];
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    float mu[12], ls[12], qq[16], lg[4];
    const bool vec = cnt == 4;
    if (vec) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 a = reinterpret_cast<const float4*>(means + 3 * i0)[k];
            const float4 b = reinterpret_cast<const float4*>(log_scales + 3 * i0)[k];
            mu[4 * k] = a.x; mu[4 * k + 1] = a.y; mu[4 * k + 2] = a.z; mu[4 * k + 3] = a.w;
            ls[4 * k] = b.x; ls[4 * k + 1] = b.y; ls[4 * k + 2] = b.z; ls[4 * k + 3] = b.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 a = reinterpret_cast<const float4*>(quats + 4 * i0)[k];
            qq[4 * k] = a.x; qq[4 * k + 1] = a.y; qq[4 * k + 2] = a.z; qq[4 * k + 3] = a.w;
        }
        const float4 a = *reinterpret_cast<const float4*>(logit + i0);
        lg[0] = a.x; lg[1] = a.y; lg[2] = a.z; lg[3] = a.w;
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bool in = g < cnt;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mu[3 * g + k] = in ? means[3 * (i0 + g) + k] : 0.f;
                ls[3 * g + k] = in ? log_scales[3 * (i0 + g) + k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) qq[4 * g + k] = in ? quats[4 * (i0 + g) + k] : (k == 0 ? 1.f : 0.f);
            lg[g] = in ? logit[i0 + g] : 0.f;
        }
    }
    // (one Gaussian at a time: its normals live only until its move -- the kernel stays out of scratch)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float z[3];
        counter_normals((uint64_t)(i0 + g), step, seed, z);
        noise_move(qq + 4 * g, ls + 3 * g, lg[g], z, strength, mu + 3 * g);
    }
    if (vec) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<float4*>(means + 3 * i0)[k] = make_float4(mu[4 * k], mu[4 * k + 1], mu[4 * k + 2], mu[4 * k + 3]);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g < cnt) {
#pragma unroll
                for (int k = 0; k < 3; ++k) means[3 * (i0 + g) + k] = mu[3 * g + k];
            }
        }
    }
}

}  // namespace gs

using namespace gs;

static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kMcmcThreads - 1) / kMcmcThreads); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int gs_mcmc_weights(void* stream, int64_t n, const float* logit_opacities, double min_opacity, int grow, uint32_t* weights,
                               int32_t* dead) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31), "0 <= n < 2^31");
    GS_REQUIRE(min_opacity >= 0.0 && min_opacity < 1.0, "0 <= min_opacity < 1");
    GS_REQUIRE(grow == 0 || grow == 1, "grow is 0 or 1");
    if (n == 0) return GS_OK;
    GS_REQUIRE(logit_opacities && weights && dead, "null pointer");
    hipLaunchKernelGGL(mcmc_weights_kernel, dim3(blocks_for(n)), dim3(kMcmcThreads), 0, (hipStream_t)stream, n, logit_opacities, min_opacity,
                       grow, weights, dead);
    GS_LAUNCH_CHECK("mcmc_weights_kernel");
    return GS_OK;
}

extern "C" size_t gs_mcmc_cdf_workspace_longs(int64_t n) {
    return n <= 0 ? 1 : (size_t)((n + kCdfChunk - 1) / kCdfChunk) + 1;
}

extern "C" int gs_mcmc_cdf(void* stream, int64_t n, const uint32_t* weights, int64_t* cdf, int64_t* workspace) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31), "0 <= n < 2^31");
    if (n == 0) return GS_OK;
    GS_REQUIRE(weights && cdf && workspace, "null pointer");
    const int64_t nb = (n + kCdfChunk - 1) / kCdfChunk;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mcmc_cdf_partial_kernel, dim3((unsigned)nb), dim3(kMcmcThreads), 0, st, n, weights, workspace);
    GS_LAUNCH_CHECK("mcmc_cdf_partial_kernel");
    hipLaunchKernelGGL(mcmc_cdf_blocksums_kernel, dim3(1), dim3(kMcmcThreads), 0, st, nb, workspace);
    GS_LAUNCH_CHECK("mcmc_cdf_blocksums_kernel");
    hipLaunchKernelGGL(mcmc_cdf_final_kernel, dim3((unsigned)nb), dim3(kMcmcThreads), 0, st, n, weights, (const int64_t*)workspace, cdf);
    GS_LAUNCH_CHECK("mcmc_cdf_final_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_sample(void* stream, int64_t n, int64_t n_slots, const int64_t* cdf, const int64_t* bits, const int32_t* dead,
                              const int32_t* dead_incl, int64_t n_draws_host, int32_t* src, int32_t* dst, int32_t* counts,
                              int64_t* n_draws_dev) {
    GS_REQUIRE(n >= 0 && n_slots >= 0 && n + n_slots < (1ll << 31), "n >= 0, n_slots >= 0, n + n_slots < 2^31");
    GS_REQUIRE((dead == nullptr) == (dead_incl == nullptr), "dead and dead_incl go together");
    GS_REQUIRE(dead_incl ? n_slots == n : (n_draws_host >= 0 && n_draws_host <= n_slots),
               "relocate: n_slots == n; grow: 0 <= n_draws_host <= n_slots");
    GS_REQUIRE(n_draws_dev != nullptr, "null n_draws_dev");
    GS_REQUIRE(n == 0 || (cdf && counts), "null pointer");
    GS_REQUIRE(n_slots == 0 || (bits && src && dst), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    GS_HIP_CHECK(hipMemsetAsync(n_draws_dev, 0, sizeof(int64_t), st));
    if (n == 0) return GS_OK;
    GS_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st));
    if (n_slots == 0) return GS_OK;
    GS_HIP_CHECK(hipMemsetAsync(src, 0xff, (size_t)n_slots * sizeof(int32_t), st));
    GS_HIP_CHECK(hipMemsetAsync(dst, 0xff, (size_t)n_slots * sizeof(int32_t), st));
    hipLaunchKernelGGL(mcmc_sample_kernel, dim3(blocks_for(n_slots)), dim3(kMcmcThreads), 0, st, n, n_slots, cdf, bits, dead, dead_incl,
                       n_draws_host, src, dst, counts, n_draws_dev);
    GS_LAUNCH_CHECK("mcmc_sample_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_relocation_values(void* stream, int64_t n, const float* opacities, const float* scales, const int32_t* ratio,
                                         float* new_opacities, float* new_scales) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31), "0 <= n < 2^31");
    if (n == 0) return GS_OK;
    GS_REQUIRE(opacities && scales && ratio && new_opacities && new_scales, "null pointer");
    hipLaunchKernelGGL(mcmc_relocation_values_kernel, dim3(blocks_for(n)), dim3(kMcmcThreads), 0, (hipStream_t)stream, n, opacities, scales,
                       ratio, new_opacities, new_scales);
    GS_LAUNCH_CHECK("mcmc_relocation_values_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_apply(void* stream, int64_t n, int64_t n_rows, int K, double min_opacity, const int32_t* src, const int32_t* dst,
                             const int32_t* counts, const int64_t* n_draws_dev, int64_t max_draws, float* params, float* exp_avg,
                             float* exp_avg_sq, const int64_t* offsets_host) {
    GS_REQUIRE(n >= 0 && n_rows >= n && n_rows < (1ll << 31), "0 <= n <= n_rows < 2^31");
    GS_REQUIRE(K >= 1 && K <= 25, "1 <= K <= 25");
    GS_REQUIRE(min_opacity >= 0.0 && min_opacity < 1.0, "0 <= min_opacity < 1");
    GS_REQUIRE(max_draws >= 0 && max_draws <= n_rows, "0 <= max_draws <= n_rows");
    if (n == 0) return GS_OK;
    GS_REQUIRE(counts && n_draws_dev && params && exp_avg && exp_avg_sq && offsets_host, "null pointer");
    GS_REQUIRE(max_draws == 0 || (src && dst), "null pointer");
    McmcApplyArgs a;
    a.n = n; a.n_rows = n_rows; a.max_draws = max_draws;
    a.p = params; a.m = exp_avg; a.v = exp_avg_sq;
    const int widths[6] = {3, 3, 4, 3, 3 * (K - 1), 1};
    a.row_floats = 0;
    for (int t = 0; t < 6; ++t) {
        GS_REQUIRE(offsets_host[t] >= 0, "negative offset");
        a.off[t] = offsets_host[t]; a.width[t] = widths[t]; a.row_floats += widths[t];
    }
    a.min_opacity = min_opacity;
    a.src = src; a.dst = dst; a.counts = counts; a.n_draws = n_draws_dev;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mcmc_values_kernel, dim3(blocks_for(n)), dim3(kMcmcThreads), 0, st, a);   // values before copies
    GS_LAUNCH_CHECK("mcmc_values_kernel");
    if (max_draws == 0) return GS_OK;
    const int64_t want = (max_draws * a.row_floats + kMcmcThreads - 1) / kMcmcThreads;
    hipLaunchKernelGGL(mcmc_copy_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(kMcmcThreads), 0, st, a);
    GS_LAUNCH_CHECK("mcmc_copy_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_noise(void* stream, int64_t n, double strength, const float* log_scales, const float* quats,
                             const float* logit_opacities, const float* z, float* means) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31), "0 <= n < 2^31");
    GS_REQUIRE(strength == strength, "strength is NaN");
    if (n == 0) return GS_OK;
    GS_REQUIRE(log_scales && quats && logit_opacities && z && means, "null pointer");
    GS_REQUIRE(aligned16(log_scales) && aligned16(quats) && aligned16(logit_opacities) && aligned16(z) && aligned16(means),
               "pointers must be 16-byte aligned");
    const unsigned nb = blocks_for((n + 3) / 4);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3(nb), dim3(kMcmcThreads), 0, st, n, strength, log_scales, quats, logit_opacities, z, means);
    GS_LAUNCH_CHECK("mcmc_noise_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_normals(void* stream, int64_t n, int64_t step, uint64_t seed, float* z_out) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31), "0 <= n < 2^31");
    GS_REQUIRE(step >= 0, "step >= 0");
    if (n == 0) return GS_OK;
    GS_REQUIRE(z_out != nullptr && aligned16(z_out), "z_out: non-null, 16-byte aligned");
    hipLaunchKernelGGL(mcmc_normals_kernel, dim3(blocks_for((n + 3) / 4)), dim3(kMcmcThreads), 0, (hipStream_t)stream, n, (uint64_t)step, seed,
                       z_out);
    GS_LAUNCH_CHECK("mcmc_normals_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_step_inputs(void* stream, double strength, int64_t step, uint64_t seed, int64_t* rec_dev) {
    GS_REQUIRE(strength == strength, "strength is NaN");
    GS_REQUIRE(step >= 0, "step >= 0");
    GS_REQUIRE(rec_dev != nullptr && aligned16(rec_dev), "rec_dev: non-null, 16-byte aligned");
    McmcStepRec r;
    memcpy(&r.w[0], &strength, sizeof(double));
    r.w[1] = step; r.w[2] = (int64_t)seed; r.w[3] = 0;
    // values travel as kernel arguments (copied at launch): no host buffer that a later call could overwrite
    hipLaunchKernelGGL(mcmc_step_inputs_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, r, rec_dev);
    GS_LAUNCH_CHECK("mcmc_step_inputs_kernel");
    return GS_OK;
}

extern "C" int gs_mcmc_noise_step(void* stream, int64_t n, const int64_t* rec_dev, const float* log_scales, const float* quats,
                                  const float* logit_opacities, float* means) {
    GS_REQUIRE(n >= 0 && n < (1ll << 31), "0 <= n < 2^31");
    if (n == 0) return GS_OK;
    GS_REQUIRE(rec_dev && log_scales && quats && logit_opacities && means, "null pointer");
    GS_REQUIRE(aligned16(rec_dev) && aligned16(log_scales) && aligned16(quats) && aligned16(logit_opacities) && aligned16(means),
               "pointers must be 16-byte aligned");
    hipLaunchKernelGGL(mcmc_noise_step_kernel, dim3(blocks_for((n + 3) / 4)), dim3(kMcmcThreads), 0, (hipStream_t)stream, n, rec_dev,
                       current_guard().info, log_scales, quats, logit_opacities, means);
    GS_LAUNCH_CHECK("mcmc_noise_step_kernel");
    return GS_OK;
}
