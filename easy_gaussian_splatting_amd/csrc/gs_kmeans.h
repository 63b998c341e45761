// gs_kmeans.h -- THE definition of the k-means assignment and update (gs_kmeans.hip; DESIGN.md "Exporting a trained model").  For a
// point x[D] and a centroid c[D], every sum one k-ascending chain of fmaf, each product rounded once:
//   dot   = fmaf(x[D-1], c[D-1], ... fmaf(x[1], c[1], fmaf(x[0], c[0], 0)))
//   cn    = fmaf(c[D-1], c[D-1], ... fmaf(c[0], c[0], 0))
//   score = fmaf(-2, dot, cn)                        (|x - c|^2 - |x|^2: the same order over the centroids)
//   label = the smallest index among the centroids of minimal score; a NaN score never wins (none wins: label 0)
//   dist2 = chain_k fmaf(d_k, d_k, acc), d_k = x_k - c_label,k
// The labels are this function of the input whatever tiles the kernel cuts the product into: a zero-padded k adds fmaf(0, 0, acc) =
// acc, and the f32-input MFMA is bit for bit this chain.  Plain C++ that compiles for the device and for the host alike:
// tests/hostmath/kmeans.cpp builds it with the host compiler, tests/test_kmeans_host.py holds it to fp64 and tests/test_gpu_kmeans.py
// holds the kernels to it bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_KM_HD __host__ __device__ __forceinline__
#else
#define GS_KM_HD static inline
#endif

namespace gs {

constexpr int32_t kKmNoLabel = 0x7fffffff;   // the running best before any score has won

GS_KM_HD float kmeans_dot(const float* a, const float* b, int D) {
    float acc = 0.f;
    for (int k = 0; k < D; ++k) acc = fmaf(a[k], b[k], acc);
    return acc;
}
GS_KM_HD float kmeans_norm(const float* c, int D) { return kmeans_dot(c, c, D); }
GS_KM_HD float kmeans_score(float dot, float cn) { return fmaf(-2.f, dot, cn); }

// does (s, i) beat the running best (bs, bi)?  Lexicographic on (score, index); false for a NaN s.  The running best starts at
// (+inf, kKmNoLabel), so a score of +inf still wins over "nothing yet".
GS_KM_HD bool kmeans_better(float s, int32_t i, float bs, int32_t bi) { return s < bs || (s == bs && i < bi); }
GS_KM_HD int32_t kmeans_final_label(int32_t bi) { return bi == kKmNoLabel ? 0 : bi; }

GS_KM_HD float kmeans_dist2(const float* x, const float* c, int D) {
    float acc = 0.f;
    for (int k = 0; k < D; ++k) {
        const float d = x[k] - c[k];
        acc = fmaf(d, d, acc);
    }
    return acc;
}

// the label of one point over K centroids [K][D] with their norms cn[K]
GS_KM_HD int32_t kmeans_label(const float* x, const float* centroids, const float* cn, int64_t K, int D) {
    float bs = INFINITY;
    int32_t bi = kKmNoLabel;
    for (int64_t j = 0; j < K; ++j) {
        const float s = kmeans_score(kmeans_dot(x, centroids + j * D, D), cn[j]);
        if (kmeans_better(s, (int32_t)j, bs, bi)) { bs = s; bi = (int32_t)j; }
    }
    return kmeans_final_label(bi);
}

// the updated coordinate of a cluster: the fp64 sum of its members' coordinates, in ascending point order, over their number
GS_KM_HD float kmeans_mean(double sum, int32_t count) { return (float)(sum / (double)count); }

}  // namespace gs
