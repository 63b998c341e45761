// Host build of csrc/gs_kmeans.h for tests/test_kmeans_host.py and tests/test_gpu_kmeans.py: the device's own text, driven over whole
// arrays -- what gs_kmeans_assign and gs_kmeans_update must return bit for bit.
#include "../../easy_gaussian_splatting_amd/csrc/gs_kmeans.h"

#include <vector>

extern "C" {
// labels[N], dist2[N] of x[N][D] over centroids[K][D]
void km_assign(int64_t N, int64_t K, int D, const float* x, const float* centroids, int32_t* labels, float* dist2) {
    std::vector<float> cn((size_t)K);
    for (int64_t j = 0; j < K; ++j) cn[(size_t)j] = gs::kmeans_norm(centroids + j * D, D);
    for (int64_t i = 0; i < N; ++i) {
        const int32_t l = gs::kmeans_label(x + i * D, centroids, cn.data(), K, D);
        labels[i] = l;
        dist2[i] = gs::kmeans_dist2(x + i * D, centroids + (int64_t)l * D, D);
    }
}
// the update from the labels themselves: a walk over the points in ascending order IS the stable sort's order inside every cluster
void km_update(int64_t N, int64_t K, int D, const float* x, const int32_t* labels, float* centroids, int32_t* counts) {
    std::vector<double> sum((size_t)K * D, 0.0);
    for (int64_t j = 0; j < K; ++j) counts[j] = 0;
    for (int64_t i = 0; i < N; ++i) {
        const int32_t l = labels[i];
        if (l < 0 || l >= K) continue;
        for (int k = 0; k < D; ++k) sum[(size_t)l * D + k] += (double)x[i * D + k];
        ++counts[l];
    }
    for (int64_t j = 0; j < K; ++j)
        if (counts[j] > 0)
            for (int k = 0; k < D; ++k) centroids[j * D + k] = gs::kmeans_mean(sum[(size_t)j * D + k], counts[j]);
}
}
