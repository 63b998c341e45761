// normals_san.cpp -- ASan / UBSan leg for csrc/gs_normals.h in its host build (normals.cpp): the exact source the gfx950 kernels
// compile, driven over random Gaussians and frames with exact-size heap buffers.  A stand-alone program, CPU only (sanitizers never
// run on the GPU pool); built and run by tests/test_normals_host.py.  TEST INFRASTRUCTURE ONLY.
#include "normals.cpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double urand() {
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
static double nrand() { return std::sqrt(-2.0 * std::log(urand() + 1e-300)) * std::cos(6.283185307179586 * urand()); }

static double gauss_case(int C, int N) {
    std::vector<float> means(3 * (size_t)N), quats(4 * (size_t)N), scales(3 * (size_t)N), viewmats(16 * (size_t)C, 0.f);
    for (auto& x : means) x = (float)(2.0 * urand() - 1.0);
    for (auto& x : quats) x = (float)(nrand() * std::pow(10.0, 2.0 * urand() - 1.0));
    for (auto& x : scales) x = (float)(nrand() - 3.0);
    for (int c = 0; c < C; ++c) {
        const double a = 0.7 * c;
        float* V = viewmats.data() + 16 * c;
        V[0] = (float)std::cos(a); V[2] = (float)-std::sin(a); V[5] = 1; V[8] = (float)std::sin(a); V[10] = (float)std::cos(a); V[11] = 3.f; V[15] = 1;
    }
    std::vector<float> normals(3 * (size_t)C * N), v_normals(3 * (size_t)C * N), v_quats(4 * (size_t)N);
    for (auto& x : v_normals) x = (float)nrand();
    nm_gauss_fwd(N, C, means.data(), quats.data(), scales.data(), viewmats.data(), normals.data());
    nm_gauss_bwd(N, C, means.data(), quats.data(), scales.data(), viewmats.data(), v_normals.data(), v_quats.data());
    double sum = 0;
    for (float x : normals) sum += std::fabs((double)x);
    for (float x : v_quats) sum += std::fabs((double)x);
    return sum;
}

static double frame_case(int H, int W, bool with_mask, int detach) {
    const size_t n = (size_t)H * W;
    std::vector<float> render4(4 * n), alphas(n), mask(with_mask ? n : 0), dn(3 * n), v_render4(4 * n);
    for (size_t p = 0; p < n; ++p) {
        render4[4 * p] = (float)(0.3 * nrand()); render4[4 * p + 1] = (float)(0.3 * nrand()); render4[4 * p + 2] = (float)(-1.0 + 0.2 * nrand());
        const double r = urand();   // a few depths that are no depth
        render4[4 * p + 3] = r < 0.01 ? 0.f : (r < 0.02 ? NAN : (r < 0.03 ? INFINITY : (r < 0.04 ? -1.f : (float)(2.0 + 0.05 * nrand()))));
        alphas[p] = urand() < 0.05 ? 0.2f : (float)(0.7 + 0.3 * urand());
        if (with_mask) mask[p] = urand() < 0.1 ? 1.f : 0.f;
    }
    const float f = 0.9f * (W > 8 ? W : 8);
    const float K[9] = {f, 0.f, 0.5f * W + 0.3f, 0.f, 1.1f * f, 0.5f * H - 0.2f, 0.f, 0.f, 1.f};
    float rec[2];
    double sums[2];
    nm_loss_fwd(H, W, K, 0.5f, render4.data(), alphas.data(), with_mask ? mask.data() : nullptr, rec, sums, dn.data());
    nm_loss_bwd(H, W, K, 0.5f, detach, render4.data(), alphas.data(), with_mask ? mask.data() : nullptr, rec[1], 0.7f, v_render4.data());
    double sum = rec[0] + sums[1];
    for (float x : dn) sum += std::fabs((double)x);
    for (float x : v_render4) sum += std::fabs((double)x);
    if (!(sum == sum)) { std::fprintf(stderr, "NaN checksum\n"); std::exit(3); }
    return sum;
}

int main() {
    const int gauss[][2] = {{1, 0}, {1, 1}, {2, 65}, {3, 5000}};
    for (const auto& c : gauss) std::printf("gaussians C=%d N=%d -> checksum %.9g\n", c[0], c[1], gauss_case(c[0], c[1]));
    const int frames[][4] = {{1, 1, 0, 0}, {2, 40, 1, 0}, {12, 1, 0, 0}, {3, 3, 0, 0}, {37, 53, 1, 0}, {17, 127, 1, 1}, {270, 480, 0, 0}};
    for (const auto& c : frames) std::printf("frame %dx%d mask=%d detach=%d -> checksum %.9g\n", c[0], c[1], c[2], c[3], frame_case(c[0], c[1], c[2] != 0, c[3]));
    std::puts("sanitizer leg ok");
    return 0;
}
