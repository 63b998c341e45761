// Host build of csrc/gs_counter_normals.h for tests/test_counter_normals_host.py: the device's own text, driven over chosen arguments.
#include "../../easy_gaussian_splatting_amd/csrc/gs_counter_normals.h"

extern "C" {
void cn_philox(uint64_t n, uint64_t t, uint64_t seed, uint32_t* out) { gs::philox4x32_10(n, t, seed, out); }
double cn_log_unit(double x) { return gs::log_unit(x); }
void cn_sincos_turn(double a, double* sn, double* cs) { gs::sincos_turn(a, sn, cs); }
void cn_normals_of_words(const uint32_t* x, float* z) { gs::normals_of_words(x, z); }
void cn_counter_normals(uint64_t n, uint64_t t, uint64_t seed, float* z) { gs::counter_normals(n, t, seed, z); }
void cn_log_unit_many(int64_t count, const double* x, double* out) { for (int64_t i = 0; i < count; ++i) out[i] = gs::log_unit(x[i]); }
void cn_sincos_turn_many(int64_t count, const double* a, double* sn, double* cs) { for (int64_t i = 0; i < count; ++i) gs::sincos_turn(a[i], sn + i, cs + i); }
void cn_normals_of_words_many(int64_t count, const uint32_t* x, float* z) { for (int64_t i = 0; i < count; ++i) gs::normals_of_words(x + 4 * i, z + 3 * i); }
}
