// Host build of csrc/gs_visible_index.h for tests/test_visible_adam_index_host.py: the device's own text, driven over every quad.
#include "../../easy_gaussian_splatting_amd/csrc/gs_visible_index.h"

extern "C" {
// out[q] = {first, last, r, pad} for every quad q of a segment of n_rows Gaussians of width w
void vi_quad_rows_all(int64_t n_quads, uint32_t w, int64_t n_rows, int64_t* out) {
    for (int64_t q = 0; q < n_quads; ++q) {
        int64_t first, last;
        uint32_t r;
        const bool pad = gs::quad_rows(q, w, n_rows, &first, &last, &r);
        out[4 * q] = first; out[4 * q + 1] = last; out[4 * q + 2] = (int64_t)r; out[4 * q + 3] = pad ? 1 : 0;
    }
}
// out = {first, last, r, pad} of the one quad q
void vi_quad_rows_one(int64_t q, uint32_t w, int64_t n_rows, int64_t* out) {
    int64_t first, last;
    uint32_t r;
    const bool pad = gs::quad_rows(q, w, n_rows, &first, &last, &r);
    out[0] = first; out[1] = last; out[2] = (int64_t)r; out[3] = pad ? 1 : 0;
}
uint32_t vi_quad_row_step(uint32_t r, uint32_t i, uint32_t w) { return gs::quad_row_step(r, i, w); }
}
