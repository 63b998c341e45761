// gs_visible_index.h -- whose elements a 16-byte quad holds (gs_adam.hip: adam_step_visible_kernel; DESIGN.md "Updating only what a
// step saw").  A segment of the flat Adam buffers holds n_rows Gaussians of w floats each, back to back, padded to a multiple of 4
// floats: quad q holds the elements [4 q, 4 q + 4), which belong to the Gaussians first..last (one for w = 4, at most two for
// w >= 3, four for w = 1) -- or to nobody, behind element n_rows * w.  Plain C++ that compiles for the device and for the host alike:
// tests/test_visible_adam_index_host.py builds it with the host compiler and holds it to a walk over the elements.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GS_VI_HD __host__ __device__ __forceinline__
#else
#define GS_VI_HD static inline
#endif

namespace gs {

// The Gaussian of element e of quad q, for i = e - 4 q in 0..3: first + quad_row_step(r, i, w) with r the offset of the quad's first
// element inside its Gaussian.  No division for w >= 3 (r + i <= w + 2 < 2 w) nor for w = 1, a shift for w = 2.
GS_VI_HD uint32_t quad_row_step(uint32_t r, uint32_t i, uint32_t w) {
    if (w >= 3) return r + i >= w ? 1u : 0u;
    return w == 1 ? i : (r + i) >> 1;
}

// Quad q of a segment of n_rows Gaussians, w >= 1 floats each, with 4 q < n_rows * w: the first and the last Gaussian that own one of
// its elements and the offset r of element 4 q inside the first; returns whether the quad reaches into the pad (elements at or behind
// n_rows * w, which `last` never counts).  ONE division per quad, in 32 bits wherever the segment's length fits them.
GS_VI_HD bool quad_rows(int64_t q, uint32_t w, int64_t n_rows, int64_t* first, int64_t* last, uint32_t* r) {
    const int64_t len = n_rows * (int64_t)w, e = q << 2;
    int64_t f;
    if (len <= (int64_t)0xffffffffu) f = (int64_t)((uint32_t)e / w);
    else f = e / (int64_t)w;
    const uint32_t off = (uint32_t)(e - f * (int64_t)w);
    const bool pad = e + 4 > len;
    int64_t l = f + (int64_t)quad_row_step(off, 3u, w);
    if (l > n_rows - 1) l = n_rows - 1;
    *first = f; *last = l; *r = off;
    return pad;
}

}  // namespace gs
