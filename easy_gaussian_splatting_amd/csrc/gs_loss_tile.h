// gs_loss_tile.h -- what the SSIM stencil kernels of gs_loss.hip (the training loss) and gs_metrics.hip (the evaluation metrics)
// share: the tile geometry, the window taps, the byte-offset loads and the XCD-aware block order.
#pragma once
#include "gs_common.h"

namespace gs {

constexpr int kLT = 32;               // tile edge (outputs)
constexpr int kHalo = 5;
constexpr int kLR = kLT + 2 * kHalo;  // 42 staged rows / cols
constexpr int kLRP = kLR + 1;         // padded row stride of the staged tiles
constexpr int kHP = kLT + 1;          // row stride of the horizontal-pass buffers
static_assert(kLT * (kLT / 4) == 256 && kLR * 6 <= 256 && kLR % 6 == 0, "thread mapping of the staging and the separable passes");
static_assert(kLR % 2 == 0 && kLR * 3 <= 128, "backward staging: two 128-thread halves, one staged row each");
constexpr int64_t kLossMaxPixels = (int64_t)1 << 28;   // 12 bytes per pixel and plane under 2^32
constexpr int kLossMaxWidth = 1 << 20;                 // a row's 12 W bytes under 2^24; the row INDEX is held under 2^24 by the entry points (24-bit multiplies)

// The window as compile-time constants: every tap is a LITERAL operand of its FMA.  From __constant__ memory the taps sat in
// scalar registers, and a VALU instruction with a scalar-register source issues every 4.4 cycles on gfx950 against 3.0 with
// vector-register or literal sources (tools/micro/valu_enc.hip) -- two thirds of these kernels' instructions.
#define GS_WIN_TAPS {1.0283800845e-03f, 7.5987581352e-03f, 3.6000772128e-02f, 1.0936068951e-01f, 2.1300553771e-01f, \
                     2.6601172486e-01f, 2.1300553771e-01f, 1.0936068951e-01f, 3.6000772128e-02f, 7.5987581352e-03f, 1.0283800845e-03f}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// base + 32-bit BYTE offset: with a block-uniform base this is one global_load with a scalar base and a vector offset
__device__ __forceinline__ float ld_off(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

struct F3 { float x, y, z; };   // one pixel of a channel-last image / one pixel's three derivative maps: a 12-byte access
__device__ __forceinline__ F3 ld3_off(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const F3*>(reinterpret_cast<const char*>(base) + byte_off);
}

// Block -> tile.  Consecutive block ids go round-robin over the eight XCDs, each with its own L2: XCD x takes the contiguous
// row-major run of tiles [x * per, (x + 1) * per) -- the halos neighbouring tiles share are met in that L2.
// (Args: a kernel's argument block with the image size in .H and .W.)
template <typename Args>
__device__ __forceinline__ bool loss_tile(const Args& a, int& x0, int& y0) {
    const int ntx = (a.W + kLT - 1) / kLT, nt = ntx * ((a.H + kLT - 1) / kLT), per = (nt + 7) >> 3;
    const int id = blockIdx.x, t = (id & 7) * per + (id >> 3);
    if ((id >> 3) >= per || t >= nt) return false;
    const int ty = t / ntx;
    x0 = (t - ty * ntx) * kLT; y0 = ty * kLT;
    return true;
}

// the separable window's horizontal pass over one staged row: thread = row x 6 output columns, register sliding window
// (42 rows x 6 column groups; the last group starts at column 26 and recomputes two: 252 of the 256 threads work)
constexpr int kHOut = 6, kHWin = kHOut + 10;

inline int loss_tile_count(int height, int width) { return ((width + kLT - 1) / kLT) * ((height + kLT - 1) / kLT); }
inline dim3 loss_grid(int nt) { return dim3((unsigned)(8 * ((nt + 7) / 8))); }   // see loss_tile()

}  // namespace gs
