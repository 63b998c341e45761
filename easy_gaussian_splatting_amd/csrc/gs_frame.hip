// gs_frame.hip -- what stands between a render and a frame on a viewer's screen or in a video file, for gfx950 (DESIGN.md
// section 16).  The reference does it on the host, per frame: `torch.clamp`, a float32 read-back, `adjust_image_aspect`'s copy into
// a zero-padded array (viewer/viewer_runtime.py:104-116) and, for a video, `floor(image * 255).astype(uint8)`
// (viewer/utils.py:118-135).  Here it is one streaming pass over the render, so what crosses the bus is the finished frame.
//
//   frame_finish_kernel : thread = FOUR consecutive pixels of the FLAT output [out_H * out_W] (12 output elements: three aligned
//                         16-byte stores of floats, or one aligned 12-byte store of packed RGB bytes -- rows of 3 out_W bytes are in
//                         general not dword aligned, the flat array is).  Where the four pixels lie side by side inside the render
//                         they are read as whole vectors (three float4 of a three-channel render when the pixel index is a multiple
//                         of four, else four 12-byte pixels; a float4 per four-channel pixel); a group that crosses a row end or
//                         touches the padding walks its pixels one by one.  The 0-3 pixels behind the last full group go to one
//                         more thread, with element stores.  Every output element is written: nothing clears the buffer first.
//   frame_range_kernel  : {min, max} of the depth channel over the covered pixels per block (fminf / fmaxf skip a NaN depth),
//   frame_range_reduce  : one block over the per-block pairs; {0, 0} when nothing is covered.  Min and max are exact in any order
//                         and there are no atomics: the same inputs give the same bits.
// Neither looks at the step guard or at a workspace of the rasterizer.
#include "gs_common.h"

namespace gs {

struct FrameArgs {
    int H, W, oW;            // the render's size; the output's row length (>= W)
    unsigned groups, tail;   // full four-pixel groups of the flat output, pixels behind them (0..3)
    const float* src;        // [H,W,CIN]
    const float* alpha;      // [H,W]  depth mode
    const float* range;      // {lo, hi}  depth mode
    float alpha_min;
    void* out;               // [out_H,out_W,3] float or uint8_t
};

// clamp(x, 0, 1).  F32: torch.clamp's values -- a NaN stays a NaN, -0 becomes +0.  U8: a NaN becomes 0 (it has no code).
template <int FMT>
__device__ __forceinline__ float frame_clamp(float x) {
    if (FMT == GS_FRAME_F32) return x > 0.f ? fminf(x, 1.f) : (x != x ? x : 0.f);
    return x > 0.f ? fminf(x, 1.f) : 0.f;
}
// the code of a clamped value: ONE rounded float32 product, then floor (the value is >= 0: the conversion truncates)
__device__ __forceinline__ unsigned frame_code(float c) { return (unsigned)(c * 255.f); }

// depth -> grey: near is bright.  t keeps a NaN depth a NaN (the format decides what becomes of it); an uncovered pixel is 0.
__device__ __forceinline__ float frame_grey(float d, float al, float alpha_min, float lo, float hi) {
    if (!(al >= alpha_min)) return 0.f;
    const float t = hi == lo ? 0.f : (d - lo) / (hi - lo);
    return 1.f - frame_clamp<GS_FRAME_F32>(t);
}

struct FramePx { float x, y, z; };   // one pixel of a three-channel render: a 12-byte access

// output values of source pixel s (any s inside the render)
template <int MODE, int CIN>
__device__ __forceinline__ void frame_load1(const FrameArgs& a, unsigned s, float lo, float hi, float v[3]) {
    if (MODE == GS_FRAME_RGB) {
        if (CIN == 3) { const FramePx p = reinterpret_cast<const FramePx*>(a.src)[s]; v[0] = p.x; v[1] = p.y; v[2] = p.z; }
        else { const float4 p = reinterpret_cast<const float4*>(a.src)[s]; v[0] = p.x; v[1] = p.y; v[2] = p.z; }
    } else {
        v[0] = v[1] = v[2] = frame_grey(a.src[(unsigned)CIN * s + (unsigned)(CIN - 1)], a.alpha[s], a.alpha_min, lo, hi);
    }
}

// the same for source pixels s .. s + 3 of one row
template <int MODE, int CIN>
__device__ __forceinline__ void frame_load4(const FrameArgs& a, unsigned s, float lo, float hi, float v[4][3]) {
    const bool al4 = (s & 3u) == 0;   // 16-byte aligned in a three- and in a one-channel image
    if (MODE == GS_FRAME_RGB && CIN == 3) {
        if (al4) {
            const float4* p = reinterpret_cast<const float4*>(a.src + 3u * s);
            const float4 q0 = p[0], q1 = p[1], q2 = p[2];
            v[0][0] = q0.x; v[0][1] = q0.y; v[0][2] = q0.z; v[1][0] = q0.w; v[1][1] = q1.x; v[1][2] = q1.y;
            v[2][0] = q1.z; v[2][1] = q1.w; v[2][2] = q2.x; v[3][0] = q2.y; v[3][1] = q2.z; v[3][2] = q2.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) frame_load1<MODE, CIN>(a, s + k, lo, hi, v[k]);
        }
    } else if (MODE == GS_FRAME_RGB) {
#pragma unroll
        for (int k = 0; k < 4; ++k) frame_load1<MODE, CIN>(a, s + k, lo, hi, v[k]);
    } else {
        float d[4], al[4];
        if (al4) {
            const float4 q = *reinterpret_cast<const float4*>(a.alpha + s);
            al[0] = q.x; al[1] = q.y; al[2] = q.z; al[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) al[k] = a.alpha[s + k];
        }
        if (CIN == 1 && al4) {
            const float4 q = *reinterpret_cast<const float4*>(a.src + s);
            d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = a.src[(unsigned)CIN * (s + k) + (unsigned)(CIN - 1)];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = frame_grey(d[k], al[k], a.alpha_min, lo, hi);
    }
}

template <int FMT, int MODE, int CIN>
__global__ __launch_bounds__(256) void frame_finish_kernel(const FrameArgs a) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.groups || (g == a.groups && a.tail == 0)) return;
    float lo = 0.f, hi = 0.f;
    if (MODE == GS_FRAME_DEPTH) { lo = a.range[0]; hi = a.range[1]; }
    const unsigned np = g == a.groups ? a.tail : 4u;   // pixels of this thread
    const unsigned p0 = 4u * g, y = p0 / (unsigned)a.oW, x = p0 - y * (unsigned)a.oW;
    float v[4][3];
    if (np == 4u && y < (unsigned)a.H && x + 3u < (unsigned)a.W) {
        frame_load4<MODE, CIN>(a, y * (unsigned)a.W + x, lo, hi, v);
    } else {
        unsigned yy = y, xx = x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k][0] = v[k][1] = v[k][2] = 0.f;
            if ((unsigned)k < np && yy < (unsigned)a.H && xx < (unsigned)a.W)
                frame_load1<MODE, CIN>(a, yy * (unsigned)a.W + xx, lo, hi, v[k]);
            if (++xx == (unsigned)a.oW) { xx = 0; ++yy; }
        }
    }
    float c[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * k + j] = frame_clamp<FMT>(v[k][j]);
    if (FMT == GS_FRAME_F32) {
        float* o = reinterpret_cast<float*>(a.out) + 12u * g;
        if (np == 4u) {
            float4* o4 = reinterpret_cast<float4*>(o);
            o4[0] = make_float4(c[0], c[1], c[2], c[3]);
            o4[1] = make_float4(c[4], c[5], c[6], c[7]);
            o4[2] = make_float4(c[8], c[9], c[10], c[11]);
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i)
                if ((unsigned)i < 3u * np) o[i] = c[i];
        }
    } else {
        unsigned b[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) b[i] = frame_code(c[i]);
        uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + 12u * g;
        if (np == 4u) {
            uint3 w;
            w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            *reinterpret_cast<uint3*>(o) = w;
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i)
                if ((unsigned)i < 3u * np) o[i] = (uint8_t)b[i];
        }
    }
}

constexpr int kRangeMaxBlocks = 1024;

struct RangeArgs {
    unsigned P;           // pixels
    const float* src;     // [H,W,CIN], depth in channel CIN - 1
    const float* alpha;   // [H,W]
    float alpha_min;
    float* partial;       // [blocks][2]
};

__device__ __forceinline__ void range_block_store(float lo, float hi, float* dst) {
    __shared__ float red[2][4];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { lo = fminf(lo, __shfl_xor(lo, d, 64)); hi = fmaxf(hi, __shfl_xor(hi, d, 64)); }
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        dst[0] = lo; dst[1] = hi;
    }
}

template <int CIN>
__global__ __launch_bounds__(256) void frame_range_kernel(const RangeArgs a) {
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
    const unsigned ngroups = (a.P + 3u) >> 2;
    for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < ngroups; g += gridDim.x * 256u) {
        const unsigned p = 4u * g;
        float d[4], al[4];
        if (p + 3u < a.P) {
            const float4 q = reinterpret_cast<const float4*>(a.alpha)[g];
            al[0] = q.x; al[1] = q.y; al[2] = q.z; al[3] = q.w;
            if (CIN == 1) {
                const float4 r = reinterpret_cast<const float4*>(a.src)[g];
                d[0] = r.x; d[1] = r.y; d[2] = r.z; d[3] = r.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = a.src[(unsigned)CIN * (p + k) + (unsigned)(CIN - 1)];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = p + k < a.P;
                al[k] = in ? a.alpha[p + k] : __builtin_nanf("");   // (a NaN is never covered, whatever alpha_min is)
                d[k] = in ? a.src[(unsigned)CIN * (p + k) + (unsigned)(CIN - 1)] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (al[k] >= a.alpha_min) { lo = fminf(lo, d[k]); hi = fmaxf(hi, d[k]); }
    }
    range_block_store(lo, hi, a.partial + 2 * blockIdx.x);
}

__global__ __launch_bounds__(256) void frame_range_reduce(int nblocks, const float* __restrict__ partial, float* __restrict__ out) {
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
    for (int i = threadIdx.x; i < nblocks; i += 256) { lo = fminf(lo, partial[2 * i]); hi = fmaxf(hi, partial[2 * i + 1]); }
    __shared__ float res[2];
    range_block_store(lo, hi, res);
    if (threadIdx.x == 0) {
        const bool any = res[0] <= res[1];   // (nothing covered, or NaN depths alone: +inf > -inf)
        out[0] = any ? res[0] : 0.f; out[1] = any ? res[1] : 0.f;
    }
}

static int range_blocks(int height, int width) {
    const int64_t groups = ((int64_t)height * width + 3) / 4, blocks = (groups + 255) / 256;
    return (int)(blocks < kRangeMaxBlocks ? blocks : kRangeMaxBlocks);
}

constexpr int64_t kFrameMaxBytes = 0x7fffffff;   // every byte offset is a 32-bit unsigned product of in-range factors

template <int FMT>
static void frame_launch(int mode, int cin, unsigned blocks, hipStream_t st, const FrameArgs& a) {
    if (mode == GS_FRAME_RGB) {
        if (cin == 3) hipLaunchKernelGGL((frame_finish_kernel<FMT, GS_FRAME_RGB, 3>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((frame_finish_kernel<FMT, GS_FRAME_RGB, 4>), dim3(blocks), dim3(256), 0, st, a);
    } else {
        if (cin == 1) hipLaunchKernelGGL((frame_finish_kernel<FMT, GS_FRAME_DEPTH, 1>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((frame_finish_kernel<FMT, GS_FRAME_DEPTH, 4>), dim3(blocks), dim3(256), 0, st, a);
    }
}

}  // namespace gs

using namespace gs;

// one {min, max} pair per launched block
extern "C" size_t gs_frame_workspace_floats(int height, int width) {
    if (height <= 0 || width <= 0) return 0;
    return 2 * (size_t)range_blocks(height, width);
}

extern "C" int gs_frame_range(void* stream, int height, int width, int cin, const float* render, const float* alpha,
                              float alpha_min, float* workspace, float* range2) {
    GS_REQUIRE(height > 0 && width > 0, "the image size must be positive");
    GS_REQUIRE(cin == 1 || cin == 4, "the depth is channel cin - 1 of a four-channel render or a one-channel depth image: cin is 1 or 4");
    GS_REQUIRE((int64_t)height * width * cin * 4 <= kFrameMaxBytes, "image too large for the frame kernels' 32-bit byte offsets (H * W * cin * 4 < 2^31)");
    GS_REQUIRE(render && alpha && workspace && range2, "null pointer");
    GS_REQUIRE((((uintptr_t)render | (uintptr_t)alpha) & 15) == 0, "render and alpha must be 16-byte aligned");
    RangeArgs a;
    a.P = (unsigned)(height * width); a.src = render; a.alpha = alpha; a.alpha_min = alpha_min; a.partial = workspace;
    const int blocks = range_blocks(height, width);
    hipStream_t st = (hipStream_t)stream;
    if (cin == 1) hipLaunchKernelGGL(frame_range_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(frame_range_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    GS_LAUNCH_CHECK("frame_range_kernel");
    hipLaunchKernelGGL(frame_range_reduce, dim3(1), dim3(256), 0, st, blocks, workspace, range2);
    GS_LAUNCH_CHECK("frame_range_reduce");
    return GS_OK;
}

extern "C" int gs_frame_finish(void* stream, int height, int width, int cin, const float* render, int mode, int format,
                               const float* alpha, const float* range2, float alpha_min, int out_height, int out_width, void* out) {
    GS_REQUIRE(height > 0 && width > 0, "the image size must be positive");
    GS_REQUIRE(out_height >= height && out_width >= width, "the output cannot be smaller than the render (out_height >= height, out_width >= width)");
    GS_REQUIRE(mode == GS_FRAME_RGB || mode == GS_FRAME_DEPTH, "unknown mode (GS_FRAME_RGB or GS_FRAME_DEPTH)");
    GS_REQUIRE(format == GS_FRAME_F32 || format == GS_FRAME_U8, "unknown format (GS_FRAME_F32 or GS_FRAME_U8)");
    if (mode == GS_FRAME_RGB) GS_REQUIRE(cin == 3 || cin == 4, "a colour frame comes from a render of 3 or 4 channels: cin is 3 or 4");
    else GS_REQUIRE(cin == 1 || cin == 4, "a depth frame comes from channel cin - 1 of a four-channel render or a one-channel depth image: cin is 1 or 4");
    GS_REQUIRE((int64_t)height * width * cin * 4 <= kFrameMaxBytes &&
               (int64_t)out_height * out_width * 3 * (format == GS_FRAME_F32 ? 4 : 1) <= kFrameMaxBytes,
               "frame too large for the frame kernels' 32-bit byte offsets (H * W * cin * 4 and the output's bytes < 2^31)");
    GS_REQUIRE(render && out && (mode == GS_FRAME_RGB || (alpha && range2)), "null pointer");
    GS_REQUIRE((((uintptr_t)render | (uintptr_t)out | (uintptr_t)(mode == GS_FRAME_DEPTH ? alpha : nullptr)) & 15) == 0,
               "render, alpha and out must be 16-byte aligned");
    FrameArgs a;
    const unsigned P = (unsigned)(out_height * out_width);
    a.H = height; a.W = width; a.oW = out_width; a.groups = P >> 2; a.tail = P & 3u;
    a.src = render; a.alpha = alpha; a.range = range2; a.alpha_min = alpha_min; a.out = out;
    const unsigned threads = a.groups + (a.tail ? 1u : 0u), blocks = (threads + 255u) / 256u;
    if (format == GS_FRAME_F32) frame_launch<GS_FRAME_F32>(mode, cin, blocks, (hipStream_t)stream, a);
    else frame_launch<GS_FRAME_U8>(mode, cin, blocks, (hipStream_t)stream, a);
    GS_LAUNCH_CHECK("frame_finish_kernel");
    return GS_OK;
}
