// Activation maximisation: the two elementwise ends of a gradient-ascent step on the PIXELS (cnn_layer_visualization.py,
// deep_dream.py, generate_class_specific_samples.py of the reference's vendored pytorch-cnn-visualizations-master/src).  Between
// them runs the encoder: a forward cut short at a stage and the data-gradient-only walk back to the tiles; DESIGN.md section 3.43.
//
//   stage_seed_kernel<T>          J_t = mean_{y,x} act[t,y,x,ch_t] (partial sums) and dz, the gradient of -J_t in the form the
//                                 backward chain carries: -(1/(h w)) * lrelu'(act) at channel ch_t, zero everywhere else
//   slice_sum_kernel<.., SumOverCount>   (slice_sum.cuh) a tile's partial sums added in slice order, divided by h w: objective [T]
//   pixel_step_kernel<RULE, PROJ> one SGD, Adam or momentum-SGD step on x [T,3,H,W] fp32 in place, the projection of the new image
//                                 (none, clamp to [-1,1], or the round trip through bytes) and its bytes, in one pass
//
// Every product, quotient, difference and sum that reaches an output is a single correctly rounded fp32 operation (rn_mul, rn_add,
// rn_sub of rounded.cuh carry no `contract` flag; __fdiv_rn, rn_sqrt): numpy's fp32 arithmetic gives the same bits.  Both are streaming
// kernels: 16-byte loads and stores where the pointers allow, no LDS beyond four words of the block sum, no atomics, every sum in
// a fixed order.
#include "slice_sum.cuh"

#define FV_THREADS SLICE_THREADS

// Workgroup t * MIL_SEED_SLICES + s owns the pixels [s per, (s + 1) per) of tile t.  A work item is one 8-channel group of one
// pixel: it writes the group's eight dz values and, when it is the group of the tile's channel, reads that ONE activation.  A
// channel outside [0, C) selects nothing (dz all zero, J = 0): no address is formed from it.  part [T][MIL_SEED_SLICES]: the sum of
// the workgroup's activations by slice_sum.cuh's tree — per thread in work-item order, then the butterfly over the wave's lanes
// and the four waves in order: one summation tree per (h w, CP), whatever the grid does.
template <typename T>
__global__ __launch_bounds__(FV_THREADS) void stage_seed_kernel(const typename T::elem* __restrict__ act, const int* __restrict__ channels,
                                                               typename T::elem* __restrict__ dz, float* __restrict__ part, int hw, int per,
                                                               int CP, int C, float neg_inv, float slope) {
    __shared__ float red[FV_THREADS / 64];
    MIL_POISON_STATIC(red);
    const SliceRange sl = slice_range<MIL_SEED_SLICES, true>(hw, per);
    const int tid = threadIdx.x, p0 = sl.lo, p1 = sl.hi;
    const size_t t = sl.t;
    const int NG = CP >> 3;
    const int ch = channels[t];
    const int cg_t = (ch >= 0 && ch < C) ? ch >> 3 : -1, cj = ch & 7;
    float sum = 0.f;
    for (int idx = tid; idx < (p1 - p0) * NG; idx += FV_THREADS) {
        const int i = idx / NG, cg = idx - i * NG;
        const size_t off = (t * hw + p0 + i) * CP + cg * 8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (cg == cg_t) {
            const float a = (float)act[off + cj];
            sum = rn_add(sum, a);
            const float g = rn_mul(neg_inv, lrelu_grad(a, slope));
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j == cj ? g : 0.f;
        }
        store8<T>(dz + off, v);
    }
    block_sum(sum, red, part + t * MIL_SEED_SLICES + sl.s);
}

// rint(clip(x / 2 + 0.5, 0, 1) * 255): x / 2 is exact, the sum and the product are rounded once each, the rounding to an integer is
// half-to-even (np.round).  A NaN encodes as 0.
__device__ __forceinline__ unsigned fv_encode(float x) {
    float y = rn_add(rn_mul(x, 0.5f), 0.5f);
    y = y > 0.f ? (y > 1.f ? 1.f : y) : 0.f;
    return (unsigned)rintf(rn_mul(y, 255.0f));
}

struct PixelStepArgs {
    float lr, wd, beta1, omb1, beta2, omb2, bc1, sqrt_bc2, eps;
};

// One thread = the four elements 4 q .. 4 q + 3 of the linear index (fewer in the last group).  vec: every pointer is on its
// 16-byte (u8_out: 4-byte) grid, so a whole group is one aligned load and store per tensor; the last, short group goes element by
// element.  RULE 0: SGD, 1: Adam, 2: SGD with momentum (m is its buffer, a.beta1 the momentum; mil_pixel_momentum_step).  PROJ 0: none, 1: clamp to [-1, 1], 2: table[encode(x)], the round trip through bytes.
template <int RULE, int PROJ>
__global__ __launch_bounds__(FV_THREADS) void pixel_step_kernel(float* __restrict__ x, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, uint8_t* __restrict__ u8_out,
                                                               const float* __restrict__ table, PixelStepArgs a, unsigned long long total,
                                                               int vec) {
    const unsigned long long q = (unsigned long long)blockIdx.x * FV_THREADS + threadIdx.x;
    const unsigned long long i0 = q * 4;
    if (i0 >= total) return;
    const int cnt = total - i0 < 4 ? (int)(total - i0) : 4;
    const bool whole = vec && cnt == 4;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
    if (whole) {
        const f32x4_t rx = *reinterpret_cast<const f32x4_t*>(x + i0), rg = *reinterpret_cast<const f32x4_t*>(g + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { xv[j] = rx[j]; gv[j] = rg[j]; }
        if constexpr (RULE == 1) {
            const f32x4_t rm = *reinterpret_cast<const f32x4_t*>(m + i0), rv = *reinterpret_cast<const f32x4_t*>(v + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) { mv[j] = rm[j]; vv[j] = rv[j]; }
        }
        if constexpr (RULE == 2) {
            const f32x4_t rm = *reinterpret_cast<const f32x4_t*>(m + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) mv[j] = rm[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) {
                xv[j] = x[i0 + j]; gv[j] = g[i0 + j];
                if constexpr (RULE == 1) { mv[j] = m[i0 + j]; vv[j] = v[i0 + j]; }
                if constexpr (RULE == 2) mv[j] = m[i0 + j];
            }
    }
    unsigned codes = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gd = rn_add(gv[j], rn_mul(a.wd, xv[j]));
        float xn;
        if constexpr (RULE == 0) {
            xn = rn_sub(xv[j], rn_mul(a.lr, gd));
        } else if constexpr (RULE == 2) {
            mv[j] = rn_add(rn_mul(a.beta1, mv[j]), gd);
            xn = rn_sub(xv[j], rn_mul(a.lr, mv[j]));
        } else {
            mv[j] = rn_add(rn_mul(a.beta1, mv[j]), rn_mul(a.omb1, gd));
            vv[j] = rn_add(rn_mul(a.beta2, vv[j]), rn_mul(rn_mul(a.omb2, gd), gd));
            const float denom = rn_add(__fdiv_rn(rn_sqrt(vv[j]), a.sqrt_bc2), a.eps);
            xn = rn_sub(xv[j], __fdiv_rn(rn_mul(__fdiv_rn(a.lr, a.bc1), mv[j]), denom));
        }
        if constexpr (PROJ == 1) xn = xn < -1.f ? -1.f : (xn > 1.f ? 1.f : xn);
        unsigned code = 0;
        if (PROJ == 2 || u8_out) code = fv_encode(xn);
        if constexpr (PROJ == 2) xn = table[code];
        xv[j] = xn;
        codes |= code << (8 * j);
    }
    if (whole) {
        *reinterpret_cast<f32x4_t*>(x + i0) = f32x4_t{xv[0], xv[1], xv[2], xv[3]};
        if constexpr (RULE == 1) {
            *reinterpret_cast<f32x4_t*>(m + i0) = f32x4_t{mv[0], mv[1], mv[2], mv[3]};
            *reinterpret_cast<f32x4_t*>(v + i0) = f32x4_t{vv[0], vv[1], vv[2], vv[3]};
        }
        if constexpr (RULE == 2) *reinterpret_cast<f32x4_t*>(m + i0) = f32x4_t{mv[0], mv[1], mv[2], mv[3]};
        if (u8_out) *reinterpret_cast<unsigned*>(u8_out + i0) = codes;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) {
                x[i0 + j] = xv[j];
                if constexpr (RULE == 1) { m[i0 + j] = mv[j]; v[i0 + j] = vv[j]; }
                if constexpr (RULE == 2) m[i0 + j] = mv[j];
                if (u8_out) u8_out[i0 + j] = (uint8_t)((codes >> (8 * j)) & 255u);
            }
    }
}

// include/mil_hip.h has the contracts.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call.
extern "C" int mil_stage_seed(const void* act, const int* channels, float* objective, void* dz, float* ws, int n, int h, int w, int cp,
                              int c, float slope, int dtype, void* stream) {
    if (!act || !channels || !objective || !dz || !ws) return MIL_ERR_ARG;
    const int rc = stage_shape(n, h, w, cp, c, dtype);
    if (rc != MIL_OK || n == 0) return rc;
    const int hw = h * w, per = (hw + MIL_SEED_SLICES - 1) / MIL_SEED_SLICES;
    const float neg_inv = -(1.0f / (float)hw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n * MIL_SEED_SLICES);
    if (dtype == MIL_DT_BF16)
        hipLaunchKernelGGL(stage_seed_kernel<BF16>, grid, dim3(FV_THREADS), 0, st, (const __bf16*)act, channels, (__bf16*)dz, ws, hw, per, cp, c,
                           neg_inv, slope);
    else
        hipLaunchKernelGGL(stage_seed_kernel<F32>, grid, dim3(FV_THREADS), 0, st, (const float*)act, channels, (float*)dz, ws, hw, per, cp, c,
                           neg_inv, slope);
    MIL_CHECK_LAUNCH();
    launch_slice_sum<MIL_SEED_SLICES>(st, ws, objective, n, SumOverCount{(float)hw});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// What mil_pixel_step and mil_pixel_momentum_step share, behind their own rule-specific checks: the checks of x, g, the
// projection and the two scalars every rule has, the grid, and `vec` from the pointers RULE actually uses (x, g, the moments
// that are not null, u8_out).
template <int RULE>
static int pixel_step_entry(float* x, const float* g, float* m, float* v, unsigned char* u8_out, const float* table, size_t total, int project,
                            const PixelStepArgs& a, void* stream) {
    if (!x || !g || project < 0 || project > 2) return MIL_ERR_ARG;
    if (project == 2 && !table) return MIL_ERR_ARG;
    if (!(a.lr == a.lr) || !(a.wd == a.wd)) return MIL_ERR_ARG;
    if (total == 0) return MIL_OK;
    const unsigned long long blocks = (((unsigned long long)total + 3) / 4 + FV_THREADS - 1) / FV_THREADS;
    if (blocks > INT_MAX) return MIL_ERR_UNSUPPORTED;
    const uintptr_t grid16 = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
    const int vec = !(grid16 & 15) && !(reinterpret_cast<uintptr_t>(u8_out) & 3);
    const dim3 grid((unsigned)blocks), block(FV_THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (project == 0)
        hipLaunchKernelGGL((pixel_step_kernel<RULE, 0>), grid, block, 0, st, x, g, m, v, u8_out, table, a, (unsigned long long)total, vec);
    else if (project == 1)
        hipLaunchKernelGGL((pixel_step_kernel<RULE, 1>), grid, block, 0, st, x, g, m, v, u8_out, table, a, (unsigned long long)total, vec);
    else
        hipLaunchKernelGGL((pixel_step_kernel<RULE, 2>), grid, block, 0, st, x, g, m, v, u8_out, table, a, (unsigned long long)total, vec);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_pixel_step(float* x, const float* g, float* m, float* v, unsigned char* u8_out, const float* table, size_t total,
                              int rule, int project, float lr, float weight_decay, float beta1, float one_minus_beta1, float beta2,
                              float one_minus_beta2, float bc1, float sqrt_bc2, float eps, void* stream) {
    if (rule < 0 || rule > 1) return MIL_ERR_ARG;
    if (rule == 1 && (!m || !v || !(bc1 > 0.f) || !(sqrt_bc2 > 0.f) || !(eps >= 0.f))) return MIL_ERR_ARG;
    const PixelStepArgs a{lr, weight_decay, beta1, one_minus_beta1, beta2, one_minus_beta2, bc1, sqrt_bc2, eps};
    if (rule == 0) return pixel_step_entry<0>(x, g, nullptr, nullptr, u8_out, table, total, project, a, stream);     // SGD reads no moments
    return pixel_step_entry<1>(x, g, m, v, u8_out, table, total, project, a, stream);
}

// The third RULE of the kernel above behind an entry of its own: mil_pixel_step's rules and their instantiations stay as they are.
extern "C" int mil_pixel_momentum_step(float* x, const float* g, float* buf, unsigned char* u8_out, const float* table, size_t total,
                                       int project, float lr, float weight_decay, float momentum, void* stream) {
    if (!buf || !(momentum == momentum)) return MIL_ERR_ARG;
    return pixel_step_entry<2>(x, g, buf, nullptr, u8_out, table, total, project, PixelStepArgs{lr, weight_decay, momentum, 0.f, 0.f, 0.f, 1.f, 1.f, 0.f},
                               stream);
}
