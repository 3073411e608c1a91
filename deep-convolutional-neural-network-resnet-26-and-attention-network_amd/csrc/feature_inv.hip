// Feature inversion (inverted_representation.py of the reference's vendored pytorch-cnn-visualizations-master/src) and the pixel
// regularisers it brings: the elementwise stages of a step around the encoder's truncated forward and its data-gradient walk;
// DESIGN.md section 3.46.  (The momentum step is the third RULE of feature_vis.hip's pixel_step_kernel.)
//
//   stage_energy_kernel<T>    E_t = sum of target^2 over the real channels of a stage output (partial sums)
//   stage_match_kernel<T>     dz, the gradient of weight * sum (act - target)^2 / E_t with respect to the pre-activation map, and the
//                             partial sums of the distance
//   slice_sum_kernel<..>      (slice_sum.cuh) a row's partial sums added in slice order: energy [T], terms [2,T]; for loss [T]
//                             followed by weight * (D / E)
//   pixel_reg_kernel<TERMS>   the pixel gradient moved back through the jitter plus the gradients of the alpha norm and of the total
//                             variation of x; with TERMS the partial sums of the two norms themselves
//   pixel_shift_kernel        the jittered copy of x: a cyclic shift of every plane, bit for bit
//
// The arithmetic contract of feature_vis.hip: every product, quotient, difference and sum that reaches an output is a single
// correctly rounded fp32 operation in the order include/mil_hip.h writes down; no atomics, every sum in a fixed order; streaming
// kernels whose neighbours come from global memory (L2), no LDS beyond the words of the block sums; 16-byte accesses where the
// pointers (the stage kernels) or the rows (the pixel kernels) allow, element by element otherwise.
#include "slice_sum.cuh"

#define FI_THREADS SLICE_THREADS

template <typename T>
__device__ __forceinline__ void fi_load8(const typename T::elem* p, float (&v)[8], int vec) {
    if (vec) { load8<T>(p, v); return; }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)p[j];
}

template <typename T>
__device__ __forceinline__ void fi_store8(typename T::elem* p, const float (&v)[8], int vec) {
    if (vec) { store8<T>(p, v); return; }
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = (typename T::elem)v[j];
}

// Workgroup t * MIL_SEED_SLICES + s owns the pixels [s per, (s + 1) per) of tile t, a work item is one 8-channel group of one pixel
// (stage_seed_kernel's scheme).  The sum: per thread in work-item order and, within a group, in channel order; then slice_sum.cuh's
// butterfly and the four waves in order.
template <typename T>
__global__ __launch_bounds__(FI_THREADS) void stage_energy_kernel(const typename T::elem* __restrict__ target, float* __restrict__ part,
                                                                 int hw, int per, int CP, int C, int vec) {
    __shared__ float red[FI_THREADS / 64];
    MIL_POISON_STATIC(red);
    const SliceRange sl = slice_range<MIL_SEED_SLICES, true>(hw, per);
    const int tid = threadIdx.x, p0 = sl.lo, p1 = sl.hi;
    const size_t t = sl.t;
    const int NG = CP >> 3;
    float sum = 0.f;
    for (int idx = tid; idx < (p1 - p0) * NG; idx += FI_THREADS) {
        const int i = idx / NG, cg = idx - i * NG;
        float a[8];
        fi_load8<T>(target + (t * hw + p0 + i) * CP + cg * 8, a, vec);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (cg * 8 + j < C) sum = rn_add(sum, rn_mul(a[j], a[j]));
    }
    block_sum(sum, red, part + t * MIL_SEED_SLICES + sl.s);
}

template <typename T>
__global__ __launch_bounds__(FI_THREADS) void stage_match_kernel(const typename T::elem* __restrict__ act, const typename T::elem* __restrict__ target,
                                                                const float* __restrict__ energy, typename T::elem* __restrict__ dz,
                                                                float* __restrict__ part, int hw, int per, int CP, int C, float two_w,
                                                                float slope, int vec) {
    __shared__ float red[FI_THREADS / 64];
    MIL_POISON_STATIC(red);
    const SliceRange sl = slice_range<MIL_SEED_SLICES, true>(hw, per);
    const int tid = threadIdx.x, p0 = sl.lo, p1 = sl.hi;
    const size_t t = sl.t;
    const int NG = CP >> 3;
    const float scale = __fdiv_rn(two_w, energy[t]);
    float sum = 0.f;
    for (int idx = tid; idx < (p1 - p0) * NG; idx += FI_THREADS) {
        const int i = idx / NG, cg = idx - i * NG;
        const size_t off = (t * hw + p0 + i) * CP + cg * 8;
        float a[8], g[8], o[8];
        fi_load8<T>(act + off, a, vec);
        fi_load8<T>(target + off, g, vec);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = 0.f;
            if (cg * 8 + j < C) {
                const float d = rn_sub(a[j], g[j]);
                sum = rn_add(sum, rn_mul(d, d));
                o[j] = rn_mul(rn_mul(scale, d), lrelu_grad(a[j], slope));
            }
        }
        fi_store8<T>(dz + off, o, vec);
    }
    block_sum(sum, red, part + t * MIL_SEED_SLICES + sl.s);
}

// Where a linear element of a tile [3,H,W] lies; fi_next: the element behind it.
struct FiCursor {
    int c, i, j;
};
__device__ __forceinline__ FiCursor fi_cursor(int e, int HW, int W) {
    FiCursor k;
    k.c = e / HW;
    const int r = e - k.c * HW;
    k.i = r / W;
    k.j = r - k.i * W;
    return k;
}
__device__ __forceinline__ void fi_next(FiCursor& k, int H, int W) {
    if (++k.j == W) {
        k.j = 0;
        if (++k.i == H) { k.i = 0; ++k.c; }
    }
}

// Four consecutive floats on any 4-byte boundary as one 16-byte access (global memory takes unaligned dwordx4 accesses).
typedef f32x4_t f32x4_u __attribute__((aligned(4)));
__device__ __forceinline__ void fi_load4(const float* p, float (&v)[4]) {
    const f32x4_u r = *reinterpret_cast<const f32x4_u*>(p);
#pragma unroll
    for (int m = 0; m < 4; ++m) v[m] = r[m];
}
__device__ __forceinline__ void fi_store4(float* p, const float (&v)[4]) {
    *reinterpret_cast<f32x4_u*>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
}

// v[m] = src[tile][c, (i + sy) mod H, (j + sx) mod W] for the cnt elements from the cursor on; 0 <= sy < H, 0 <= sx < W.  One
// 16-byte load where the four lie in one row and their sources do not wrap, element by element otherwise.
__device__ __forceinline__ void fi_gather4(const float* src, size_t base, int HW, int H, int W, FiCursor k, int cnt, int sy, int sx, float (&v)[4]) {
    {
        const int si = k.i + sy >= H ? k.i + sy - H : k.i + sy, sj = k.j + sx >= W ? k.j + sx - W : k.j + sx;
        if (cnt == 4 && k.j + 3 < W && sj + 3 < W) {
            fi_load4(src + base + (size_t)k.c * HW + (size_t)si * W + sj, v);
            return;
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m < cnt) {
            const int si = k.i + sy >= H ? k.i + sy - H : k.i + sy, sj = k.j + sx >= W ? k.j + sx - W : k.j + sx;
            v[m] = src[base + (size_t)k.c * HW + (size_t)si * W + sj];
            fi_next(k, H, W);
        }
    }
}

struct PixelRegArgs {
    float ca, ct;           // alpha_weight * alpha, 2 * tv_weight
    int alpha, alpha_on, tv_on, dy, dx;
};

// Workgroup t * MIL_REG_SLICES + s owns the groups [s per, (s + 1) per) of tile t, a group being four consecutive elements of the
// tile's 3 H W (fewer in the last).  A whole group is one 16-byte load of x and one store of out; where it lies in one row, the rows
// above and below are one load each, the neighbours left of its first and right of its last element one word each, and the other
// horizontal neighbours are in the registers.  A group that crosses a row end reads its neighbours word by word.
// g and out carry no __restrict__: at shift (0, 0) they may be one tensor, and a thread reads exactly the elements it writes.
template <bool TERMS>
__global__ __launch_bounds__(FI_THREADS) void pixel_reg_kernel(const float* __restrict__ x, const float* g, float* out, float* __restrict__ part,
                                                              int n, int H, int W, int per, PixelRegArgs a) {
    __shared__ float red[2][FI_THREADS / 64];
    MIL_POISON_STATIC(red);
    const int HW = H * W, E = 3 * HW;
    const SliceRange sl = slice_range<MIL_REG_SLICES, true>((E + 3) >> 2, per);
    const int tid = threadIdx.x, g0 = sl.lo, g1 = sl.hi;
    const size_t t = sl.t;
    const size_t base = t * (size_t)E;
    const bool need_pow = TERMS || a.alpha_on, need_tv = TERMS || a.tv_on;
    float sum_a = 0.f, sum_t = 0.f;
    for (int q = g0 + tid; q < g1; q += FI_THREADS) {
        const int e0 = q * 4, cnt = E - e0 < 4 ? E - e0 : 4;
        const size_t at0 = base + e0;
        FiCursor k = fi_cursor(e0, HW, W);
        const bool row4 = cnt == 4 && k.j + 3 < W;
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, up[4] = {0.f, 0.f, 0.f, 0.f}, dn[4] = {0.f, 0.f, 0.f, 0.f}, ov[4];
        float lf = 0.f, rt = 0.f;
        if (cnt == 4) {
            fi_load4(x + at0, xv);
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < cnt) xv[m] = x[at0 + m];
        }
        if (need_tv && row4) {
            if (k.i >= 1) fi_load4(x + at0 - W, up);
            if (k.i < H - 1) fi_load4(x + at0 + W, dn);
            if (k.j >= 1) lf = x[at0 - 1];
            if (k.j + 4 < W) rt = x[at0 + 4];
        }
        fi_gather4(g, base, HW, H, W, k, cnt, a.dy, a.dx, gv);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (m < cnt) {
                const size_t at = at0 + m;
                const float v = xv[m];
                float r = gv[m], p = 0.f, st = 0.f, dd = 0.f, dr = 0.f;
                const bool own = k.i < H - 1 && k.j < W - 1, above = k.i >= 1 && k.j < W - 1, before = k.j >= 1 && k.i < H - 1;
                if (need_pow) {
                    p = v;
                    for (int e = 2; e < a.alpha; ++e) p = rn_mul(p, v);
                }
                if (a.alpha_on) r = rn_add(r, rn_mul(a.ca, p));
                if (need_tv) {
                    float right, down, upper, left;
                    if (row4) {
                        right = m < 3 ? xv[(m + 1) & 3] : rt;
                        left = m > 0 ? xv[(m + 3) & 3] : lf;
                        down = dn[m];
                        upper = up[m];
                    } else {
                        right = own ? (m + 1 < cnt ? xv[(m + 1) & 3] : x[at + 1]) : 0.f;
                        left = before ? (m > 0 ? xv[(m + 3) & 3] : x[at - 1]) : 0.f;
                        down = own ? x[at + W] : 0.f;
                        upper = above ? x[at - W] : 0.f;
                    }
                    if (own) {
                        dd = rn_sub(v, down);
                        dr = rn_sub(v, right);
                        st = rn_add(st, rn_add(dd, dr));
                    }
                    if (above) st = rn_add(st, rn_sub(v, upper));
                    if (before) st = rn_add(st, rn_sub(v, left));
                }
                if (a.tv_on) r = rn_add(r, rn_mul(a.ct, st));
                if (TERMS) {
                    sum_a = rn_add(sum_a, rn_mul(p, v));
                    if (own) sum_t = rn_add(sum_t, rn_add(rn_mul(dd, dd), rn_mul(dr, dr)));
                }
                ov[m] = r;
                fi_next(k, H, W);
            }
        }
        if (cnt == 4) {
            fi_store4(out + at0, ov);
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < cnt) out[at0 + m] = ov[m];
        }
    }
    if constexpr (TERMS) {
        sum_a = wave_sum(sum_a);
        sum_t = wave_sum(sum_t);
        waves_put(sum_a, red[0]);
        waves_put(sum_t, red[1]);
        __syncthreads();
        if (tid < 2) part[((size_t)tid * n + t) * MIL_REG_SLICES + sl.s] = waves_get(red[tid]);         // part [2][n][MIL_REG_SLICES]
    }
}

// out[tile][c,i,j] = x[tile][c, (i + sy) mod H, (j + sx) mod W], (sy, sx) = (-dy mod H, -dx mod W) formed by the entry point.
__global__ __launch_bounds__(FI_THREADS) void pixel_shift_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int per, int sy,
                                                                int sx) {
    const int HW = H * W, E = 3 * HW;
    const SliceRange sl = slice_range<MIL_REG_SLICES, true>((E + 3) >> 2, per);
    const int tid = threadIdx.x, g0 = sl.lo, g1 = sl.hi;
    const size_t t = sl.t;
    const size_t base = t * (size_t)E;
    for (int q = g0 + tid; q < g1; q += FI_THREADS) {
        const int e0 = q * 4, cnt = E - e0 < 4 ? E - e0 : 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        fi_gather4(x, base, HW, H, W, fi_cursor(e0, HW, W), cnt, sy, sx, v);
        if (cnt == 4) {
            fi_store4(out + base + e0, v);
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < cnt) out[base + e0 + m] = v[m];
        }
    }
}

static int fi_mod(int v, int m) { return ((v % m) + m) % m; }

// include/mil_hip.h has the contracts.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call.
extern "C" int mil_stage_energy(const void* target, float* energy, float* ws, int n, int h, int w, int cp, int c, int dtype, void* stream) {
    if (!target || !energy || !ws) return MIL_ERR_ARG;
    const int rc = stage_shape(n, h, w, cp, c, dtype);
    if (rc != MIL_OK || n == 0) return rc;
    const int hw = h * w, per = (hw + MIL_SEED_SLICES - 1) / MIL_SEED_SLICES, vec = mil_on16(target);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n * MIL_SEED_SLICES);
    if (dtype == MIL_DT_BF16)
        hipLaunchKernelGGL(stage_energy_kernel<BF16>, grid, dim3(FI_THREADS), 0, st, (const __bf16*)target, ws, hw, per, cp, c, vec);
    else
        hipLaunchKernelGGL(stage_energy_kernel<F32>, grid, dim3(FI_THREADS), 0, st, (const float*)target, ws, hw, per, cp, c, vec);
    MIL_CHECK_LAUNCH();
    launch_slice_sum<MIL_SEED_SLICES>(st, ws, energy, n, SumItself{});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_stage_match(const void* act, const void* target, const float* energy, float* loss, void* dz, float* ws, int n, int h, int w,
                               int cp, int c, float weight, float slope, int dtype, void* stream) {
    if (!act || !target || !energy || !loss || !dz || !ws) return MIL_ERR_ARG;
    const int rc = stage_shape(n, h, w, cp, c, dtype);
    if (rc != MIL_OK || n == 0) return rc;
    const int hw = h * w, per = (hw + MIL_SEED_SLICES - 1) / MIL_SEED_SLICES, vec = mil_on16(act) && mil_on16(target) && mil_on16(dz);
    const float two_w = 2.0f * weight;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n * MIL_SEED_SLICES);
    if (dtype == MIL_DT_BF16)
        hipLaunchKernelGGL(stage_match_kernel<BF16>, grid, dim3(FI_THREADS), 0, st, (const __bf16*)act, (const __bf16*)target, energy, (__bf16*)dz, ws,
                           hw, per, cp, c, two_w, slope, vec);
    else
        hipLaunchKernelGGL(stage_match_kernel<F32>, grid, dim3(FI_THREADS), 0, st, (const float*)act, (const float*)target, energy, (float*)dz, ws, hw,
                           per, cp, c, two_w, slope, vec);
    MIL_CHECK_LAUNCH();
    launch_slice_sum<MIL_SEED_SLICES>(st, ws, loss, n, SumWeightedRatio{energy, weight});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// MIL_OK when [n,3,H,W] is a stack the pixel kernels take.
static int fi_pixel_shape(int n, int H, int W) {
    if (n < 0 || H < 1 || W < 1) return MIL_ERR_ARG;
    if (n > 0 && (3ull * (unsigned long long)H * W > 0x7fffffffull - 3 || n > INT_MAX / MIL_REG_SLICES)) return MIL_ERR_UNSUPPORTED;
    return MIL_OK;
}

extern "C" int mil_pixel_reg(const float* x, const float* g, float* out, float* terms, float* ws, int n, int H, int W, int alpha,
                             float alpha_weight, float tv_weight, int dy, int dx, void* stream) {
    if (!x || !g || !out || (terms && !ws) || alpha < 2 || alpha > 8 || (alpha & 1)) return MIL_ERR_ARG;
    if (!(alpha_weight == alpha_weight) || !(tv_weight == tv_weight)) return MIL_ERR_ARG;
    const int rc = fi_pixel_shape(n, H, W);
    if (rc != MIL_OK) return rc;
    dy = fi_mod(dy, H);
    dx = fi_mod(dx, W);
    const unsigned long long bytes = 12ull * (unsigned long long)n * H * W;
    if (out == g ? (dy || dx) : mil_overlap(out, g, bytes)) return MIL_ERR_ARG;
    if (mil_overlap(out, x, bytes)) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    const int G = (3 * H * W + 3) / 4, per = (G + MIL_REG_SLICES - 1) / MIL_REG_SLICES;
    const PixelRegArgs a{alpha_weight * (float)alpha, 2.0f * tv_weight, alpha, alpha_weight != 0.f, tv_weight != 0.f, dy, dx};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n * MIL_REG_SLICES);
    if (terms) {
        hipLaunchKernelGGL(pixel_reg_kernel<true>, grid, dim3(FI_THREADS), 0, st, x, g, out, ws, n, H, W, per, a);
        MIL_CHECK_LAUNCH();
        launch_slice_sum<MIL_REG_SLICES>(st, ws, terms, 2 * n, SumItself{});
    } else {
        hipLaunchKernelGGL(pixel_reg_kernel<false>, grid, dim3(FI_THREADS), 0, st, x, g, out, ws, n, H, W, per, a);
    }
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_pixel_shift(const float* x, float* out, int n, int H, int W, int dy, int dx, void* stream) {
    if (!x || !out) return MIL_ERR_ARG;
    const int rc = fi_pixel_shape(n, H, W);
    if (rc != MIL_OK) return rc;
    if (mil_overlap(out, x, 12ull * (unsigned long long)n * H * W)) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    const int G = (3 * H * W + 3) / 4, per = (G + MIL_REG_SLICES - 1) / MIL_REG_SLICES;
    hipLaunchKernelGGL(pixel_shift_kernel, dim3((unsigned)n * MIL_REG_SLICES), dim3(FI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), x, out, H, W,
                       per, fi_mod(-fi_mod(dy, H), H), fi_mod(-fi_mod(dx, W), W));
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
