// Path attributions of a slide's tiles: the two elementwise ends of integrated gradients and SmoothGrad
// (integrated_gradients.py, smooth_grad.py of the reference's vendored pytorch-cnn-visualizations-master/src).  Between them
// runs the encoder, forward and backward, with stem_dgrad_kernel<T, true> (stem_dgrad.hip) adding each step's gradient into
// the running sum; DESIGN.md section 3.40.
//
//   path_point_kernel<U8>    out[t,c,y,x] = base[c] + alpha * (v - base[c]) + sigma * n(seed, sample, i)      fp32 [T,3,H,W]
//   attr_finish_kernel<U8>   attr = (v - base[c]) * acc, a map [T,H,W] of it (or of acc), and 32 partial sums per tile
//   slice_sum_kernel<..>     (slice_sum.cuh) the 32 partial sums of a tile added in slice order: tile_sum [T]
//
// v is the fp32 tile value or mil_u8_decode(code) of a uint8 tile (u8_feed.cuh: bit for bit `U8Tiles.float()`).  Every
// product, difference and sum that reaches an output is a single correctly rounded fp32 operation (rn_sub, rn_mul,
// rn_add of rounded.cuh, compiled with contraction off: no product meets a sum in a fused multiply-add), so torch's fp32 arithmetic
// on the CPU gives the same bits.
//
// The noise is counter-based: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
// Random123 generator) keyed by the 64-bit seed, counter (i >> 2 low, i >> 2 high, sample, 0) with i the linear element index:
// one counter yields the four standard normals of elements 4 (i >> 2) .. + 3 by two Box-Muller transforms, and the thread that
// owns those four elements draws them — a value depends on (seed, sample, i) and on nothing else, not on the launch geometry
// and not on T, H or W beyond i.  Both kernels are streaming: 16-byte loads and stores where the pointers allow, no LDS beyond
// four words of the block sum, no atomics, every sum in a fixed order.
#include "slice_sum.cuh"
#include "u8_feed.cuh"

#define PA_THREADS SLICE_THREADS

__device__ __forceinline__ void pa_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                                 unsigned (&r)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// Two standard normals from two words: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1); both exact in fp32,
// as is 2 u2.  u1 == 1: log = 0, the radius and both normals are zeros.
__device__ __forceinline__ void pa_box_muller(unsigned a, unsigned b, float& n0, float& n1) {
    const float u1 = rn_mul((float)((a >> 8) + 1u), 0x1p-24f), u2 = rn_mul((float)(b >> 8), 0x1p-24f);
    const float rad = __fsqrt_rn(rn_mul(-2.0f, logf(u1)));
    float s, c;
    sincospif(rn_mul(2.0f, u2), &s, &c);
    n0 = rn_mul(rad, c);
    n1 = rn_mul(rad, s);
}

// One thread = the four elements 4 q .. 4 q + 3 of the linear index (fewer in the last group).  vec: both pointers are on the
// 16-byte (uint8: 4-byte) grid, so group q is one aligned load and one aligned store.
template <bool U8>
__global__ __launch_bounds__(PA_THREADS) void path_point_kernel(const void* __restrict__ tiles, float* __restrict__ out, float b0, float b1,
                                                               float b2, float alpha, float noise_level, const float* __restrict__ range,
                                                               unsigned k0, unsigned k1, unsigned sample, unsigned long long total,
                                                               unsigned hw, int vec) {
    const unsigned long long q = (unsigned long long)blockIdx.x * PA_THREADS + threadIdx.x;
    const unsigned long long i0 = q * 4;
    if (i0 >= total) return;
    const int cnt = total - i0 < 4 ? (int)(total - i0) : 4;
    const bool whole = vec && cnt == 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (U8) {
        const uint8_t* src = static_cast<const uint8_t*>(tiles);
        if (whole) {
            const unsigned w = *reinterpret_cast<const unsigned*>(src + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = mil_u8_decode((w >> (8 * j)) & 255u);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) v[j] = mil_u8_decode(src[i0 + j]);
        }
    } else {
        const float* src = static_cast<const float*>(tiles);
        if (whole) {
            const f32x4_t r = *reinterpret_cast<const f32x4_t*>(src + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = r[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) v[j] = src[i0 + j];
        }
    }
    // the colour channel of element i is (i / hw) % 3; four consecutive elements may cross a plane (hw need not be a multiple of 4)
    const unsigned long long plane = i0 / hw;
    unsigned rem = (unsigned)(i0 - plane * hw);
    int c = (int)(plane % 3);
    float p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float b = c == 0 ? b0 : (c == 1 ? b1 : b2);
        p[j] = rn_add(b, rn_mul(alpha, rn_sub(v[j], b)));
        if (++rem == hw) { rem = 0; c = c == 2 ? 0 : c + 1; }
    }
    if (noise_level != 0.f) {
        const float sigma = range ? rn_mul(noise_level, rn_sub(range[1], range[0])) : noise_level;
        unsigned r[4];
        pa_philox4x32_10((unsigned)q, (unsigned)(q >> 32), sample, 0u, k0, k1, r);
        float n[4];
        pa_box_muller(r[0], r[1], n[0], n[1]);
        pa_box_muller(r[2], r[3], n[2], n[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = rn_add(p[j], rn_mul(sigma, n[j]));
    }
    if (whole) {
        *reinterpret_cast<f32x4_t*>(out + i0) = f32x4_t{p[0], p[1], p[2], p[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) out[i0 + j] = p[j];
    }
}

// Workgroup t * MIL_ATTR_SLICES + s owns the pixels [s per, (s + 1) per) of tile t (per: a multiple of 4), all three channels
// of each: a thread takes four consecutive pixels at a time.  vec: hw % 4 == 0 and every pointer on its 16-byte (uint8: 4-byte) grid.
// part (nullable) [T][MIL_ATTR_SLICES]: the sum of attr over the workgroup's pixels — per thread in pixel order, (a0 + a1) + a2
// per pixel, then slice_sum.cuh's butterfly over the wave's lanes and the four waves in order: one summation tree per (hw), no
// atomics.  The start of a slice is NOT clamped to hw (an empty trailing slice has p0 > p1 and its loop does not run).
template <bool U8>
__global__ __launch_bounds__(PA_THREADS) void attr_finish_kernel(const float* __restrict__ acc, const void* __restrict__ tiles, float b0, float b1,
                                                                float b2, float* __restrict__ attr, float* __restrict__ map, int mode,
                                                                float* __restrict__ part, int hw, int per, int vec) {
    __shared__ float red[PA_THREADS / 64];
    MIL_POISON_STATIC(red);
    const SliceRange sl = slice_range<MIL_ATTR_SLICES, false>(hw, per);
    const int tid = threadIdx.x, p0 = sl.lo, p1 = sl.hi;
    const size_t t = sl.t;
    const bool need_x = attr || part || (map && mode != 2);
    const float base[3] = {b0, b1, b2};
    float sum = 0.f;
    for (int p = p0 + tid * 4; p < p1; p += PA_THREADS * 4) {
        const int cnt = p1 - p < 4 ? p1 - p : 4;
        const bool whole = vec && cnt == 4;
        float g[3][4], a[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t at = (t * 3 + c) * (size_t)hw + p;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (whole) {
                const f32x4_t r = *reinterpret_cast<const f32x4_t*>(acc + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) g[c][j] = r[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[c][j] = j < cnt ? acc[at + j] : 0.f;
            }
            if (need_x) {
                if constexpr (U8) {
                    const uint8_t* src = static_cast<const uint8_t*>(tiles);
                    if (whole) {
                        const unsigned w = *reinterpret_cast<const unsigned*>(src + at);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = mil_u8_decode((w >> (8 * j)) & 255u);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < cnt) v[j] = mil_u8_decode(src[at + j]);
                    }
                } else {
                    const float* src = static_cast<const float*>(tiles);
                    if (whole) {
                        const f32x4_t r = *reinterpret_cast<const f32x4_t*>(src + at);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = r[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < cnt) v[j] = src[at + j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) a[c][j] = need_x ? rn_mul(rn_sub(v[j], base[c]), g[c][j]) : 0.f;
            if (attr) {
                if (whole) {
                    *reinterpret_cast<f32x4_t*>(attr + at) = f32x4_t{a[c][0], a[c][1], a[c][2], a[c][3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < cnt) attr[at + j] = a[c][j];
                }
            }
        }
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float tot = rn_add(rn_add(a[0][j], a[1][j]), a[2][j]);
            if (mode == 0) m[j] = fabsf(tot);
            else if (mode == 1) m[j] = fmaxf(fmaxf(fabsf(a[0][j]), fabsf(a[1][j])), fabsf(a[2][j]));
            else m[j] = fmaxf(fmaxf(fabsf(g[0][j]), fabsf(g[1][j])), fabsf(g[2][j]));
            if (j < cnt) sum = rn_add(sum, tot);
        }
        if (map) {
            const size_t at = t * (size_t)hw + p;
            if (whole) {
                *reinterpret_cast<f32x4_t*>(map + at) = f32x4_t{m[0], m[1], m[2], m[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) map[at + j] = m[j];
            }
        }
    }
    if (part) block_sum(sum, red, part + t * MIL_ATTR_SLICES + sl.s);          // (part is the same for the whole workgroup)
}

// include/mil_hip.h has the contracts.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call.
extern "C" int mil_path_point(const void* tiles, int is_u8, float* out, float base0, float base1, float base2, float alpha,
                              float noise_level, const float* range, unsigned long long seed, unsigned sample, int n, int H, int W,
                              void* stream) {
    if (!tiles || !out || n < 0 || H < 1 || W < 1 || is_u8 < 0 || is_u8 > 1) return MIL_ERR_ARG;
    if (!(noise_level >= 0.f) || !(alpha == alpha)) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    const unsigned long long hw = (unsigned long long)H * W, total = 3ull * n * hw;
    const unsigned long long blocks = ((total + 3) / 4 + PA_THREADS - 1) / PA_THREADS;
    if (hw > 0x7fffffffull || blocks > INT_MAX) return MIL_ERR_UNSUPPORTED;
    const uintptr_t pt = reinterpret_cast<uintptr_t>(tiles), po = reinterpret_cast<uintptr_t>(out);
    const int vec = !(po & 15) && !(pt & (is_u8 ? 3 : 15));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    if (is_u8)
        hipLaunchKernelGGL(path_point_kernel<true>, dim3((unsigned)blocks), dim3(PA_THREADS), 0, st, tiles, out, base0, base1, base2, alpha,
                           noise_level, range, k0, k1, sample, total, (unsigned)hw, vec);
    else
        hipLaunchKernelGGL(path_point_kernel<false>, dim3((unsigned)blocks), dim3(PA_THREADS), 0, st, tiles, out, base0, base1, base2, alpha,
                           noise_level, range, k0, k1, sample, total, (unsigned)hw, vec);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_attr_finish(const float* acc, const void* tiles, int is_u8, float base0, float base1, float base2, float* attr,
                               float* map, int map_mode, float* tile_sum, float* ws, int n, int H, int W, void* stream) {
    if (!acc || (!attr && !map && !tile_sum) || n < 0 || H < 1 || W < 1 || is_u8 < 0 || is_u8 > 1) return MIL_ERR_ARG;
    if (map_mode < 0 || map_mode > 2) return MIL_ERR_ARG;
    if (!tiles && (attr || tile_sum || map_mode != 2)) return MIL_ERR_ARG;         // only the map of the gradient itself reads no tiles
    if (tile_sum && !ws) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    const unsigned long long hw = (unsigned long long)H * W;
    if (3 * hw > 0x7fffffffull || n > INT_MAX / MIL_ATTR_SLICES) return MIL_ERR_UNSUPPORTED;
    const int per = (int)((((hw + MIL_ATTR_SLICES - 1) / MIL_ATTR_SLICES) + 3) & ~3ull);
    uintptr_t grid16 = reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(attr) | reinterpret_cast<uintptr_t>(map);
    if (!is_u8) grid16 |= reinterpret_cast<uintptr_t>(tiles);
    const int vec = !(hw & 3) && !(grid16 & 15) && !(is_u8 && (reinterpret_cast<uintptr_t>(tiles) & 3));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* part = tile_sum ? ws : nullptr;
    const dim3 grid((unsigned)n * MIL_ATTR_SLICES);
    if (is_u8)
        hipLaunchKernelGGL(attr_finish_kernel<true>, grid, dim3(PA_THREADS), 0, st, acc, tiles, base0, base1, base2, attr, map, map_mode, part,
                           (int)hw, per, vec);
    else
        hipLaunchKernelGGL(attr_finish_kernel<false>, grid, dim3(PA_THREADS), 0, st, acc, tiles, base0, base1, base2, attr, map, map_mode, part,
                           (int)hw, per, vec);
    MIL_CHECK_LAUNCH();
    if (tile_sum) {
        launch_slice_sum<MIL_ATTR_SLICES>(st, ws, tile_sum, n, SumItself{});
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}
