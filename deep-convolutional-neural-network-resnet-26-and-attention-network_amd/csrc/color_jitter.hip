// Colour jitter on the device: the line the reference's train chain keeps commented out,
//     transforms.ColorJitter(brightness=0.2, contrast=0.1, saturation=0.05, hue=0.02)                    (RoiBuilder.py:200)
// as torchvision's PIL backend computes it, on the resized uint8 tiles [T,3,R,R] (planar) that mil_tile_preprocess*_u8 write,
// in place, bit for bit Pillow's bytes.  Per tile: an order of up to four ops (ColorJitter.forward's fn_idx) and their factors.
//     blend(d, x, a) = d + a * (x - d) in float32, a rounded multiply THEN a rounded add (libImaging/Blend.c); truncated when
//                      0 <= a <= 1, else 0 where <= 0, 255 where >= 255, truncated between
//     L(pixel)       = (19595 R + 38470 G + 7471 B + 0x8000) >> 16                                       (convert("L"))
//     op 0 brightness  blend(0, x, fb)                                                          (ImageEnhance.Brightness)
//     op 1 contrast    blend(m, x, fc), m = int(ImageStat.Stat(L).mean[0] + 0.5) = (2 sum L + n) / (2n) of the tile AS IT IS
//                      WHEN THE OP IS REACHED (n = R * R; the integer form is exact)               (ImageEnhance.Contrast)
//     op 2 saturation  blend(L(pixel), x, fs)                                                        (ImageEnhance.Color)
//     op 3 hue         convert("HSV"), h = (h + shift) mod 256, convert("RGB") — lossy also at shift 0       (adjust_hue)
// rgb2hsv / hsv2rgb are Pillow's (libImaging/Convert.c) with its number formats: float32 rc / gc / bc / s / h / f / fs, double
// expressions between them.  NO CONTRACTION anywhere in this file (the pragma below): an FMA in blend or in hsv2rgb changes
// bytes.  Divisions are IEEE divisions (correctly rounded).  fmod(x, 1.0) of rgb2hsv is x - 1 for 1 <= x < 2 (exact).
//
// Layout of the work.  Everything is pointwise except contrast's mean, which needs sum L of the tile after the ops ordered
// before contrast.  Two launches over (tile, chunk of CJ_PIX pixels), so that a bag of twenty tiles still covers the chip and
// nothing waits on another workgroup inside a launch:
//   pass A (color_jitter_kernel<true>)   tiles whose order holds contrast: the ops before it in registers, sum L per thread,
//       wave shuffle, four partials in LDS, ONE 32-bit vector atomic per workgroup into lsum[t] (zeroed by the entry point on
//       the same stream; 255 n < 2^32 for R <= 4096).  Tiles without contrast return at once.
//   pass B (color_jitter_kernel<false>)  re-reads the original bytes, applies the whole chain with m from lsum[t], stores.
// Integer sums: the result does not depend on the order of the atomics.
//
// A thread takes groups of four neighbouring pixels of a plane.  The planes of a tile start at ANY byte alignment (R * R odd):
// a whole group is one 4-byte access per plane at that alignment (global memory takes unaligned dwords), the last, partial
// group of a plane is read and written byte by byte — no access leaves the tile's plane.
#include "common.cuh"

#pragma clang fp contract(off)

#define CJ_THREADS 256
#define CJ_GROUPS 4                                     // groups of four pixels per thread
#define CJ_PIX (CJ_THREADS * 4 * CJ_GROUPS)             // pixels per workgroup
#define CJ_MAX_R 4096

struct JitterArgs {
    uint8_t* tiles;                 // [T,3,R,R] of this launch
    const int* order;               // [T,4] op codes 0..3, anything else = skip
    const float* factors;           // [T,3] fb, fc, fs
    const int* shift;               // [T]
    unsigned* lsum;                 // [T]
    int n;                          // R * R
};

__device__ __forceinline__ int cj_blend(int d, int x, float a, bool inside) {
    const float prod = a * (float)(x - d);
    const float t = (float)d + prod;
    if (inside) return (int)t;
    return !(t > 0.0f) ? 0 : t >= 255.0f ? 255 : (int)t;
}

__device__ __forceinline__ int cj_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int cj_clip8(int v) { return min(max(v, 0), 255); }

// Pillow's rgb2hsv_row followed by the shift of h and hsv2rgb_row
__device__ __forceinline__ void cj_hue(int& r, int& g, int& b, int shift) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int h = 0, s = 0;
    const int v = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float sf = cr / (float)mx;
        const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
        float hf;
        if (r == mx) hf = bc - gc;
        else if (g == mx) hf = (float)(2.0 + (double)rc - (double)bc);
        else hf = (float)(4.0 + (double)gc - (double)rc);
        double x = (double)hf / 6.0 + 1.0;                              // in [5/6, 11/6]
        x = x >= 1.0 ? x - 1.0 : x;                                     // fmod(x, 1.0)
        const float h32 = (float)x;
        h = cj_clip8((int)((double)h32 * 255.0));
        s = cj_clip8((int)((double)sf * 255.0));
    }
    h = (h + shift) & 255;
    if (s == 0) { r = g = b = v; return; }
    const double hh = (double)h * 6.0 / 255.0;
    const int i = (int)hh;                                              // floor: hh >= 0
    const double f = (double)(float)(hh - (double)i);
    const double fs = (double)(float)((double)s / 255.0);
    const double dv = (double)v;
    const double fsf = fs * f, fsg = fs * (1.0 - f);
    const int p = cj_clip8((int)__builtin_round(dv * (1.0 - fs)));
    const int q = cj_clip8((int)__builtin_round(dv * (1.0 - fsf)));
    const int t = cj_clip8((int)__builtin_round(dv * (1.0 - fsg)));
    const int k = i % 6;                                                // h = 255: i = 6, case 0 with f = 0
    r = (k == 0 || k == 5) ? v : k == 1 ? q : k == 4 ? t : p;
    g = (k == 1 || k == 2) ? v : k == 0 ? t : k == 3 ? q : p;
    b = (k == 3 || k == 4) ? v : k == 2 ? t : k == 5 ? q : p;
}

template <bool SUM>
__global__ __launch_bounds__(CJ_THREADS) void color_jitter_kernel(JitterArgs a) {
    const int tid = threadIdx.x, t = blockIdx.y, n = a.n;
    const int* const ord = a.order + 4 * (size_t)t;
    // pass A applies the ops before contrast and stops there; a tile without contrast has nothing to sum
    int nops = 4, cpos = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k) if (ord[k] == 1) cpos = k;
    if (SUM) {
        if (cpos < 0) return;
        nops = cpos;
    }
    const float fb = a.factors[3 * (size_t)t], fc = a.factors[3 * (size_t)t + 1], fs = a.factors[3 * (size_t)t + 2];
    const bool in_b = fb >= 0.0f && fb <= 1.0f, in_c = fc >= 0.0f && fc <= 1.0f, in_s = fs >= 0.0f && fs <= 1.0f;
    const int shift = a.shift[t] & 255;
    int m = 0;
    if (!SUM && cpos >= 0) m = (int)((2ull * a.lsum[t] + (unsigned)n) / (2ull * (unsigned)n));

    uint8_t* const pr = a.tiles + (size_t)t * 3 * (size_t)n;
    uint8_t* const pg = pr + n;
    uint8_t* const pb = pg + n;
    const int base = blockIdx.x * CJ_PIX;
    unsigned acc = 0;
    for (int j = 0; j < CJ_GROUPS; ++j) {
        const int i = base + (j * CJ_THREADS + tid) * 4;
        if (i >= n) break;
        const int cnt = min(4, n - i);
        int r[4], g[4], b[4];
        if (cnt == 4) {
            unsigned wr, wg, wb;
            __builtin_memcpy(&wr, pr + i, 4); __builtin_memcpy(&wg, pg + i, 4); __builtin_memcpy(&wb, pb + i, 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) { r[q] = (wr >> (8 * q)) & 255; g[q] = (wg >> (8 * q)) & 255; b[q] = (wb >> (8 * q)) & 255; }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                r[q] = q < cnt ? pr[i + q] : 0; g[q] = q < cnt ? pg[i + q] : 0; b[q] = q < cnt ? pb[i + q] : 0;
            }
        }
#pragma unroll 1
        for (int k = 0; k < nops; ++k) {
            const int op = ord[k];                                      // uniform over the workgroup
            if (op == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { r[q] = cj_blend(0, r[q], fb, in_b); g[q] = cj_blend(0, g[q], fb, in_b); b[q] = cj_blend(0, b[q], fb, in_b); }
            } else if (op == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { r[q] = cj_blend(m, r[q], fc, in_c); g[q] = cj_blend(m, g[q], fc, in_c); b[q] = cj_blend(m, b[q], fc, in_c); }
            } else if (op == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int l = cj_grey(r[q], g[q], b[q]);
                    r[q] = cj_blend(l, r[q], fs, in_s); g[q] = cj_blend(l, g[q], fs, in_s); b[q] = cj_blend(l, b[q], fs, in_s);
                }
            } else if (op == 3) {
#pragma unroll
                for (int q = 0; q < 4; ++q) cj_hue(r[q], g[q], b[q], shift);
            }
        }
        if (SUM) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += q < cnt ? (unsigned)cj_grey(r[q], g[q], b[q]) : 0u;
        } else if (cnt == 4) {
            const unsigned wr = (unsigned)r[0] | ((unsigned)r[1] << 8) | ((unsigned)r[2] << 16) | ((unsigned)r[3] << 24);
            const unsigned wg = (unsigned)g[0] | ((unsigned)g[1] << 8) | ((unsigned)g[2] << 16) | ((unsigned)g[3] << 24);
            const unsigned wb = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
            __builtin_memcpy(pr + i, &wr, 4); __builtin_memcpy(pg + i, &wg, 4); __builtin_memcpy(pb + i, &wb, 4);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < cnt) { pr[i + q] = (uint8_t)r[q]; pg[i + q] = (uint8_t)g[q]; pb[i + q] = (uint8_t)b[q]; }
        }
    }
    if (SUM) {
        __shared__ unsigned red[CJ_THREADS / 64];
        MIL_POISON_STATIC(red);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
        if ((tid & 63) == 0) red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            unsigned v = 0;
#pragma unroll
            for (int w = 0; w < CJ_THREADS / 64; ++w) v += red[w];
            atomicAdd(a.lsum + t, v);
        }
    }
}

// ColorJitter of T planar uint8 tiles in place (RoiBuilder.py:200); include/mil_hip.h has the contract.  Everything that can be
// refused is refused here, on the host, before any GPU call.
extern "C" int mil_color_jitter_u8(uint8_t* tiles, const int32_t* order, const float* factors, const int32_t* hue_shift,
                                   uint32_t* lsum, int T, int R, void* stream) {
    if (!tiles || !order || !factors || !hue_shift || !lsum || T < 0 || R < 1) return MIL_ERR_ARG;
    if (R > CJ_MAX_R) return MIL_ERR_UNSUPPORTED;
    if (T == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(lsum, 0, (size_t)T * sizeof(uint32_t), st) != hipSuccess) return MIL_ERR_LAUNCH;
    JitterArgs a{};
    a.n = R * R;
    const int split = (a.n + CJ_PIX - 1) / CJ_PIX;
    for (int done = 0; done < T; done += 65535) {               // grid.y limit
        const int m = T - done < 65535 ? T - done : 65535;
        a.tiles = tiles + (size_t)done * 3 * (size_t)a.n;
        a.order = order + 4 * (size_t)done;
        a.factors = factors + 3 * (size_t)done;
        a.shift = hue_shift + done;
        a.lsum = lsum + done;
        hipLaunchKernelGGL(color_jitter_kernel<true>, dim3(split, m), dim3(CJ_THREADS), 0, st, a);
        MIL_CHECK_LAUNCH();
        hipLaunchKernelGGL(color_jitter_kernel<false>, dim3(split, m), dim3(CJ_THREADS), 0, st, a);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}
