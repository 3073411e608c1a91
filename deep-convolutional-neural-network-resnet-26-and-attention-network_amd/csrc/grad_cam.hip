// Grad-CAM per tile (gradcam.py:75-89 of the reference's vendored pytorch-cnn-visualizations-master/src): from the output of a
// convolutional stage, act [n,h,w,cs], and the gradient of the class evidence with respect to it, grad [n,h,w,cs] (the padded
// NHWC layouts of DESIGN.md section 2: c real channels of cs stored), to the map the toolkit draws over the tile:
//     w_k      = (sum over the tile's pixels of grad[.,.,k]) / (h w)                          np.mean(guided_gradients, axis=(1, 2))
//     raw[i,j] = max(offset + sum_k w_k act[i,j,k], 0)                                        np.ones + the weighted sum, np.maximum
//     q[i,j]   = (uint8)(((raw - mn) / (mx - mn)) * 255.0f)                                   the min-max normalisation, np.uint8
//     out      = Pillow's Image.fromarray(q).resize((W, H), LANCZOS)                          the antialiased resize to the tile
// One workgroup of 256 threads owns one tile and keeps everything between the two tensors and the bytes in LDS:
//   phase 1  channel sums of grad: thread (plane, piece) walks the pixels plane, plane + G, ... of its 16-byte piece of the pixel
//            record (a wave instruction reads 1 KiB of consecutive bytes), the G partial rows go to LDS and one thread per channel
//            adds them in plane order
//   phase 2  one pixel per thread: the weighted sum over the record's pieces in channel order (pad channels are never multiplied:
//            they may hold anything), ReLU, the fp32 map to LDS (and to `raw`), min / max by wave shuffles and four LDS words
//   phase 3  the quantised map q [h][w] to LDS; after a barrier the horizontal pass writes the strip [h][W] over the fp32 map
//   phase 4  the vertical pass: a thread makes four consecutive bytes of the tile's output and stores them as one dword
// The resampling is Pillow's 8-bit two-pass filter restated (as in preprocess.hip): 22-bit coefficients from the host
// (mil_resample_coeffs, MIL_FILTER_LANCZOS), each pass from 1 << 21, int32 accumulation, arithmetic shift, clamp to a byte; a
// pass whose two sizes are equal is skipped as Pillow skips it.  The division is the correctly rounded one and nothing else in
// the normalisation can be contracted, so q is what numpy's fp32 arithmetic makes of the same map, bit for bit.
// No atomics, no workspace, every sum in a fixed order: bit-repeatable.  By its bytes the kernel would be memory-bound (two reads
// of h w cs elements and H W bytes written per tile against ~2 flops per element), and the launch that stops at `raw` does run
// at 0.26-0.40 of the HBM peak on 64x64 maps; the one that goes on to the bytes does not: its time is the two resampling
// passes, byte reads from LDS by the four waves a tile has (DESIGN.md section 3.36 has the figures).
#include "common.cuh"
#include <climits>

#define GC_BITS 22
#define GC_THREADS 256
#define GC_PART_BYTES (GC_THREADS * 8 * 4)      // phase 1's partial rows: at most 256 pieces of at most 8 channels, fp32

extern "C" int mil_resample_plan(int in_size, int out_size, int filter, int* ksize);

template <typename T> struct GcPiece;
template <> struct GcPiece<BF16> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const __bf16* p, float (&v)[8]) {
        const bf16x8_t r = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
    }
};
template <> struct GcPiece<F32> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const f32x4_t r = *reinterpret_cast<const f32x4_t*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = r[j];
    }
};

__device__ __forceinline__ unsigned gc_clip8(int v) { v >>= GC_BITS; return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// LDS carve (bytes, every offset a multiple of 16): [0, q_off) the partial rows, then the fp32 map, then the strip;
// [q_off, w_off) the quantised map; [w_off, t_off) the channel weights; from t_off the tables xkk, xbounds, ykk, ybounds.
template <typename T>
__global__ __launch_bounds__(GC_THREADS) void grad_cam_kernel(const typename T::elem* __restrict__ act, const typename T::elem* __restrict__ grad,
                                                             int h, int w, int c, int cs, float offset, const float* __restrict__ range,
                                                             const int* __restrict__ ybounds, const int* __restrict__ ykk, int yksize,
                                                             const int* __restrict__ xbounds, const int* __restrict__ xkk, int xksize,
                                                             float* __restrict__ raw, uint8_t* __restrict__ out, int H, int W,
                                                             int q_off, int w_off, int t_off) {
    constexpr int EPP = GcPiece<T>::N;                      // elements of a 16-byte piece
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    MIL_POISON(gsm);
    __shared__ float red[8];                                // per wave: minimum, maximum
    MIL_POISON_STATIC(red);
    float* part = reinterpret_cast<float*>(gsm);
    float* map = reinterpret_cast<float*>(gsm);
    unsigned char* strip = gsm;
    unsigned char* q = gsm + q_off;
    float* wts = reinterpret_cast<float*>(gsm + w_off);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w;
    const size_t t = blockIdx.x;
    const typename T::elem* gt = grad + t * (size_t)hw * cs;
    const typename T::elem* at = act + t * (size_t)hw * cs;

    // ---- phase 1: w_k = mean over the pixels of grad[., ., k] ---------------------------------------------------------------
    const int PP = cs / EPP, G = GC_THREADS / PP;           // pieces per pixel record; pixel planes walked side by side
    if (tid < G * PP) {
        const int plane = tid / PP, piece = tid - plane * PP;
        float acc[EPP];
#pragma unroll
        for (int j = 0; j < EPP; ++j) acc[j] = 0.f;
        for (int pix = plane; pix < hw; pix += G) {
            float v[EPP];
            GcPiece<T>::load(gt + (size_t)pix * cs + piece * EPP, v);
#pragma unroll
            for (int j = 0; j < EPP; ++j) acc[j] += v[j];
        }
#pragma unroll
        for (int j = 0; j < EPP; ++j) part[tid * EPP + j] = acc[j];     // = part[plane][piece * EPP + j]
    }
    __syncthreads();
    for (int k = tid; k < cs; k += GC_THREADS) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += part[g * cs + k];
        wts[k] = s / (float)hw;
    }
    __syncthreads();

    // ---- phase 2: raw = max(offset + sum_k w_k act_k, 0), its minimum and maximum ---------------------------------------------
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int pix = tid; pix < hw; pix += GC_THREADS) {
        float s = offset;
        for (int p = 0; p < PP; ++p) {
            float v[EPP];
            GcPiece<T>::load(at + (size_t)pix * cs + p * EPP, v);
#pragma unroll
            for (int j = 0; j < EPP; ++j) {
                const int k = p * EPP + j;
                if (k < c) s = fmaf(wts[k], v[j], s);
            }
        }
        const float r = fmaxf(s, 0.f);
        map[pix] = r;
        if (raw) raw[t * (size_t)hw + pix] = r;
        mn = fminf(mn, r); mx = fmaxf(mx, r);
    }
    if (!out) return;
    if (range) {
        mn = range[0]; mx = range[1];
    } else {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, d));
            mx = fmaxf(mx, __shfl_xor(mx, d));
        }
        if (lane == 0) { red[wave] = mn; red[4 + wave] = mx; }
    }
    // the tables of the two passes: read once per tile
    int* xk = reinterpret_cast<int*>(gsm + t_off);
    int* xb = xk + W * xksize;
    int* yk = xb + 2 * W;
    int* yb = yk + H * yksize;
    const bool hpass = w != W, vpass = h != H;
    if (hpass) {
        for (int i = tid; i < W * xksize; i += GC_THREADS) xk[i] = xkk[i];
        for (int i = tid; i < 2 * W; i += GC_THREADS) xb[i] = xbounds[i];
    }
    if (vpass) {
        for (int i = tid; i < H * yksize; i += GC_THREADS) yk[i] = ykk[i];
        for (int i = tid; i < 2 * H; i += GC_THREADS) yb[i] = ybounds[i];
    }
    __syncthreads();
    if (!range) {
        mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    }

    // ---- phase 3: the quantised map, then the horizontal pass over it -----------------------------------------------------------
    const float span = mx - mn;
    for (int pix = tid; pix < hw; pix += GC_THREADS) {
        float r = map[pix];
        if (range) r = fminf(fmaxf(r, mn), mx);
        int b = 0;
        if (span != 0.f) b = (int)(__fdiv_rn(r - mn, span) * 255.0f);        // truncation toward zero, as np.uint8
        q[pix] = (unsigned char)(b < 0 ? 0 : (b > 255 ? 255 : b));
    }
    __syncthreads();                                        // the fp32 map is dead: the strip takes its place
    if (hpass) {
        for (int i = tid; i < h * W; i += GC_THREADS) {
            const int y = i / W, X = i - y * W;
            const int xmin = xb[2 * X], cnt = xb[2 * X + 1];
            const unsigned char* p = q + y * w + xmin;
            const int* kw = xk + X * xksize;
            int s = 1 << (GC_BITS - 1);
            for (int k = 0; k < cnt; ++k) s += (int)p[k] * kw[k];
            strip[i] = (unsigned char)gc_clip8(s);
        }
        __syncthreads();
    }

    // ---- phase 4: the vertical pass; four consecutive bytes of the tile's output per thread, one dword store ---------------------
    const unsigned char* src = hpass ? strip : q;           // [h][W] either way
    const int HW = H * W;
    uint8_t* ot = out + t * (size_t)HW;
    const int a0 = (int)(reinterpret_cast<uintptr_t>(ot) & 3);              // the dword grid of the output, not of the tile
    for (int i = tid; i * 4 < a0 + HW; i += GC_THREADS) {
        unsigned b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = 4 * i - a0 + j;
            b[j] = 0u;
            if (f < 0 || f >= HW) continue;
            if (!vpass) { b[j] = src[f]; continue; }
            const int Y = f / W, X = f - Y * W;
            const int ymin = yb[2 * Y], cnt = yb[2 * Y + 1];
            const unsigned char* p = src + ymin * W + X;
            const int* kw = yk + Y * yksize;
            int s = 1 << (GC_BITS - 1);
            for (int k = 0; k < cnt; ++k) s += (int)p[k * W] * kw[k];
            b[j] = gc_clip8(s);
        }
        const int f0 = 4 * i - a0;
        if (f0 >= 0 && f0 + 4 <= HW) {
            *reinterpret_cast<unsigned*>(ot + f0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (f0 + j >= 0 && f0 + j < HW) ot[f0 + j] = (uint8_t)b[j];
        }
    }
}

static int gc_round16(long long v) { return (int)((v + 15) & ~15ll); }

template <typename T>
static int launch_grad_cam(const void* act, const void* grad, int n, int h, int w, int c, int cs, float offset, const float* range,
                           const int32_t* ybounds, const int32_t* ykk, int yksize, const int32_t* xbounds, const int32_t* xkk, int xksize,
                           float* raw, uint8_t* out, int H, int W, hipStream_t st) {
    const long long hw = (long long)h * w;
    if (cs * T::ESZ / 16 > GC_THREADS || hw * cs * T::ESZ >= 0x80000000ll || hw > INT_MAX / 4) return MIL_ERR_UNSUPPORTED;
    long long first = hw * 4 > GC_PART_BYTES ? hw * 4 : GC_PART_BYTES, q_bytes = 0, t_bytes = 0;
    if (out) {
        if ((long long)H * W > INT_MAX / 4) return MIL_ERR_UNSUPPORTED;
        if (w != W && (long long)h * W > first) first = (long long)h * W;
        q_bytes = hw;
        t_bytes = 4ll * ((long long)W * xksize + 2 * W + (long long)H * yksize + 2 * H);
    }
    const long long total = ((first + 15) & ~15ll) + ((q_bytes + 15) & ~15ll) + cs * 4ll + t_bytes;
    if (total > 160 * 1024 - 64) return MIL_ERR_UNSUPPORTED;         // (- the static words)
    const int q_off = gc_round16(first), w_off = q_off + gc_round16(q_bytes), t_off = w_off + cs * 4;
    const int lds = (int)total;
    auto kern = grad_cam_kernel<T>;
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return MIL_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(n), dim3(GC_THREADS), lds, st, (const typename T::elem*)act, (const typename T::elem*)grad, h, w, c, cs,
                       offset, range, ybounds, ykk, yksize, xbounds, xkk, xksize, raw, out, H, W, q_off, w_off, t_off);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// include/mil_hip.h has the contract.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call.
extern "C" int mil_grad_cam(const void* act, const void* grad, int n, int h, int w, int c, int cs, int dtype, float offset,
                            const float* range, const int32_t* ybounds, const int32_t* ykk, int yksize, const int32_t* xbounds,
                            const int32_t* xkk, int xksize, float* raw, uint8_t* out, int H, int W, void* stream) {
    if (!act || !grad || (!raw && !out) || n < 0 || h < 1 || w < 1 || H < 1 || W < 1) return MIL_ERR_ARG;
    if (c < 1 || c > cs || (cs & 7)) return MIL_ERR_ARG;
    if (dtype != MIL_DT_BF16 && dtype != MIL_DT_F32 && dtype != MIL_DT_F32S) return MIL_ERR_ARG;
    if (out) {
        if (!ybounds || !ykk || !xbounds || !xkk) return MIL_ERR_ARG;
        int yks = 0, xks = 0;
        if (mil_resample_plan(h, H, MIL_FILTER_LANCZOS, &yks) != MIL_OK || mil_resample_plan(w, W, MIL_FILTER_LANCZOS, &xks) != MIL_OK) return MIL_ERR_ARG;
        if (yksize != yks || xksize != xks) return MIL_ERR_ARG;
    }
    if (n == 0) return MIL_OK;
    if ((reinterpret_cast<uintptr_t>(act) | reinterpret_cast<uintptr_t>(grad)) & 15) return MIL_ERR_UNSUPPORTED;     // 16-byte loads
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIL_DT_BF16)
        return launch_grad_cam<BF16>(act, grad, n, h, w, c, cs, offset, range, ybounds, ykk, yksize, xbounds, xkk, xksize, raw, out, H, W, st);
    return launch_grad_cam<F32>(act, grad, n, h, w, c, cs, offset, range, ybounds, ykk, yksize, xbounds, xkk, xksize, raw, out, H, W, st);
}
