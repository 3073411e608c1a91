// Data gradient of the stem convolution (Conv2d(3,20,7,2,3), gbm/model.py:24): the link between the un-pooled stem gradient and
// the pixels of the tiles.  The forward runs the 7x7 stride-2 filter as a 4x4 stride-1 filter over the 12 space-to-depth
// channels (mil_stem_s2d, MIL_PACK_STEM), so its data gradient is a 4x4 transposed convolution from dstem [n,H2,W2,24] to those
// 12 channels, stored depth-to-space straight into dx [n,3,H,W]:
//     dxs[r][q][c,dy,dx] = sum_{a,b,co} dstem[r-1+a][q-1+b][co] * W[co][c][5-2a+dy][5-2b+dx]        a, b = 0..3  (a = 3 - ty)
// One implicit GEMM per tile of 16x16 space-to-depth pixels: K = 16 taps x 24 channels = 384 = 12 k-steps of 32, 16 output
// columns (12 real).  The FILTER is the MFMA A operand (rows = s2d channel), the pixels are the B operand, so the accumulator
// of lane l holds pixel column l&15 and rows 4*(l>>4)..+3 = the 2x2 output block (dy,dx) of colour channel c = l>>4: a lane
// stores two float2 (16 lanes = 128 contiguous bytes of an output row), and max_c |dx| is two cross-lane maxima.
// Memory-bound: dstem is read once per tile with its 3-pixel halo (19x19 records, re-read from LDS by the 16 taps), the filter
// fragments (12 KB bf16 / 24 KB) stay in registers over the tiles a workgroup walks, dx / sal are written once.
#include "common.cuh"
#include "pf_common.cuh"
#include <climits>

#define SDG_TS 16                       // tile edge in s2d pixels
#define SDG_HS (SDG_TS + 3)             // with the halo: one pixel before, two behind
#define SDG_NPIX (SDG_HS * SDG_HS)
#define SDG_KSTEPS 12
#define SDG_CP 24

// The ACC epilogue: the eight row pieces of dx this lane owns (rows 2 (r0 + m) + dy of colour channel g, columns 2 q, 2 q + 1):
// all loads first (they overlap), then dx = dx + scale * acc as a product and a sum, and the stores.
__device__ __forceinline__ void sdg_acc_store(float* __restrict__ dx, const f32x4_t (&acc)[4], float scale, int img, int g, int q, int r0,
                                              int H, int W, int H2, int W2, bool w_even) {
#pragma clang fp contract(off)          // (HIP's __fmul_rn / __fadd_rn are plain operators that contract into an fma)
    const int x = 2 * q;
    const bool two = x + 1 < W;
    float old[4][2][2];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = r0 + m;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * r + dy;
            old[m][dy][0] = old[m][dy][1] = 0.f;
            if (g >= 3 || r >= H2 || q >= W2 || y >= H || x >= W) continue;
            const float* o = dx + (((size_t)img * 3 + g) * H + y) * W + x;
            if (two && w_even) {
                const f32x2_t v = *reinterpret_cast<const f32x2_t*>(o);
                old[m][dy][0] = v[0]; old[m][dy][1] = v[1];
            } else {
                old[m][dy][0] = o[0];
                if (two) old[m][dy][1] = o[1];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = r0 + m;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * r + dy;
            if (g >= 3 || r >= H2 || q >= W2 || y >= H || x >= W) continue;
            float* o = dx + (((size_t)img * 3 + g) * H + y) * W + x;
            const float v0 = old[m][dy][0] + scale * acc[m][2 * dy];
            const float v1 = old[m][dy][1] + scale * acc[m][2 * dy + 1];
            if (two && w_even) *reinterpret_cast<f32x2_t*>(o) = f32x2_t{v0, v1};
            else { o[0] = v0; if (two) o[1] = v1; }
        }
    }
}

// The GATED epilogue (mil_stem_dgrad_gated: guided Grad-CAM): the same eight row pieces, each element
// multiplied by its pixel's gate byte / 255 — one correctly rounded division and one product, contraction off — and stored.
// The byte is the same for the three colour channels; a lane reads the two bytes of its two columns.
__device__ __forceinline__ void sdg_gated_store(float* __restrict__ dx, const uint8_t* __restrict__ gate, const f32x4_t (&acc)[4], int img,
                                                int g, int q, int r0, int H, int W, int H2, int W2, bool w_even) {
#pragma clang fp contract(off)
    const int x = 2 * q;
    const bool two = x + 1 < W;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = r0 + m;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * r + dy;
            if (g >= 3 || r >= H2 || q >= W2 || y >= H || x >= W) continue;
            const uint8_t* gp = gate + ((size_t)img * H + y) * W + x;
            const float s0 = (float)gp[0] / 255.f;
            const float s1 = two ? (float)gp[1] / 255.f : 0.f;
            float* o = dx + (((size_t)img * 3 + g) * H + y) * W + x;
            const float v0 = acc[m][2 * dy] * s0;
            const float v1 = acc[m][2 * dy + 1] * s1;
            if (two && w_even) *reinterpret_cast<f32x2_t*>(o) = f32x2_t{v0, v1};
            else { o[0] = v0; if (two) o[1] = v1; }
        }
    }
}

// bf16: three workgroups per CU (146 VGPRs, no spill; four would spill 35).  The fp32 forms hold 96 registers of filter
// fragments and run one workgroup per SIMD set (252-254 VGPRs, no spill).
// ACC (mil_stem_dgrad_acc: the inner step of integrated gradients and SmoothGrad): dx is a running sum
// and the store epilogue is dx = dx + scale * (this launch's gradient), a product and a sum with contraction off; no
// `reduce` form.  An output element belongs to one workgroup and one lane, so the read-modify-write needs no atomics.  The
// ACC = false instantiations compile to the code they were before the parameter existed (`scale` is never read there).
// EPI: the store epilogue, a third one beside those two — SDG_PLAIN (dx / sal), SDG_ACC, SDG_GATED (mil_stem_dgrad_gated: `gate`
// [n,H,W] uint8, no `reduce` form).  The loop is one function; stem_dgrad_kernel<T, ACC> keeps its name and its arguments and
// compiles to the code it was (`gate` is never read there).
enum { SDG_PLAIN = 0, SDG_ACC = 1, SDG_GATED = 2 };
template <typename T, int EPI>
__device__ __forceinline__ void stem_dgrad_body(const typename T::elem* dstem, const void* wpack,
                                                float* dx, float* sal, const uint8_t* gate, int H, int W,
                                                int H2, int W2, int tiles_x, int tiles_y, int ntiles, int reduce, float scale) {
    constexpr int ESZ = T::ESZ;
    constexpr int REC = SDG_CP * ESZ;                       // bytes of a pixel record in HBM (and of its LDS image)
    constexpr int PITCH = mil_pix_pitch(SDG_CP, ESZ);       // 48 (bf16) / 112 bytes
    constexpr int PP = REC / 16;                            // 16-byte pieces per record: 3 / 6
    constexpr int NPIECE = SDG_NPIX * PP;
    constexpr int NIT = (NPIECE + 255) / 256;
    constexpr int FRAGB = T::DT == MIL_DT_BF16 ? 16 : 32;
    __shared__ __attribute__((aligned(16))) char lds[SDG_NPIX * PITCH];
    MIL_POISON_STATIC(lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;

    // filter fragments: [kstep][64 lanes][8], this lane's piece of every k-step
    Frag8<T> wf[SDG_KSTEPS];
#pragma unroll
    for (int s = 0; s < SDG_KSTEPS; ++s) wf[s] = lds_frag<T>(static_cast<const char*>(wpack) + ((size_t)s * 64 + lane) * FRAGB);
    // LDS offset of this lane's pixel fragment of k-step s, relative to halo pixel (row of the output pixel, its column):
    // k-group q = 4s + g = tap * 3 + cg, tap = a * 4 + b reads halo pixel (+a, +b)
    int foff[SDG_KSTEPS];
#pragma unroll
    for (int s = 0; s < SDG_KSTEPS; ++s) {
        const int q = 4 * s + g, tap = q / 3, cg = q - 3 * tap;
        foff[s] = ((tap >> 2) * SDG_HS + (tap & 3)) * PITCH + cg * T::CGB;
    }
    // this thread's pieces of the halo: piece id = tid + 256 i -> (halo pixel id / PP, piece id % PP)
    const size_t img_bytes = (size_t)H2 * W2 * REC;         // < 2^31 (checked on the host)
    u32x4_t rz[NIT];
    auto fetch = [&](int t) {
        const int tx = t % tiles_x, r = t / tiles_x;
        const int ty = r % tiles_y, img = r / tiles_y;
        const __amdgpu_buffer_rsrc_t rs = mil_rsrc(reinterpret_cast<const char*>(dstem) + (size_t)img * img_bytes, (unsigned)img_bytes);
        const int gy0 = ty * SDG_TS - 1, gx0 = tx * SDG_TS - 1;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int id = tid + 256 * i;
            const int pix = id / PP, piece = id - pix * PP;
            const int hy = pix / SDG_HS, hx = pix - hy * SDG_HS;
            const int gy = gy0 + hy, gx = gx0 + hx;
            const bool ok = id < NPIECE && gy >= 0 && gy < H2 && gx >= 0 && gx < W2;
            rz[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? (unsigned)((gy * W2 + gx) * REC + piece * 16) : MIL_OOB, 0, 0);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int id = tid + 256 * i;
            if (id >= NPIECE) continue;
            const int pix = id / PP, piece = id - pix * PP;
            char* rec = lds + pix * PITCH;
            if constexpr (T::SPLIT) {                       // [hi: 24 bf16][lo: 24 bf16]; this piece = channels 4 piece .. +3
                bf16x4_t h, l;
                mil_split4(__builtin_bit_cast(f32x4_t, rz[i]), h, l);
                *reinterpret_cast<bf16x4_t*>(rec + piece * 8) = h;
                *reinterpret_cast<bf16x4_t*>(rec + SDG_CP * 2 + piece * 8) = l;
            } else {
                *reinterpret_cast<u32x4_t*>(rec + piece * 16) = rz[i];
            }
        }
    };

    const bool w_even = (W & 1) == 0;
    int t = blockIdx.x;
    if (t < ntiles) fetch(t);
    for (; t < ntiles; t += gridDim.x) {
        commit();
        __syncthreads();
        const int tn = t + gridDim.x;
        if (tn < ntiles) fetch(tn);                         // in flight behind this tile's matrix work
        const int tx = t % tiles_x, rr = t / tiles_x;
        const int ty = rr % tiles_y, img = rr / tiles_y;
        f32x4_t acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < SDG_KSTEPS; ++s) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const char* p = lds + ((wave * 4 + m) * SDG_HS + col) * PITCH + foff[s];
                acc[m] = mma8(wf[s], lds_pix_frag<T, SDG_CP * 2>(p), acc[m]);
            }
        }
        // depth-to-space store: register j of lane group g is dx[img][c = g][2r + (j >> 1)][2q + (j & 1)]
        const int q = tx * SDG_TS + col;
        if constexpr (EPI == SDG_ACC) {
            sdg_acc_store(dx, acc, scale, img, g, q, ty * SDG_TS + wave * 4, H, W, H2, W2, w_even);
            __syncthreads();
            continue;
        }
        if constexpr (EPI == SDG_GATED) {
            sdg_gated_store(dx, gate, acc, img, g, q, ty * SDG_TS + wave * 4, H, W, H2, W2, w_even);
            __syncthreads();
            continue;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int r = ty * SDG_TS + wave * 4 + m;
            const bool in = r < H2 && q < W2;
            float sv[4];
            if (reduce) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = g < 3 ? fabsf(acc[m][j]) : 0.f;
                    v = fmaxf(v, __shfl_xor(v, 16));
                    v = fmaxf(v, __shfl_xor(v, 32));
                    sv[j] = v;
                }
            }
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int y = 2 * r + dy, x = 2 * q;
                if (!in || y >= H || x >= W) continue;
                const bool two = x + 1 < W;
                if (dx && g < 3) {
                    float* o = dx + (((size_t)img * 3 + g) * H + y) * W + x;
                    if (two && w_even) *reinterpret_cast<f32x2_t*>(o) = f32x2_t{acc[m][2 * dy], acc[m][2 * dy + 1]};
                    else { o[0] = acc[m][2 * dy]; if (two) o[1] = acc[m][2 * dy + 1]; }
                }
                if (reduce && g == 0) {
                    float* o = sal + ((size_t)img * H + y) * W + x;
                    if (two && w_even) *reinterpret_cast<f32x2_t*>(o) = f32x2_t{sv[2 * dy], sv[2 * dy + 1]};
                    else { o[0] = sv[2 * dy]; if (two) o[1] = sv[2 * dy + 1]; }
                }
            }
        }
        __syncthreads();                                    // every wave is done reading this tile's records
    }
}

template <typename T, bool ACC = false>
__global__ __launch_bounds__(256, T::DT == MIL_DT_BF16 ? 3 : 1) void stem_dgrad_kernel(const typename T::elem* __restrict__ dstem, const void* __restrict__ wpack,
                                                         float* __restrict__ dx, float* __restrict__ sal, int H, int W, int H2,
                                                         int W2, int tiles_x, int tiles_y, int ntiles, int reduce, float scale) {
    stem_dgrad_body<T, ACC ? SDG_ACC : SDG_PLAIN>(dstem, wpack, dx, sal, nullptr, H, W, H2, W2, tiles_x, tiles_y, ntiles, reduce, scale);
}

template <typename T>
__global__ __launch_bounds__(256, T::DT == MIL_DT_BF16 ? 3 : 1) void stem_dgrad_gated_kernel(const typename T::elem* __restrict__ dstem, const void* __restrict__ wpack,
                                                         float* __restrict__ dx, const uint8_t* __restrict__ gate, int H, int W, int H2,
                                                         int W2, int tiles_x, int tiles_y, int ntiles) {
    stem_dgrad_body<T, SDG_GATED>(dstem, wpack, dx, nullptr, gate, H, W, H2, W2, tiles_x, tiles_y, ntiles, 0, 0.f);
}

template <typename T, bool ACC = false>
static int launch_stem_dgrad(const void* dstem, const void* wpack, float* dx, float* sal, int n, int H, int W, int reduce,
                             hipStream_t st, float scale = 0.f) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const int tiles_x = (W2 + SDG_TS - 1) / SDG_TS, tiles_y = (H2 + SDG_TS - 1) / SDG_TS;
    const long long ntiles = (long long)n * tiles_x * tiles_y;
    if (ntiles > INT_MAX || (size_t)H2 * W2 * SDG_CP * T::ESZ >= 0x80000000ull) return MIL_ERR_UNSUPPORTED;
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    hipLaunchKernelGGL((stem_dgrad_kernel<T, ACC>), dim3(grid), dim3(256), 0, st, (const typename T::elem*)dstem, wpack, dx, sal, H, W,
                       H2, W2, tiles_x, tiles_y, (int)ntiles, reduce, scale);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_stem_dgrad(const void* dstem, const void* wpack, float* dx_nchw, float* sal, int n, int H, int W, int reduce,
                              int dtype, void* stream) {
    if (!dstem || !wpack || (!dx_nchw && !sal) || reduce < 0 || reduce > 1 || n < 0 || H <= 0 || W <= 0) return MIL_ERR_ARG;
    if ((reduce && !sal) || (!reduce && !dx_nchw)) return MIL_ERR_ARG;
    if (dtype != MIL_DT_BF16 && dtype != MIL_DT_F32 && dtype != MIL_DT_F32S) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIL_DT_BF16) return launch_stem_dgrad<BF16>(dstem, wpack, dx_nchw, sal, n, H, W, reduce, st);
    if (dtype == MIL_DT_F32) return launch_stem_dgrad<F32>(dstem, wpack, dx_nchw, sal, n, H, W, reduce, st);
    return launch_stem_dgrad<F32S>(dstem, wpack, dx_nchw, sal, n, H, W, reduce, st);
}

// acc_nchw [n,3,H,W] fp32 += scale * dx, dx what mil_stem_dgrad(reduce = 0) writes for the same arguments: include/mil_hip.h.
extern "C" int mil_stem_dgrad_acc(const void* dstem, const void* wpack, float* acc_nchw, float scale, int n, int H, int W, int dtype,
                                  void* stream) {
    if (!dstem || !wpack || !acc_nchw || n < 0 || H <= 0 || W <= 0) return MIL_ERR_ARG;
    if (dtype != MIL_DT_BF16 && dtype != MIL_DT_F32 && dtype != MIL_DT_F32S) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIL_DT_BF16) return launch_stem_dgrad<BF16, true>(dstem, wpack, acc_nchw, nullptr, n, H, W, 0, st, scale);
    if (dtype == MIL_DT_F32) return launch_stem_dgrad<F32, true>(dstem, wpack, acc_nchw, nullptr, n, H, W, 0, st, scale);
    return launch_stem_dgrad<F32S, true>(dstem, wpack, acc_nchw, nullptr, n, H, W, 0, st, scale);
}

template <typename T>
static int launch_stem_dgrad_gated(const void* dstem, const void* wpack, const uint8_t* gate, float* dx, int n, int H, int W, hipStream_t st) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const int tiles_x = (W2 + SDG_TS - 1) / SDG_TS, tiles_y = (H2 + SDG_TS - 1) / SDG_TS;
    const long long ntiles = (long long)n * tiles_x * tiles_y;
    if (ntiles > INT_MAX || (size_t)H2 * W2 * SDG_CP * T::ESZ >= 0x80000000ull) return MIL_ERR_UNSUPPORTED;
    const int grid = (int)(ntiles < 2048 ? ntiles : 2048);
    hipLaunchKernelGGL((stem_dgrad_gated_kernel<T>), dim3(grid), dim3(256), 0, st, (const typename T::elem*)dstem, wpack, dx, gate, H, W,
                       H2, W2, tiles_x, tiles_y, (int)ntiles);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// dx_nchw [n,3,H,W] fp32 = dx * (gate / 255), dx what mil_stem_dgrad(reduce = 0) writes for the same arguments: include/mil_hip.h.
extern "C" int mil_stem_dgrad_gated(const void* dstem, const void* wpack, const uint8_t* gate, float* dx_nchw, int n, int H, int W,
                                    int dtype, void* stream) {
    if (!dstem || !wpack || !gate || !dx_nchw || n < 0 || H <= 0 || W <= 0) return MIL_ERR_ARG;
    if (dtype != MIL_DT_BF16 && dtype != MIL_DT_F32 && dtype != MIL_DT_F32S) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIL_DT_BF16) return launch_stem_dgrad_gated<BF16>(dstem, wpack, gate, dx_nchw, n, H, W, st);
    if (dtype == MIL_DT_F32) return launch_stem_dgrad_gated<F32>(dstem, wpack, gate, dx_nchw, n, H, W, st);
    return launch_stem_dgrad_gated<F32S>(dstem, wpack, gate, dx_nchw, n, H, W, st);
}
