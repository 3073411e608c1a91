// The fixed-order sum of a tile in slices, shared by feature_vis.hip, feature_inv.hip and path_attr.hip: the ONE summation tree
// include/mil_hip.h promises for objective, energy, loss, terms and tile_sum (tests/slice_sum_reference.py restates it).
//
//   first pass    workgroup t * SLICES + s of 256 threads owns the work items [s per, (s + 1) per) of tile t (slice_range); a
//                 thread adds its items' terms in work-item order, the wave's 64 lanes by a butterfly (wave_sum), the four waves
//                 in order (waves_put / waves_get, or block_sum for all three), and thread 0 writes the slice's partial sum
//   second pass   slice_sum_kernel<SLICES, EPILOGUE>: one thread per row adds the row's SLICES partial sums in slice order and
//                 applies the entry's last operation
// Every addition is an rn_add and every product an rn_mul of rounded.cuh (no fused multiply-add); no atomics, no LDS beyond the
// kernels' own four words per sum: the same bits whatever the grid does.
#pragma once
#include "common.cuh"
#include "rounded.cuh"
#include <climits>

#define SLICE_THREADS 256
// include/mil_hip.h states these for the callers, _lib.py for Python: partial sums per tile ...
#define MIL_SEED_SLICES 16              // ... of mil_stage_seed, mil_stage_energy and mil_stage_match
#define MIL_REG_SLICES 16               // ... and norm of mil_pixel_reg (also the run length of mil_pixel_shift)
#define MIL_ATTR_SLICES 32              // ... of mil_attr_finish

// Which tile and slice this workgroup is, and its run [lo, hi) of the tile's `count` work items at `per` items a slice.
// CLAMP_LO: lo is held to count, so hi - lo is never negative; without it an empty trailing slice has lo > hi = count.
struct SliceRange { size_t t; int s, lo, hi; };
template <int SLICES, bool CLAMP_LO>
__device__ __forceinline__ SliceRange slice_range(int count, int per) {
    SliceRange r;
    r.s = blockIdx.x % SLICES;
    r.t = blockIdx.x / SLICES;
    r.lo = !CLAMP_LO || r.s * per < count ? r.s * per : count;
    r.hi = r.lo + per < count ? r.lo + per : count;
    return r;
}

// The butterfly over a wave's 64 lanes: every lane ends with the same sum, in one order whatever the grid does.
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s = rn_add(s, __shfl_xor(s, d));
    return s;
}

// The four waves' sums through red, the kernel's own `__shared__ float [4]` (MIL_POISON_STATIC'd there, at kernel entry), in two
// halves around the caller's barrier.  waves_put: each wave's first lane stores the wave's sum; waves_get, behind
// __syncthreads(): ((w0 + w1) + w2) + w3.
__device__ __forceinline__ void waves_put(float wave, float* red) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave;
}
__device__ __forceinline__ float waves_get(const float* red) { return rn_add(rn_add(rn_add(red[0], red[1]), red[2]), red[3]); }

// One sum per workgroup: every thread hands in its own, thread 0 writes the workgroup's to *out.
__device__ __forceinline__ void block_sum(float sum, float* red, float* out) {
    waves_put(wave_sum(sum), red);
    __syncthreads();
    if (threadIdx.x == 0) *out = waves_get(red);
}

// What the second pass does with row r's sum s: nothing, the mean s / count, or weight * (s / energy[r]).
struct SumItself { __device__ float operator()(float s, int) const { return s; } };
struct SumOverCount { float count; __device__ float operator()(float s, int) const { return __fdiv_rn(s, count); } };
struct SumWeightedRatio {
    const float* energy;
    float weight;
    __device__ float operator()(float s, int r) const { return rn_mul(weight, __fdiv_rn(s, energy[r])); }
};

template <int SLICES, typename EPILOGUE>
__global__ __launch_bounds__(SLICE_THREADS) void slice_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int rows, EPILOGUE fin) {
    const int r = blockIdx.x * SLICE_THREADS + threadIdx.x;
    if (r >= rows) return;
    float s = 0.f;
    for (int k = 0; k < SLICES; ++k) s = rn_add(s, part[(size_t)r * SLICES + k]);
    out[r] = fin(s, r);
}

template <int SLICES, typename EPILOGUE>
static void launch_slice_sum(hipStream_t st, const float* part, float* out, int rows, EPILOGUE fin) {
    hipLaunchKernelGGL((slice_sum_kernel<SLICES, EPILOGUE>), dim3((rows + SLICE_THREADS - 1) / SLICE_THREADS), dim3(SLICE_THREADS), 0, st, part, out,
                       rows, fin);
}

// What the stage entries (mil_stage_seed / _energy / _match) share: MIL_OK when [n,h,w,cp] with c real channels is a shape
// their kernels take.
static int stage_shape(int n, int h, int w, int cp, int c, int dtype) {
    if (n < 0 || h < 1 || w < 1 || cp < 8 || (cp & 7) || c < 1 || c > cp) return MIL_ERR_ARG;
    if (dtype != MIL_DT_BF16 && dtype != MIL_DT_F32) return MIL_ERR_ARG;
    const unsigned long long hw = (unsigned long long)h * w;
    if (n > 0 && (hw >= (1ull << 24) || hw * (unsigned long long)cp > 0x7fffffffull || n > INT_MAX / MIL_SEED_SLICES)) return MIL_ERR_UNSUPPORTED;
    return MIL_OK;
}
