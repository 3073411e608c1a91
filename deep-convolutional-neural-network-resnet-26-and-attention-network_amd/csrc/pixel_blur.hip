// A separable symmetric filter over a stack of fp32 planes, both passes in one launch: the Gaussian blur of the pixel optimisers
// (the image every few steps, the gradient every step) and of attribution maps; DESIGN.md section 3.47.
//
//   pixel_blur_kernel    a workgroup owns one 64 x 64 output tile of one plane: it stages the tile with its halo into LDS through
//                        the edge index map, writes the horizontal pass of the tile's rows and of the vertical halo rows into a
//                        second LDS array, and after ONE barrier writes the vertical pass to global memory
//
// The arithmetic contract (include/mil_hip.h): acc = w[0] * v[0], then for k = 1 .. radius acc = acc + w[k] * (v[-k] + v[+k]) —
// the pair's sum, the product, the accumulation, each a single correctly rounded fp32 operation — along W first, rounded to fp32,
// then along H.  No atomics; the edge rule is a run-time switch of the staging phase only, the two filter loops never see it.
//
// LDS, for radius R and Rp = R rounded up to 4:  hp [64 + 2R][68] fp32, then st [64 + 2R][64 + 2 Rp + 1] fp32 — 63360 bytes at
// R = 16 (two workgroups per CU of 160 KB), 40608 at R = 4.  A work item of either pass owns a run of consecutive outputs along
// the filter axis and keeps a window of as many samples on each side in registers, moved by one sample per tap (pb_run), so that
// a pass costs (run + 2R) / run LDS reads per output and not 2R + 1:
//   staging     8 lanes take 8 consecutive quads of one row, the next 8 lanes the next row: 16-byte global loads where the quad
//               lies inside the plane on the 16-byte grid, element by element through the index map otherwise; the odd pitch of
//               st sends the 32 lanes of a ds_write_b32 group to 32 banks
//   horizontal  lane <-> row, 8 consecutive columns per item: ds_read_b32 at the odd pitch, one bank per lane; two ds_write_b128
//   vertical    lane <-> 4 consecutive columns, 4 rows per item: ds_read_b128 of consecutive 16-byte slots; 16-byte stores where
//               the four lie inside the plane on the 16-byte grid
#include "common.cuh"
#include "rounded.cuh"
#include <climits>

#define PB_THREADS 256
#define PB_TILE 64
#define PB_HP_PITCH (PB_TILE + 4)       // floats: rows stay on the 16-byte grid, consecutive rows on consecutive 16-byte slots
#ifndef MIL_BLUR_MAX_RADIUS
#define MIL_BLUR_MAX_RADIUS 16          // include/mil_hip.h
#endif

// The source index of sample i of a line of n under the edge rule (0 reflect, 1 replicate, 2 wrap).  The final clamp changes
// nothing inside the halo the rule is defined for; it keeps the padding cells of the staged tile, which no output reads, in bounds.
__device__ __forceinline__ int pb_src(int i, int n, int edge) {
    if (edge == 0) {
        if (i < 0) i = -i;
        if (i > n - 1) i = 2 * (n - 1) - i;
    } else if (edge == 2) {
        i %= n;
        if (i < 0) i += n;
    }
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

template <int V>
__device__ __forceinline__ void pb_ld(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4_t r = *reinterpret_cast<const f32x4_t*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e];
    } else {
        v[0] = p[0];
    }
}

// SEG consecutive outputs along the filter axis (samples `pitch` floats apart in LDS, the first output's own sample at p) of V
// adjacent lines.  lo / hi hold, at tap k, the samples m - k and m + k of the SEG outputs in slot (index mod SEG): tap k reads one
// new sample on each side into the slot that tap k - 1 used last.  Every index is a constant once the loops are unrolled.
template <int SEG, int V>
__device__ __forceinline__ void pb_run(const float* p, int pitch, const float (&w)[MIL_BLUR_MAX_RADIUS + 1], int R, float (&acc)[SEG][V]) {
    float lo[SEG][V], hi[SEG][V];
#pragma unroll
    for (int m = 0; m < SEG; ++m) {
        pb_ld<V>(p + m * pitch, lo[m]);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            hi[m][e] = lo[m][e];
            acc[m][e] = rn_mul(w[0], lo[m][e]);
        }
    }
#pragma unroll
    for (int k = 1; k <= MIL_BLUR_MAX_RADIUS; ++k) {
        if (k <= R) {
            pb_ld<V>(p - k * pitch, lo[((SEG - k) % SEG + SEG) % SEG]);
            pb_ld<V>(p + (SEG - 1 + k) * pitch, hi[(SEG - 1 + k) % SEG]);
#pragma unroll
            for (int m = 0; m < SEG; ++m)
#pragma unroll
                for (int e = 0; e < V; ++e)
                    acc[m][e] = rn_add(acc[m][e], rn_mul(w[k], rn_add(lo[((m - k) % SEG + SEG) % SEG][e], hi[(m + k) % SEG][e])));
        }
    }
}

__global__ __launch_bounds__(PB_THREADS) void pixel_blur_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ taps,
                                                               int H, int W, int tiles_x, int tiles_y, int R, int edge) {
    extern __shared__ __attribute__((aligned(16))) float pb_lds[];
    MIL_POISON(pb_lds);
    const int tid = threadIdx.x;
    const int Rp = (R + 3) & ~3, S = PB_TILE + 2 * Rp + 1;
    float* hp = pb_lds;                                           // [64 + 2R][PB_HP_PITCH]
    float* st = pb_lds + (PB_TILE + 2 * R) * PB_HP_PITCH;         // [64 + 2R][S]
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, plane = b / tiles_y;
    const int x0 = tx * PB_TILE, y0 = ty * PB_TILE;
    const int tw = W - x0 < PB_TILE ? W - x0 : PB_TILE, th = H - y0 < PB_TILE ? H - y0 : PB_TILE;
    const int twp = (tw + 7) & ~7, thp = (th + 3) & ~3;           // whole runs of the two passes
    const int rows = thp + 2 * R, nq = (Rp + twp + R + 3) >> 2;   // staged rows; staged quads per row (4 nq <= S - 1)
    const float* xp = x + (size_t)plane * H * W;
    float* op = out + (size_t)plane * H * W;

    float w[MIL_BLUR_MAX_RADIUS + 1];                             // one read per workgroup, constant indices from here on
#pragma unroll
    for (int k = 0; k <= MIL_BLUR_MAX_RADIUS; ++k) w[k] = taps[k <= R ? k : 0];

    // staged row rr is the plane's row src(y0 - R + rr), staged column lc its column src(x0 - Rp + lc)
    for (int idx = tid; idx < ((nq + 7) >> 3) * rows * 8; idx += PB_THREADS) {
        const int grp = idx >> 3, rr = grp % rows, q = grp / rows * 8 + (idx & 7);
        if (q >= nq) continue;
        const float* rowp = xp + (size_t)pb_src(y0 - R + rr, H, edge) * W;
        const int gx = x0 - Rp + 4 * q;
        float v[4];
        if (gx >= 0 && gx + 3 < W && !(reinterpret_cast<uintptr_t>(rowp + gx) & 15)) {
            pb_ld<4>(rowp + gx, v);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rowp[pb_src(gx + e, W, edge)];
        }
        float* d = st + rr * S + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = v[e];
    }
    __syncthreads();

    // horizontal pass: hp[rr][j] for every staged row and the columns j < twp
    for (int idx = tid; idx < (twp >> 3) * rows; idx += PB_THREADS) {
        const int seg = idx / rows, rr = idx - seg * rows;
        float acc[8][1];
        pb_run<8, 1>(st + rr * S + Rp + seg * 8, 1, w, R, acc);
        f32x4_t* d = reinterpret_cast<f32x4_t*>(hp + rr * PB_HP_PITCH + seg * 8);
        d[0] = f32x4_t{acc[0][0], acc[1][0], acc[2][0], acc[3][0]};
        d[1] = f32x4_t{acc[4][0], acc[5][0], acc[6][0], acc[7][0]};
    }
    __syncthreads();

    // vertical pass over the rounded rows of hp: output row i of the tile has its own sample in hp row R + i
    const int nqc = twp >> 2;
    for (int idx = tid; idx < nqc * (thp >> 2); idx += PB_THREADS) {
        const int rs = idx / nqc, qc = idx - rs * nqc;
        float acc[4][4];
        pb_run<4, 4>(hp + (R + 4 * rs) * PB_HP_PITCH + 4 * qc, PB_HP_PITCH, w, R, acc);
        const int cx = x0 + 4 * qc;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int y = y0 + 4 * rs + m;
            if (y >= H) continue;
            float* d = op + (size_t)y * W + cx;
            if (cx + 3 < W && !(reinterpret_cast<uintptr_t>(d) & 15)) {
                *reinterpret_cast<f32x4_t*>(d) = f32x4_t{acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (cx + e < W) d[e] = acc[m][e];
            }
        }
    }
}

// include/mil_hip.h has the contract.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call.
extern "C" int mil_pixel_blur(const float* x, float* out, const float* taps, int planes, int H, int W, int radius, int edge, void* stream) {
    if (!x || !out || !taps || planes < 0 || H < 1 || W < 1) return MIL_ERR_ARG;
    if (radius < 1 || radius > MIL_BLUR_MAX_RADIUS || edge < 0 || edge > 2) return MIL_ERR_ARG;
    if (edge == 0 && (radius > H - 1 || radius > W - 1)) return MIL_ERR_ARG;
    const unsigned long long hw = (unsigned long long)H * W;
    const unsigned long long tiles = (unsigned long long)((W + PB_TILE - 1) / PB_TILE) * (unsigned long long)((H + PB_TILE - 1) / PB_TILE);
    // a plane as large as the stacks [n,3,H,W] of mil_pixel_shift take, a grid that fits an int
    if (planes > 0 && (3ull * hw > 0x7fffffffull - 3 || tiles * (unsigned long long)planes > (unsigned long long)INT_MAX)) return MIL_ERR_UNSUPPORTED;
    if (mil_overlap(out, x, 4ull * (unsigned long long)planes * hw)) return MIL_ERR_ARG;
    if (planes == 0) return MIL_OK;
    const int tiles_x = (W + PB_TILE - 1) / PB_TILE, tiles_y = (H + PB_TILE - 1) / PB_TILE;
    const int rp = (radius + 3) & ~3;
    const size_t lds = sizeof(float) * (size_t)(PB_TILE + 2 * radius) * (size_t)(PB_HP_PITCH + PB_TILE + 2 * rp + 1);
    hipLaunchKernelGGL(pixel_blur_kernel, dim3((unsigned)(tiles * planes)), dim3(PB_THREADS), lds, reinterpret_cast<hipStream_t>(stream), x, out, taps,
                       H, W, tiles_x, tiles_y, radius, edge);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
