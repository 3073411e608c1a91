// Slide mosaics of per-tile attribution maps: the uint8 maps or pictures of AttributionRenderer / TileGradCam, resampled into
// the blocks of thumbnail pixels their windows own (mil_heatmap_render's convention), coloured and composited over the tissue
// thumbnail with Pillow's alpha_composite; DESIGN.md section 3.42, include/mil_hip.h states the arithmetic.
//
// Window t owns the n x n block at (out_pos[t][0], out_pos[t][1]).  Owned pixel (a, b) is the area average of the map over its
// footprint [a Hm / n, (a+1) Hm / n) x [b Wm / n, (b+1) Wm / n) in map pixels: on the common grid of n Hm x n Wm sub-pixels
// (a map pixel = n x n of them, an output pixel = Hm x Wm) the weight of map pixel (k, l) is the length of the overlap of
// [a Hm, (a+1) Hm) with [k n, (k+1) n) times that of [b Wm, (b+1) Wm) with [l n, (l+1) n).  Everything is an integer, the sums
// are 32-bit (255 Hm Wm + Hm Wm / 2 < 2^32 for Hm Wm <= 2^24), so any split of a footprint over lanes gives the same bits.
//
//   attr_mosaic_kernel<C, I, false>   one THREAD per owned pixel: it walks its footprint rows and, inside, columns itself; a
//                                     row's weight multiplies the row's sum once.  Neighbouring lanes own neighbouring
//                                     pixels of a block row and read neighbouring map columns.
//   attr_mosaic_kernel<C, I, true>    one WAVE per owned pixel: the 64 lanes stride the footprint row-major (adjacent lanes on
//                                     adjacent map columns), MOSAIC_DEPTH pixels per lane at a time with all loads issued
//                                     first; the partial sums meet in a shuffle butterfly, lane 0 colours, blends and
//                                     stores.  No LDS in either form.
// The host takes the wave form when a footprint holds at least one wave's worth of map pixels:
// ceil(Hm / n) * ceil(Wm / n) >= 64.  I is the type of the sub-pixel coordinates: unsigned where n (max(Hm, Wm) + 1) and the
// owned pixels of a block stay below 2^31, unsigned long long otherwise.
//
// Only the part of a block inside the [Ht, Wt] canvas is visited: at most min(n, Ht) x min(n, Wt) pixels from the first owned
// row and column that are not above or left of the canvas (out_pos is a device array the host cannot check, and may be
// negative).  Each output pixel is read (on_tissue) and written by one thread only.
#include "common.cuh"

#define MOSAIC_THREADS 256
#define MOSAIC_MAX_HW (1 << 24)
#define MOSAIC_WAVE_FOOTPRINT 64            // footprints of this many map pixels and more take the wave-per-pixel form
#define MOSAIC_MAX_GRID_X 65535
#define MOSAIC_DEPTH 8                      // footprint pixels a lane of the wave form loads before it sums them

struct MosaicArgs {
    const uint8_t* maps;            // [T,Hm,Wm,C]
    const int* pos;                 // [T,2] top-left output pixel (row, col) of each window
    const uint8_t* lut;             // [256,3] (C == 1)
    uint8_t* heat;                  // [Ht,Wt,3] or null
    uint8_t* on_tissue;             // [Ht,Wt,3] or null
    int Hm, Wm, n, Ht, Wt, nh, nw;  // nh = min(n, Ht), nw = min(n, Wt): the most rows / columns of a block inside the canvas
    unsigned alpha, by_value;
};

// overlap of [s, e) with [g, g + n): positive for every map pixel the loops below visit
template <typename I>
__device__ __forceinline__ unsigned mosaic_weight(I s, I e, I g, I n) {
    const I hi = e < g + n ? e : g + n, lo = s > g ? s : g;
    return (unsigned)(hi - lo);
}

// colour, blend and store one owned pixel from its weighted sums; dst: the three bytes on_tissue holds there
template <int C>
__device__ __forceinline__ void mosaic_store(const MosaicArgs& a, const unsigned (&sum)[C], const unsigned (&dst)[3], size_t o) {
    const unsigned hw = (unsigned)a.Hm * (unsigned)a.Wm, half = hw / 2u;
    unsigned v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (sum[c] + half) / hw;
    const unsigned A = a.by_value ? (a.alpha * v[0] + 127u) / 255u : a.alpha;
    unsigned src[3];                                                        // all three before the first store (bytes may alias)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (C == 1) src[c] = a.lut[v[0] * 3u + c];
        else src[c] = v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.heat) a.heat[o + c] = (uint8_t)src[c];
        if (a.on_tissue) {
            const unsigned tmp = 64u * (src[c] * A + dst[c] * (255u - A)) + (0x80u << 6);
            a.on_tissue[o + c] = (uint8_t)((((tmp >> 8) + tmp) >> 8) >> 6);
        }
    }
}

template <int C, typename I, bool WAVE>
__global__ __launch_bounds__(MOSAIC_THREADS) void attr_mosaic_kernel(MosaicArgs a) {
    const int t = blockIdx.y;
    const long long oy0 = a.pos[2 * (size_t)t], ox0 = a.pos[2 * (size_t)t + 1];
    const long long alo = oy0 < 0 ? -oy0 : 0, blo = ox0 < 0 ? -ox0 : 0;     // first owned row / column not above / left of the canvas
    const I n = (I)a.n, Hm = (I)a.Hm, Wm = (I)a.Wm, nw = (I)a.nw;
    const I total = (I)a.nh * nw;
    const uint8_t* const map = a.maps + (size_t)t * (size_t)a.Hm * (size_t)a.Wm * C;
    const unsigned lane = threadIdx.x & 63;
    const I first = WAVE ? (I)blockIdx.x * (MOSAIC_THREADS / 64) + (threadIdx.x >> 6) : (I)blockIdx.x * MOSAIC_THREADS + threadIdx.x;
    const I step = (I)gridDim.x * (WAVE ? MOSAIC_THREADS / 64 : MOSAIC_THREADS);
    for (I p = first; p < total; p += step) {                               // (wave form: p is the same in all lanes of a wave)
        const I ar = p / nw, bc = p - ar * nw;
        const long long al = alo + (long long)ar, bl = blo + (long long)bc;
        const long long oy = oy0 + al, ox = ox0 + bl;
        if (al >= a.n || bl >= a.n || oy >= a.Ht || ox >= a.Wt) continue;   // behind the block or the canvas
        const bool writer = !WAVE || lane == 0;
        const size_t o = ((size_t)oy * (size_t)a.Wt + (size_t)ox) * 3;
        unsigned dst[3] = {0u, 0u, 0u};
        if (writer && a.on_tissue) {                                        // on its way while the footprint is summed
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = a.on_tissue[o + c];
        }
        // footprint: map rows from k0 and columns from l0 on, while they start below ye / xe on the sub-pixel grid.  A map holds
        // at most 3 * 2^24 bytes: 32-bit offsets into it
        const I ys = (I)al * Hm, ye = ys + Hm, xs = (I)bl * Wm, xe = xs + Wm;
        const I k0 = ys / n, l0 = xs / n;
        const unsigned wm = (unsigned)a.Wm;
        unsigned sum[C];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = 0u;
        if constexpr (!WAVE) {
            // rows outside, columns inside: a row's weight multiplies the row's sum once
            I ky = k0 * n;
            for (unsigned k = (unsigned)k0; ky < ye; ++k, ky += n) {
                const unsigned wy = mosaic_weight<I>(ys, ye, ky, n);
                unsigned rs[C];
#pragma unroll
                for (int c = 0; c < C; ++c) rs[c] = 0u;
                I lx = l0 * n;
                for (unsigned at = (k * wm + (unsigned)l0) * C; lx < xe; at += C, lx += n) {
                    const unsigned wx = mosaic_weight<I>(xs, xe, lx, n);
#pragma unroll
                    for (int c = 0; c < C; ++c) rs[c] += wx * map[at + c];
                }
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += wy * rs[c];
            }
        } else {
            // the nr x nc <= Hm x Wm <= 2^24 pixels of the footprint row-major, walked with carries: this lane takes pixels
            // lane, lane + 64, ... (adjacent lanes on adjacent map columns), MOSAIC_DEPTH of them at a time with all loads
            // issued before the first is used; one behind the footprint reads the map's first pixel with weight zero
            const unsigned nr = (unsigned)((ye + n - 1) / n - k0), nc = (unsigned)((xe + n - 1) / n - l0);
            const unsigned count = nr * nc;
            unsigned r = lane / nc, q = lane - r * nc;
            const unsigned dr = 64u / nc, dq = 64u - dr * nc;
            for (unsigned i = lane; i < count; i += MOSAIC_DEPTH * 64u) {
                unsigned w[MOSAIC_DEPTH], b[MOSAIC_DEPTH][C];
#pragma unroll
                for (int j = 0; j < MOSAIC_DEPTH; ++j) {
                    const bool live = i + j * 64u < count;
                    const I k = k0 + r, l = l0 + q;
                    w[j] = live ? mosaic_weight<I>(ys, ye, k * n, n) * mosaic_weight<I>(xs, xe, l * n, n) : 0u;
                    const unsigned at = live ? ((unsigned)k * wm + (unsigned)l) * C : 0u;
#pragma unroll
                    for (int c = 0; c < C; ++c) b[j][c] = map[at + c];
                    r += dr; q += dq;
                    if (q >= nc) { q -= nc; ++r; }
                }
#pragma unroll
                for (int j = 0; j < MOSAIC_DEPTH; ++j)
#pragma unroll
                    for (int c = 0; c < C; ++c) sum[c] += w[j] * b[j][c];
            }
        }
        if constexpr (WAVE) {
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) sum[c] += __shfl_xor(sum[c], d);
        }
        if (writer) mosaic_store<C>(a, sum, dst, o);
    }
}

template <int C, typename I>
static void mosaic_launch(bool wave, dim3 grid, hipStream_t st, const MosaicArgs& a) {
    if (wave) hipLaunchKernelGGL((attr_mosaic_kernel<C, I, true>), grid, dim3(MOSAIC_THREADS), 0, st, a);
    else hipLaunchKernelGGL((attr_mosaic_kernel<C, I, false>), grid, dim3(MOSAIC_THREADS), 0, st, a);
}

// include/mil_hip.h has the contract.  Everything that can be refused is refused here, on the host, before any GPU call.
extern "C" int mil_attr_mosaic(const uint8_t* maps, int channels, int T, int Hm, int Wm, int n, const int32_t* out_pos, const uint8_t* lut,
                               int alpha, int alpha_by_value, uint8_t* heat, uint8_t* on_tissue, int Ht, int Wt, void* stream) {
    if (!maps || !out_pos || (!heat && !on_tissue) || (channels != 1 && channels != 3) || (channels == 1 && !lut)) return MIL_ERR_ARG;
    if (alpha < 0 || alpha > 255 || alpha_by_value < 0 || alpha_by_value > 1 || (alpha_by_value && channels == 3)) return MIL_ERR_ARG;
    if (T < 0 || Hm < 1 || Wm < 1 || n < 1 || Ht < 1 || Wt < 1) return MIL_ERR_ARG;
    if ((int64_t)Hm * Wm > MOSAIC_MAX_HW) return MIL_ERR_UNSUPPORTED;
    if (T == 0) return MIL_OK;

    MosaicArgs a{};
    a.lut = lut; a.heat = heat; a.on_tissue = on_tissue;
    a.Hm = Hm; a.Wm = Wm; a.n = n; a.Ht = Ht; a.Wt = Wt;
    a.nh = n < Ht ? n : Ht; a.nw = n < Wt ? n : Wt;
    a.alpha = (unsigned)alpha; a.by_value = (unsigned)alpha_by_value;
    const uint64_t total = (uint64_t)a.nh * (uint64_t)a.nw;
    const uint64_t fy = ((uint64_t)Hm + n - 1) / n, fx = ((uint64_t)Wm + n - 1) / n;
    const bool wave = fy * fx >= MOSAIC_WAVE_FOOTPRINT;
    // 32-bit sub-pixel coordinates reach (a + 1) Hm + n <= n (Hm + 1), and the pixel index total + one grid stride
    const uint64_t side = (uint64_t)(Hm > Wm ? Hm : Wm) + 1;
    const bool wide = (uint64_t)n * side >= 0x80000000ull || total >= 0x80000000ull;
    const uint64_t per_block = wave ? MOSAIC_THREADS / 64 : MOSAIC_THREADS;
    const uint64_t blocks = (total + per_block - 1) / per_block;
    const unsigned gx = (unsigned)(blocks < MOSAIC_MAX_GRID_X ? blocks : MOSAIC_MAX_GRID_X);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int done = 0; done < T; done += 65535) {               // grid.y limit
        const int m = T - done < 65535 ? T - done : 65535;
        a.maps = maps + (size_t)done * (size_t)Hm * (size_t)Wm * channels;
        a.pos = out_pos + 2 * (size_t)done;
        const dim3 grid(gx, m);
        if (channels == 1) {
            if (wide) mosaic_launch<1, unsigned long long>(wave, grid, st, a);
            else mosaic_launch<1, unsigned>(wave, grid, st, a);
        } else {
            if (wide) mosaic_launch<3, unsigned long long>(wave, grid, st, a);
            else mosaic_launch<3, unsigned>(wave, grid, st, a);
        }
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}
