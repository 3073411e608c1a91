// Attribution tensors to the pictures of the reference's vendored saliency toolkit (misc_functions.py of
// pytorch-cnn-visualizations-master/src): convert_to_grayscale, save_gradient_images / format_np_output,
// get_positive_negative_saliency and apply_colormap_on_image; DESIGN.md section 3.41.
//
//   aq_hist_kernel<C>     one digit pass of an exact radix select: digit counts of the keys that carry a group's prefix
//   aq_select_kernel      one workgroup per group: the digit and the remaining rank of BOTH ranks lo and hi; the last pass
//                         turns the two keys, the minimum and the maximum into the group's statistics
//   attr_render_kernel<MODE, C>   gradient or map + statistics -> bytes (grayscale, colour, positive / negative)
//   cam_overlay_kernel    map bytes -> colour table -> Pillow's alpha_composite over the tile
//
// A group is one tile or the whole bag.  The key of an fp32 value is its bit pattern made order preserving (sign bit set for
// the non-negatives, all bits flipped for the negatives; -0.0 counts as +0.0), cut into digits of 11, 11 and 10 bits from the
// top.  A NaN orders by its bits: above +inf with the sign bit clear, below -inf with it set.  All counts are integers and
// are merged with integer atomics, so two calls give the same bits.
#include "common.cuh"
#include "rounded.cuh"
#include <climits>

#define AQ_THREADS 256
#define AQ_BINS 2048
#define AQ_WS_WORDS (2 * AQ_BINS + 8)     // include/mil_hip.h MIL_QUANTILE_WS_WORDS: two digit tables and eight words of state
#define AQ_CHUNK 4096                     // pixels of one tile per histogram workgroup
#define AQ_BAG_TABLES 16                  // include/mil_hip.h MIL_QUANTILE_BAG_TABLES: copies of the bag's tables (tile t adds to copy t % 16)
// state words behind the two tables
#define AQ_PLO 0                          // key prefix of rank lo / of rank hi (the digits fixed so far)
#define AQ_PHI 1
#define AQ_RLO 2                          // rank of lo / of hi among the keys that carry its prefix
#define AQ_RHI 3
#define AQ_MAX 4                          // largest key, and the complement of the smallest (both start at zero)
#define AQ_NMIN 5

__device__ __forceinline__ unsigned aq_key(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float aq_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// convert_to_grayscale's np.sum(np.abs(g), axis=0): (|g0| + |g1|) + |g2|
__device__ __forceinline__ float ar_gray(float g0, float g1, float g2) { return rn_add(rn_add(fabsf(g0), fabsf(g1)), fabsf(g2)); }

// Four consecutive pixels p .. p + 3 (cnt of them inside the tile) of plane `plane`; whole: one aligned 16-byte load.
__device__ __forceinline__ void ar_load4(const float* __restrict__ x, size_t plane, int hw, int p, int cnt, bool whole, float (&v)[4]) {
    const float* src = x + plane * (size_t)hw + p;
    if (whole) {
        const f32x4_t r = *reinterpret_cast<const f32x4_t*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = r[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? src[j] : 0.f;
    }
}

// The values that are ranked: C == 3 the grayscale of a [T,3,hw] gradient, C == 1 a [T,hw] map as it is.
template <int C>
__device__ __forceinline__ void ar_values4(const float* __restrict__ x, size_t t, int hw, int p, int cnt, bool whole, float (&v)[4]) {
    if constexpr (C == 3) {
        float a[4], b[4], c[4];
        ar_load4(x, t * 3, hw, p, cnt, whole, a);
        ar_load4(x, t * 3 + 1, hw, p, cnt, whole, b);
        ar_load4(x, t * 3 + 2, hw, p, cnt, whole, c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ar_gray(a[j], b[j], c[j]);
    } else {
        ar_load4(x, t, hw, p, cnt, whole, v);
    }
}

// Workgroup b: chunk b % chunks of tile b / chunks.  pass 0, 1, 2: the digit is key bits 31..21, 20..10, 9..0 and a key counts
// when the bits above the digit equal the group's prefix — table 0 for the prefix of rank lo, table 1 for that of rank hi when
// the two differ (they share table 0 while they agree).  Pass 0 also takes the minimum and the maximum key.  A tile adds to its
// own group's tables; in a bag, where every workgroup would add to the same 2048 words, to copy t % AQ_BAG_TABLES of the bag's
// tables (the select kernel sums the copies; the bag's state is that of copy 0).
template <int C>
__global__ __launch_bounds__(AQ_THREADS) void aq_hist_kernel(const float* __restrict__ x, unsigned* __restrict__ ws, int hw, int chunks,
                                                            int pass, int bag, int vec) {
    __shared__ unsigned hist[2 * AQ_BINS];
    MIL_POISON_STATIC(hist);
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * AQ_BINS; i += AQ_THREADS) hist[i] = 0u;
    __syncthreads();
    const size_t t = blockIdx.x / (unsigned)chunks;
    const int chunk = blockIdx.x % (unsigned)chunks;
    unsigned* W = ws + (bag ? t % AQ_BAG_TABLES : t) * AQ_WS_WORDS;
    const unsigned* S = ws + (bag ? (size_t)0 : t) * AQ_WS_WORDS + 2 * AQ_BINS;
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const unsigned mask = pass == 2 ? 1023u : 2047u;
    const int pshift = pass == 1 ? 21 : 10;                    // pass 0 has no prefix
    const unsigned plo = pass ? S[AQ_PLO] : 0u, phi = pass ? S[AQ_PHI] : 0u;
    const bool same = plo == phi;
    unsigned mn = 0xffffffffu, mx = 0u;
    const int p0 = chunk * AQ_CHUNK, p1 = p0 + AQ_CHUNK < hw ? p0 + AQ_CHUNK : hw;
    for (int p = p0 + tid * 4; p < p1; p += AQ_THREADS * 4) {
        const int cnt = p1 - p < 4 ? p1 - p : 4;
        float v[4];
        ar_values4<C>(x, t, hw, p, cnt, vec && cnt == 4, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) continue;
            const unsigned k = aq_key(v[j]);
            const unsigned d = (k >> shift) & mask;
            if (pass == 0) {
                atomicAdd(&hist[d], 1u);
                mn = k < mn ? k : mn;
                mx = k > mx ? k : mx;
            } else {
                const unsigned pre = k >> pshift;
                if (pre == plo) atomicAdd(&hist[d], 1u);
                if (!same && pre == phi) atomicAdd(&hist[AQ_BINS + d], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < AQ_BINS; i += AQ_THREADS) {
        const unsigned a = hist[i];
        if (a) atomicAdd(&W[i], a);
        if (!same) {
            const unsigned b = hist[AQ_BINS + i];
            if (b) atomicAdd(&W[AQ_BINS + i], b);
        }
    }
    if (pass == 0) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned on = __shfl_xor(mn, d), ox = __shfl_xor(mx, d);
            mn = on < mn ? on : mn;
            mx = ox > mx ? ox : mx;
        }
        if ((tid & 63) == 0 && mn <= mx) {                     // (a wave with no pixel keeps mn > mx)
            atomicMax(&W[2 * AQ_BINS + AQ_MAX], mx);
            atomicMax(&W[2 * AQ_BINS + AQ_NMIN], ~mn);
        }
    }
}

// Exclusive prefix of `mine` over the workgroup's threads in thread order (integer: exact).
__device__ __forceinline__ unsigned aq_block_exclusive(unsigned mine, unsigned* wave_sum) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                          // the previous use of wave_sum is over
    if (lane == 63) wave_sum[tid >> 6] = inc;
    __syncthreads();
    unsigned before = 0u;
    for (int w = 0; w < (tid >> 6); ++w) before += wave_sum[w];
    return before + inc - mine;
}

// One workgroup per group.  Each thread owns eight consecutive bins; the bin whose running count passes a rank is that rank's
// digit, and the rank minus the count before the bin is its rank in the next pass.  lo and hi = lo + 1 may fall into different
// bins, from then on they carry different prefixes and the histogram pass keeps a table for each.  The tables are cleared for
// the next pass.  The last pass (pass 2) has the two whole keys: stats[g] = (min, max, s[lo], s[hi]) and
//     p[g] = s[lo] + (s[hi] - s[lo]) t   (t < 0.5)     s[hi] - (s[hi] - s[lo]) (1 - t)   (otherwise)
// in fp64, each operation rounded on its own: numpy's _lerp.
__global__ __launch_bounds__(AQ_THREADS) void aq_select_kernel(unsigned* __restrict__ ws, int copies, int pass, unsigned rank_lo, unsigned rank_hi,
                                                              double tfrac, float* __restrict__ stats, double* __restrict__ pout) {
    __shared__ unsigned wave_sum[AQ_THREADS / 64];
    __shared__ unsigned found[4];
    MIL_POISON_STATIC(wave_sum);
    MIL_POISON_STATIC(found);
    const int tid = threadIdx.x;
    unsigned* W = ws + (size_t)blockIdx.x * copies * AQ_WS_WORDS;
    unsigned* S = W + 2 * AQ_BINS;
    const unsigned plo = pass ? S[AQ_PLO] : 0u, phi = pass ? S[AQ_PHI] : 0u;
    const unsigned rlo = pass ? S[AQ_RLO] : rank_lo, rhi = pass ? S[AQ_RHI] : rank_hi;
    unsigned kmax = 0u, knmin = 0u;
    for (int k = 0; k < copies; ++k) {
        const unsigned a = S[(size_t)k * AQ_WS_WORDS + AQ_MAX], b = S[(size_t)k * AQ_WS_WORDS + AQ_NMIN];
        kmax = a > kmax ? a : kmax;
        knmin = b > knmin ? b : knmin;
    }
    const bool same = plo == phi;
    if (tid < 4) found[tid] = 0u;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const unsigned* table = W + (which && !same ? AQ_BINS : 0);
        const unsigned r = which ? rhi : rlo;
        unsigned c[8], mine = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = 0u;
        for (int k = 0; k < copies; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] += table[(size_t)k * AQ_WS_WORDS + tid * 8 + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) mine += c[j];
        unsigned run = aq_block_exclusive(mine, wave_sum);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (r >= run && r - run < c[j]) { found[which * 2] = tid * 8 + j; found[which * 2 + 1] = r - run; }
            run += c[j];
        }
    }
    __syncthreads();
    for (int k = 0; k < copies; ++k)
        for (int i = tid; i < 2 * AQ_BINS; i += AQ_THREADS) W[(size_t)k * AQ_WS_WORDS + i] = 0u;
    if (tid != 0) return;
    const int bits = pass == 2 ? 10 : 11;
    const unsigned klo = (plo << bits) | found[0], khi = (phi << bits) | found[2];
    S[AQ_PLO] = klo; S[AQ_PHI] = khi; S[AQ_RLO] = found[1]; S[AQ_RHI] = found[3];
    if (pass != 2) return;
    const float slo = aq_unkey(klo), shi = aq_unkey(khi);
    const double d = rn_dsub((double)shi, (double)slo);
    const double p = tfrac < 0.5 ? rn_dadd((double)slo, rn_dmul(d, tfrac)) : rn_dsub((double)shi, rn_dmul(d, rn_dsub(1.0, tfrac)));
    float* st = stats + (size_t)blockIdx.x * 4;
    st[0] = aq_unkey(~knmin); st[1] = aq_unkey(kmax); st[2] = slo; st[3] = shi;
    pout[blockIdx.x] = p;
}

// q == 100: lo = hi = n - 1 and t = 0, so s[lo] = s[hi] = p = the maximum: the statistics after the first histogram pass.
__global__ __launch_bounds__(AQ_THREADS) void aq_minmax_kernel(const unsigned* __restrict__ ws, int copies, float* __restrict__ stats,
                                                              double* __restrict__ pout, int groups) {
    const int g = blockIdx.x * AQ_THREADS + threadIdx.x;
    if (g >= groups) return;
    const unsigned* S = ws + (size_t)g * copies * AQ_WS_WORDS + 2 * AQ_BINS;
    unsigned kmax = 0u, knmin = 0u;
    for (int k = 0; k < copies; ++k) {
        const unsigned a = S[(size_t)k * AQ_WS_WORDS + AQ_MAX], b = S[(size_t)k * AQ_WS_WORDS + AQ_NMIN];
        kmax = a > kmax ? a : kmax;
        knmin = b > knmin ? b : knmin;
    }
    const float mn = aq_unkey(~knmin), mx = aq_unkey(kmax);
    float* st = stats + (size_t)g * 4;
    st[0] = mn; st[1] = mx; st[2] = mx; st[3] = mx;
    pout[g] = (double)mx;
}

__device__ __forceinline__ unsigned ar_byte(float v) { return (unsigned)(int)v & 255u; }

// Four bytes per pixel group (gray) or twelve (interleaved RGB): whole = the destination is on the 4-byte grid.
__device__ __forceinline__ void ar_store_gray(uint8_t* __restrict__ out, size_t at, const unsigned (&b)[4], int cnt, bool whole) {
    if (whole) {
        *reinterpret_cast<unsigned*>(out + at) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) out[at + j] = (uint8_t)b[j];
    }
}
__device__ __forceinline__ void ar_store_rgb(uint8_t* __restrict__ out, size_t at, const unsigned (&b)[3][4], int cnt, bool whole) {
    if (whole) {
        unsigned* dst = reinterpret_cast<unsigned*>(out + at * 3);
        dst[0] = b[0][0] | (b[1][0] << 8) | (b[2][0] << 16) | (b[0][1] << 24);
        dst[1] = b[1][1] | (b[2][1] << 8) | (b[0][2] << 16) | (b[1][2] << 24);
        dst[2] = b[2][2] | (b[0][3] << 8) | (b[1][3] << 16) | (b[2][3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(at + j) * 3 + c] = (uint8_t)b[c][j];
            }
    }
}

// One thread = four consecutive pixels of one tile (fewer at a tile's end).  MODE 0: grayscale, x [T,C,hw] (C == 3: the sum of
// magnitudes; C == 1: the map), out0 [T,hw].  MODE 1: colour, MODE 2: positive / negative; x [T,3,hw], out0 (and out1) [T,hw,3].
// vec: 16-byte loads and 4-byte stores (hw % 4 == 0 and every pointer on its grid).
template <int MODE, int C>
__global__ __launch_bounds__(AQ_THREADS) void attr_render_kernel(const float* __restrict__ x, const float* __restrict__ stats, const double* __restrict__ pq,
                                                                uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, unsigned long long quads, int qpt,
                                                                int hw, int bag, int vec) {
    const unsigned long long q = (unsigned long long)blockIdx.x * AQ_THREADS + threadIdx.x;
    if (q >= quads) return;
    const size_t t = q / (unsigned)qpt;
    const int p = (int)(q % (unsigned)qpt) * 4;
    const int cnt = hw - p < 4 ? hw - p : 4;
    const bool whole = vec && cnt == 4;
    const size_t g = bag ? 0 : t;
    const float mn = stats[g * 4], mx = stats[g * 4 + 1];
    const size_t at = t * (size_t)hw + p;
    if constexpr (MODE == 0) {
        float v[4];
        ar_values4<C>(x, t, hw, p, cnt, whole, v);
        const double dmn = (double)mn, den = rn_dsub(pq[g], dmn);
        unsigned b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double r = rn_ddiv(rn_dsub((double)v[j], dmn), den);
            r = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);                       // np.clip; a NaN passes and converts to 0
            b[j] = den == 0.0 ? 0u : ((unsigned)(int)rn_dmul(255.0, r) & 255u);
        }
        ar_store_gray(out0, at, b, cnt, whole);
    } else {
        float gch[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) ar_load4(x, t * 3 + c, hw, p, cnt, whole, gch[c]);
        unsigned b0[3][4], b1[3][4];
        if constexpr (MODE == 1) {
            const float span = rn_sub(mx, mn);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    b0[c][j] = span == 0.f ? 0u : ar_byte(rn_mul(rn_div(rn_sub(gch[c][j], mn), span), 255.f));
            ar_store_rgb(out0, at, b0, cnt, whole);
        } else {
            const float nmn = -mn;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = gch[c][j];
                    // np.maximum(0, g) and np.maximum(0, -g)
                    b0[c][j] = mx > 0.f ? ar_byte(rn_mul(rn_div(v > 0.f ? v : 0.f, mx), 255.f)) : 0u;
                    b1[c][j] = nmn > 0.f ? ar_byte(rn_mul(rn_div(-v > 0.f ? -v : 0.f, nmn), 255.f)) : 0u;
                }
            ar_store_rgb(out0, at, b0, cnt, whole);
            ar_store_rgb(out1, at, b1, cnt, whole);
        }
    }
}

// apply_colormap_on_image: heat = lut[map] and Pillow's alpha_composite of (heat, alpha A) over the opaque tile, per channel
//     tmp = 64 (src A + dst (255 - A)) + (0x80 << 6);   out = (((tmp >> 8) + tmp) >> 8) >> 6
// tiles [T,3,hw] uint8 planar, map [T,hw] uint8, lut [256,3]; heat and on_image [T,hw,3].  The table sits in LDS.
__global__ __launch_bounds__(AQ_THREADS) void cam_overlay_kernel(const uint8_t* __restrict__ tiles, const uint8_t* __restrict__ map, const uint8_t* __restrict__ lut,
                                                                unsigned A, uint8_t* __restrict__ heat, uint8_t* __restrict__ on_image,
                                                                unsigned long long quads, int qpt, int hw, int vec) {
    __shared__ __attribute__((aligned(16))) uint8_t table[768];
    MIL_POISON_STATIC(table);
    for (int i = threadIdx.x; i < 768; i += AQ_THREADS) table[i] = lut[i];
    __syncthreads();
    const unsigned long long q = (unsigned long long)blockIdx.x * AQ_THREADS + threadIdx.x;
    if (q >= quads) return;
    const size_t t = q / (unsigned)qpt;
    const int p = (int)(q % (unsigned)qpt) * 4;
    const int cnt = hw - p < 4 ? hw - p : 4;
    const bool whole = vec && cnt == 4;
    const size_t at = t * (size_t)hw + p;
    unsigned m[4], dst[3][4];
    if (whole) {
        const unsigned w = *reinterpret_cast<const unsigned*>(map + at);
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = (w >> (8 * j)) & 255u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned d = *reinterpret_cast<const unsigned*>(tiles + (t * 3 + c) * (size_t)hw + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[c][j] = (d >> (8 * j)) & 255u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = j < cnt ? map[at + j] : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c][j] = j < cnt ? tiles[(t * 3 + c) * (size_t)hw + p + j] : 0u;
        }
    }
    unsigned h[3][4], o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned src = table[m[j] * 3 + c];
            const unsigned tmp = 64u * (src * A + dst[c][j] * (255u - A)) + (0x80u << 6);
            h[c][j] = src;
            o[c][j] = (((tmp >> 8) + tmp) >> 8) >> 6;
        }
    if (heat) ar_store_rgb(heat, at, h, cnt, whole);
    if (on_image) ar_store_rgb(on_image, at, o, cnt, whole);
}

// The virtual index of numpy's linear method, (n - 1) (q / 100) in fp64, split into lo = floor, hi = min(lo + 1, n - 1) and
// t = vi - lo; every operation rounded on its own.
static void aq_ranks(unsigned long long n, double q, unsigned* lo, unsigned* hi, double* t) {
#pragma clang fp contract(off)
    volatile double qq = q / 100.0;
    volatile double vi = (double)(n - 1) * qq;
    unsigned long long l = (unsigned long long)vi;             // vi >= 0: truncation is floor
    if (l > n - 1) l = n - 1;
    *lo = (unsigned)l;
    *hi = (unsigned)(l + 1 < n ? l + 1 : n - 1);
    *t = vi - (double)l;
}

// include/mil_hip.h has the contracts.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call.
extern "C" int mil_map_quantile_workspace(size_t* bytes, int n, int bag) {
    if (!bytes || n < 1 || bag < 0 || bag > 1) return MIL_ERR_ARG;
    *bytes = (size_t)(bag ? AQ_BAG_TABLES : n) * AQ_WS_WORDS * sizeof(unsigned);
    return MIL_OK;
}

extern "C" int mil_map_quantile(const float* x, int n, int channels, int H, int W, double q, int bag, void* workspace, size_t workspace_bytes,
                                float* stats, double* p, void* stream) {
    if (!x || !workspace || !stats || !p || n < 1 || H < 1 || W < 1 || (channels != 1 && channels != 3) || bag < 0 || bag > 1) return MIL_ERR_ARG;
    if (!(q > 0.0 && q <= 100.0)) return MIL_ERR_ARG;
    const int groups = bag ? 1 : n, copies = bag ? AQ_BAG_TABLES : 1;
    const size_t ws_bytes = (size_t)groups * copies * AQ_WS_WORDS * sizeof(unsigned);
    if (workspace_bytes < ws_bytes) return MIL_ERR_ARG;
    const unsigned long long hw = (unsigned long long)H * W, count = bag ? hw * (unsigned long long)n : hw;
    if (hw > 0x40000000ull || count > 0x7fffffffull) return MIL_ERR_UNSUPPORTED;      // (pixel indices are ints, stepped by a chunk)
    const unsigned long long chunks = (hw + AQ_CHUNK - 1) / AQ_CHUNK;
    if (chunks * (unsigned long long)n > INT_MAX) return MIL_ERR_UNSUPPORTED;
    const int vec = !(hw & 3) && !(reinterpret_cast<uintptr_t>(x) & 15);
    unsigned lo, hi;
    double t;
    aq_ranks(count, q, &lo, &hi, &t);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned* ws = static_cast<unsigned*>(workspace);
    if (hipMemsetAsync(ws, 0, ws_bytes, st) != hipSuccess) return MIL_ERR_LAUNCH;
    const dim3 grid((unsigned)(chunks * n)), block(AQ_THREADS);
    const int passes = q == 100.0 ? 1 : 3;
    for (int pass = 0; pass < passes; ++pass) {
        if (channels == 3)
            hipLaunchKernelGGL(aq_hist_kernel<3>, grid, block, 0, st, x, ws, (int)hw, (int)chunks, pass, bag, vec);
        else
            hipLaunchKernelGGL(aq_hist_kernel<1>, grid, block, 0, st, x, ws, (int)hw, (int)chunks, pass, bag, vec);
        MIL_CHECK_LAUNCH();
        if (passes == 1)
            hipLaunchKernelGGL(aq_minmax_kernel, dim3((groups + AQ_THREADS - 1) / AQ_THREADS), block, 0, st, ws, copies, stats, p, groups);
        else
            hipLaunchKernelGGL(aq_select_kernel, dim3(groups), block, 0, st, ws, copies, pass, lo, hi, t, stats, p);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_attr_render(const float* x, int n, int channels, int H, int W, int mode, int bag, const float* stats, const double* p,
                               uint8_t* out0, uint8_t* out1, void* stream) {
    if (!x || !stats || !out0 || n < 0 || H < 1 || W < 1 || bag < 0 || bag > 1 || mode < 0 || mode > 2) return MIL_ERR_ARG;
    if (mode == 0 ? ((channels != 1 && channels != 3) || !p) : channels != 3) return MIL_ERR_ARG;
    if (mode == 2 && !out1) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    const unsigned long long hw = (unsigned long long)H * W;
    if (hw > 0x7fffffffull) return MIL_ERR_UNSUPPORTED;
    const unsigned long long qpt = (hw + 3) / 4, quads = qpt * n, blocks = (quads + AQ_THREADS - 1) / AQ_THREADS;
    if (blocks > INT_MAX) return MIL_ERR_UNSUPPORTED;
    const uintptr_t grid4 = reinterpret_cast<uintptr_t>(out0) | reinterpret_cast<uintptr_t>(out1);
    const int vec = !(hw & 3) && !(reinterpret_cast<uintptr_t>(x) & 15) && !(grid4 & 3);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(AQ_THREADS);
    if (mode == 0 && channels == 3)
        hipLaunchKernelGGL((attr_render_kernel<0, 3>), grid, block, 0, st, x, stats, p, out0, out1, quads, (int)qpt, (int)hw, bag, vec);
    else if (mode == 0)
        hipLaunchKernelGGL((attr_render_kernel<0, 1>), grid, block, 0, st, x, stats, p, out0, out1, quads, (int)qpt, (int)hw, bag, vec);
    else if (mode == 1)
        hipLaunchKernelGGL((attr_render_kernel<1, 3>), grid, block, 0, st, x, stats, p, out0, out1, quads, (int)qpt, (int)hw, bag, vec);
    else
        hipLaunchKernelGGL((attr_render_kernel<2, 3>), grid, block, 0, st, x, stats, p, out0, out1, quads, (int)qpt, (int)hw, bag, vec);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_cam_overlay(const uint8_t* tiles, const uint8_t* map, const uint8_t* lut, int alpha, int n, int H, int W, uint8_t* heat,
                               uint8_t* on_image, void* stream) {
    if (!tiles || !map || !lut || (!heat && !on_image) || alpha < 0 || alpha > 255 || n < 0 || H < 1 || W < 1) return MIL_ERR_ARG;
    if (n == 0) return MIL_OK;
    const unsigned long long hw = (unsigned long long)H * W;
    if (hw > 0x7fffffffull) return MIL_ERR_UNSUPPORTED;
    const unsigned long long qpt = (hw + 3) / 4, quads = qpt * n, blocks = (quads + AQ_THREADS - 1) / AQ_THREADS;
    if (blocks > INT_MAX) return MIL_ERR_UNSUPPORTED;
    const uintptr_t grid4 = reinterpret_cast<uintptr_t>(tiles) | reinterpret_cast<uintptr_t>(map) | reinterpret_cast<uintptr_t>(heat) |
                            reinterpret_cast<uintptr_t>(on_image);
    const int vec = !(hw & 3) && !(grid4 & 3);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cam_overlay_kernel, dim3((unsigned)blocks), dim3(AQ_THREADS), 0, st, tiles, map, lut, (unsigned)alpha, heat, on_image, quads,
                       (int)qpt, (int)hw, vec);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
