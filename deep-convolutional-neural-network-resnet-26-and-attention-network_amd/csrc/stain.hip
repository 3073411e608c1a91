// H&E stain handling on the device for the resized uint8 tiles [T,3,H,W] (planar) that mil_tile_preprocess*_u8 write: the
// affine map in optical-density (OD) space that both stain normalisation (Macenko et al. 2009) and stain augmentation (Tellez
// et al. 2018) are, and the two reductions a Macenko fit needs.  include/mil_hip.h has the contracts; tests/stain_reference.py
// restates them in numpy.
//
// The byte contract.  tables (511 floats, built on the host in fp64 with log and rounded once) holds
//     L[v]  = -ln((v + 1) / 256),   v = 0..255   the OD of a byte (L[255] = 0)                                  tables[v]
//     TH[k] = -ln((k + 0.5) / 256), k = 1..255   strictly decreasing: the OD at which the byte goes from k - 1 to k   tables[255 + k]
// and byte(o) = #{k : o <= TH[k]}.  No exp decides a byte here: od_byte GUESSES the count from __expf and then moves it by
// comparisons against TH until  (c == 255 or o > TH[c + 1]) and (c == 0 or o <= TH[c])  holds, which only the count itself
// satisfies (TH is strictly decreasing).  A NaN compares false everywhere: byte 0, as the count gives.  Measured against an
// 8-step bisection of TH in LDS (24 dependent LDS reads per pixel instead of about 6): 0.150 against 0.248 ms for 500 tiles of
// 300 x 300 on an MI355X.
//
//   stain_affine_kernel   o_i = ((A[i,0] L[r] + A[i,1] L[g]) + A[i,2] L[b]) + b_i, every product and sum rounded once (rn_mul /
//                         rn_add: no fused multiply-add), stored as byte(o_i), in place: a thread reads the three planes' bytes of
//                         its four pixels before it writes any.
//   od_moments_kernel     per tissue pixel (L[r], L[g], L[b] all >= beta) the ten terms 1, od_c, od_c od_d (c <= d) in fp64 — the
//                         product of two fp32 values is exact there — added with rn_dadd in the slice layout of slice_sum.cuh:
//                         workgroup (t, s) owns a run of four-pixel groups of tile t, a thread adds its groups in order, the wave
//                         by a butterfly, the four waves in order; od_moments_finish adds the partial sums of a tile in slice order
//                         (bag 0) or of the whole stack in one workgroup's fixed tree (bag 1).  No floating-point atomics.
//   od_project_kernel     p_k = (P[k,0] L[r] + P[k,1] L[g]) + P[k,2] L[b] as fp32 maps; +inf where the pixel is not tissue (or, for
//                         the ratio, p_0 <= 0: the division is not evaluated there); valid[t] by one integer atomic per workgroup.
//                         Its third form ("sparse", mil_od_code_u8) writes the code (h0, h1) of snmf_code instead.
//   od_snmf_kernel        Vahadane's fit (sparse non-negative factorisation): per tissue pixel the closed-form two-variable
//                         non-negative lasso code in fp32 (snmf_code) and its twelve fp64 sums, in od_moments_kernel's layout.
//   od_snmf_finish        ONE workgroup adds the slice sums of the stack (bag 1's tree); one thread then updates W in fp64, writes
//                         the history row and the coder of the next pass: mil_od_snmf_fit_u8 enqueues iters x (od_snmf_kernel +
//                         od_snmf_finish) with W resident on the device and no host synchronisation.
//
// Accesses.  A thread takes four consecutive pixels of a plane.  The planes of a tile start at ANY byte alignment: a whole group
// whose address lies on the 4-byte grid is one dword access, every other group (and the last, partial one of a plane) goes byte
// by byte — no access leaves a plane.  The L (and TH) tables sit in LDS, filled behind a barrier.
#include "common.cuh"
#include "rounded.cuh"
#include <cfloat>
#include <climits>

#pragma clang fp contract(off)

#define ST_THREADS 256
#define ST_GROUPS 4                                     // groups of four pixels per thread (affine, project)
#define ST_PIX (ST_THREADS * 4 * ST_GROUPS)             // pixels per workgroup (affine, project)
#define OD_SLICES 16                                    // MIL_OD_SLICES of include/mil_hip.h (_lib.py states it for Python)
#define OD_TERMS 10
#define SNMF_TERMS 12                                   // MIL_SNMF_TERMS: the sums of one coding pass
#define SNMF_CODER 9                                    // fp32 W (6), c, d, lam
#define SNMF_EXTRA 20                                   // MIL_SNMF_EXTRA: the stack's twelve sums and the coder behind the slice sums

// four pixels of a plane from pixel i on (cnt of them real, the rest 0)
__device__ __forceinline__ void st_load4(const uint8_t* p, int i, int cnt, int v[4]) {
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(p + i) & 3) == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p + i);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (w >> (8 * q)) & 255;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = q < cnt ? p[i + q] : 0;
    }
}

__device__ __forceinline__ void st_store4(uint8_t* p, int i, int cnt, const int v[4]) {
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(p + i) & 3) == 0) {
        *reinterpret_cast<unsigned*>(p + i) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < cnt) p[i + q] = (uint8_t)v[q];
    }
}

// byte(o) = #{k in 1..255 : o <= th[k]}; th points at TH[0] (never read), th[1..255] strictly decreasing
__device__ __forceinline__ int od_byte(float o, const float* th) {
    const float g = 256.0f * __expf(-o) - 0.5f;                          // the guess: o <= TH[k] <=> 256 exp(-o) - 0.5 >= k
    int c = g >= 0.0f ? (g < 255.0f ? (int)g : 255) : 0;                 // a NaN starts at 0
    while (c < 255 && o <= th[c + 1]) ++c;
    while (c > 0 && !(o <= th[c])) --c;
    return c;
}

__global__ __launch_bounds__(ST_THREADS) void stain_affine_kernel(uint8_t* __restrict__ tiles, const float* __restrict__ affine,
                                                                   const float* __restrict__ tables, int n, int shared) {
    __shared__ float tab[512];
    MIL_POISON_STATIC(tab);
    const int tid = threadIdx.x, t = blockIdx.y;
    for (int k = tid; k < 511; k += ST_THREADS) tab[k] = tables[k];
    __syncthreads();
    const float* const th = tab + 255;
    const float* const a = affine + (shared ? 0 : 12 * (size_t)t);        // uniform over the workgroup
    float A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = a[k];
    uint8_t* const pr = tiles + (size_t)t * 3 * (size_t)n;
    uint8_t* const pg = pr + n;
    uint8_t* const pb = pg + n;
    const int base = blockIdx.x * ST_PIX;
    for (int j = 0; j < ST_GROUPS; ++j) {
        const int i = base + (j * ST_THREADS + tid) * 4;
        if (i >= n) break;
        const int cnt = min(4, n - i);
        int r[4], g[4], b[4];
        st_load4(pr, i, cnt, r); st_load4(pg, i, cnt, g); st_load4(pb, i, cnt, b);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float lr = tab[r[q]], lg = tab[g[q]], lb = tab[b[q]];
            int o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                o[c] = od_byte(rn_add(rn_add(rn_add(rn_mul(A[4 * c], lr), rn_mul(A[4 * c + 1], lg)), rn_mul(A[4 * c + 2], lb)), A[4 * c + 3]), th);
            r[q] = o[0]; g[q] = o[1]; b[q] = o[2];
        }
        st_store4(pr, i, cnt, r); st_store4(pg, i, cnt, g); st_store4(pb, i, cnt, b);
    }
}

// the fp64 siblings of slice_sum.cuh's wave_sum / waves_put / waves_get
__device__ __forceinline__ double od_wave_sum(double s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s = rn_dadd(s, __shfl_xor(s, d));
    return s;
}

// every thread hands in its N sums (ten moments, twelve coding sums); threads 0..N-1 return the workgroup's, term by term:
// ((w0 + w1) + w2) + w3
template <int N>
__device__ __forceinline__ double od_block_sums(double acc[N], double (*red)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double w = od_wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    const int k = threadIdx.x < N ? threadIdx.x : 0;
    return rn_dadd(rn_dadd(rn_dadd(red[0][k], red[1][k]), red[2][k]), red[3][k]);
}

// first pass: part[(t * OD_SLICES + s) * 10 + k]
__global__ __launch_bounds__(ST_THREADS) void od_moments_kernel(const uint8_t* __restrict__ tiles, const float* __restrict__ tables,
                                                                 double* __restrict__ part, int n, int per, float beta) {
    __shared__ float tab[256];
    __shared__ double red[ST_THREADS / 64][OD_TERMS];
    MIL_POISON_STATIC(tab); MIL_POISON_STATIC(red);
    const int tid = threadIdx.x, s = blockIdx.x % OD_SLICES;
    const size_t t = blockIdx.x / OD_SLICES;
    tab[tid] = tables[tid];
    __syncthreads();
    const uint8_t* const pr = tiles + t * 3 * (size_t)n;
    const uint8_t* const pg = pr + n;
    const uint8_t* const pb = pg + n;
    const int groups = (n + 3) / 4;                                      // groups of four pixels of the tile; slice s owns [lo, hi)
    const int lo = s * per < groups ? s * per : groups;
    const int hi = lo + per < groups ? lo + per : groups;
    double acc[OD_TERMS];
#pragma unroll
    for (int k = 0; k < OD_TERMS; ++k) acc[k] = 0.0;
    for (int gi = lo + tid; gi < hi; gi += ST_THREADS) {
        const int i = gi * 4, cnt = min(4, n - i);
        int r[4], g[4], b[4];
        st_load4(pr, i, cnt, r); st_load4(pg, i, cnt, g); st_load4(pb, i, cnt, b);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float lr = tab[r[q]], lg = tab[g[q]], lb = tab[b[q]];
            const bool tissue = q < cnt && lr >= beta && lg >= beta && lb >= beta;
            const double m = tissue ? 1.0 : 0.0;                         // a pixel that is not tissue adds ten exact zeros
            const double x = m * (double)lr, y = m * (double)lg, z = m * (double)lb;
            acc[0] = rn_dadd(acc[0], m);
            acc[1] = rn_dadd(acc[1], x); acc[2] = rn_dadd(acc[2], y); acc[3] = rn_dadd(acc[3], z);
            acc[4] = rn_dadd(acc[4], rn_dmul(x, x)); acc[5] = rn_dadd(acc[5], rn_dmul(x, y)); acc[6] = rn_dadd(acc[6], rn_dmul(x, z));
            acc[7] = rn_dadd(acc[7], rn_dmul(y, y)); acc[8] = rn_dadd(acc[8], rn_dmul(y, z)); acc[9] = rn_dadd(acc[9], rn_dmul(z, z));
        }
    }
    const double v = od_block_sums(acc, red);
    if (tid < OD_TERMS) part[((size_t)blockIdx.x) * OD_TERMS + tid] = v;
}

// second pass.  bag 0: workgroup t, thread k < 10 adds tile t's OD_SLICES partial sums of term k in slice order.  bag 1: ONE
// workgroup; thread i adds the rows i, i + 256, ... of part [rows,10] in order, then the workgroup's tree.
__global__ __launch_bounds__(ST_THREADS) void od_moments_finish(const double* __restrict__ part, double* __restrict__ out, int rows, int bag) {
    __shared__ double red[ST_THREADS / 64][OD_TERMS];
    MIL_POISON_STATIC(red);
    const int tid = threadIdx.x;
    if (!bag) {
        if (tid >= OD_TERMS) return;
        const double* const p = part + (size_t)blockIdx.x * OD_SLICES * OD_TERMS;
        double s = 0.0;
        for (int k = 0; k < OD_SLICES; ++k) s = rn_dadd(s, p[k * OD_TERMS + tid]);
        out[(size_t)blockIdx.x * OD_TERMS + tid] = s;
        return;
    }
    double acc[OD_TERMS];
#pragma unroll
    for (int k = 0; k < OD_TERMS; ++k) acc[k] = 0.0;
    for (int r = tid; r < rows; r += ST_THREADS) {
#pragma unroll
        for (int k = 0; k < OD_TERMS; ++k) acc[k] = rn_dadd(acc[k], part[(size_t)r * OD_TERMS + k]);
    }
    const double v = od_block_sums(acc, red);
    if (tid < OD_TERMS) out[tid] = v;
}

// ---- Vahadane's fit: the sparse non-negative factorisation's code, sums and dictionary update (include/mil_hip.h) ---------------
// k: the nine coder values W[0,0], W[0,1], W[1,0], W[1,1], W[2,0], W[2,1], c, d, lam.  The exact minimiser over h >= 0 of
// 1/2 |v - W h|^2 + lam (h0 + h1) for unit columns with 0 <= c < 1 (DESIGN.md section 3.53 has the KKT argument); d == 0 (collinear
// columns) gives (+-0, +-0).
__device__ __forceinline__ void snmf_code(const float k[SNMF_CODER], float lr, float lg, float lb, float& a0, float& a1) {
    const float q0 = rn_sub(rn_add(rn_add(rn_mul(k[0], lr), rn_mul(k[2], lg)), rn_mul(k[4], lb)), k[8]);
    const float q1 = rn_sub(rn_add(rn_add(rn_mul(k[1], lr), rn_mul(k[3], lg)), rn_mul(k[5], lb)), k[8]);
    const float h0 = rn_mul(rn_sub(q0, rn_mul(k[6], q1)), k[7]);
    const float h1 = rn_mul(rn_sub(q1, rn_mul(k[6], q0)), k[7]);
    if (h0 >= 0.0f && h1 >= 0.0f) { a0 = h0; a1 = h1; }
    else if (h1 < 0.0f) { a0 = q0 > 0.0f ? q0 : 0.0f; a1 = 0.0f; }
    else { a0 = 0.0f; a1 = q1 > 0.0f ? q1 : 0.0f; }
}

// od_moments_kernel's pass with the twelve coding sums: part[(t * OD_SLICES + s) * 12 + k]
__global__ __launch_bounds__(ST_THREADS) void od_snmf_kernel(const uint8_t* __restrict__ tiles, const float* __restrict__ tables,
                                                              const float* __restrict__ coder, double* __restrict__ part, int n, int per,
                                                              float beta) {
    __shared__ float tab[256];
    __shared__ double red[ST_THREADS / 64][SNMF_TERMS];
    MIL_POISON_STATIC(tab); MIL_POISON_STATIC(red);
    const int tid = threadIdx.x, s = blockIdx.x % OD_SLICES;
    const size_t t = blockIdx.x / OD_SLICES;
    tab[tid] = tables[tid];
    __syncthreads();
    float k[SNMF_CODER];
#pragma unroll
    for (int j = 0; j < SNMF_CODER; ++j) k[j] = coder[j];
    const uint8_t* const pr = tiles + t * 3 * (size_t)n;
    const uint8_t* const pg = pr + n;
    const uint8_t* const pb = pg + n;
    const int groups = (n + 3) / 4;
    const int lo = s * per < groups ? s * per : groups;
    const int hi = lo + per < groups ? lo + per : groups;
    double acc[SNMF_TERMS];
#pragma unroll
    for (int j = 0; j < SNMF_TERMS; ++j) acc[j] = 0.0;
    for (int gi = lo + tid; gi < hi; gi += ST_THREADS) {
        const int i = gi * 4, cnt = min(4, n - i);
        int r[4], g[4], b[4];
        st_load4(pr, i, cnt, r); st_load4(pg, i, cnt, g); st_load4(pb, i, cnt, b);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float lr = tab[r[q]], lg = tab[g[q]], lb = tab[b[q]];
            const bool tissue = q < cnt && lr >= beta && lg >= beta && lb >= beta;
            float a0, a1;
            snmf_code(k, lr, lg, lb, a0, a1);
            const double m = tissue ? 1.0 : 0.0;                         // a pixel that is not tissue adds twelve exact zeros
            const double h0 = tissue ? (double)a0 : 0.0, h1 = tissue ? (double)a1 : 0.0;
            const double x = (double)lr, y = (double)lg, z = (double)lb;
            acc[0] = rn_dadd(acc[0], m);
            acc[1] = rn_dadd(acc[1], rn_dmul(h0, h0)); acc[2] = rn_dadd(acc[2], rn_dmul(h0, h1)); acc[3] = rn_dadd(acc[3], rn_dmul(h1, h1));
            acc[4] = rn_dadd(acc[4], rn_dmul(x, h0)); acc[5] = rn_dadd(acc[5], rn_dmul(x, h1));
            acc[6] = rn_dadd(acc[6], rn_dmul(y, h0)); acc[7] = rn_dadd(acc[7], rn_dmul(y, h1));
            acc[8] = rn_dadd(acc[8], rn_dmul(z, h0)); acc[9] = rn_dadd(acc[9], rn_dmul(z, h1));
            acc[10] = rn_dadd(acc[10], h0); acc[11] = rn_dadd(acc[11], h1);
        }
    }
    const double v = od_block_sums(acc, red);
    if (tid < SNMF_TERMS) part[((size_t)blockIdx.x) * SNMF_TERMS + tid] = v;
}

// c = W_0 . W_1, d = 1 / (1 - c c) (0 for collinear columns) and the fp32 W of the next coding pass, from the fp64 W
__device__ __forceinline__ void snmf_put_coder(const double W[6], float lam, float* __restrict__ coder) {
    const double c = rn_dadd(rn_dadd(rn_dmul(W[0], W[1]), rn_dmul(W[2], W[3])), rn_dmul(W[4], W[5]));
    const double e = rn_dsub(1.0, rn_dmul(c, c));
    const double d = e > 0.0 ? rn_ddiv(1.0, e) : 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) coder[j] = (float)W[j];
    coder[6] = (float)c; coder[7] = (float)d; coder[8] = lam;
}

__global__ void od_snmf_init(const double* __restrict__ W, float lam, float* __restrict__ coder) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double w[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) w[j] = W[j];
    snmf_put_coder(w, lam, coder);
}

// ONE workgroup: od_moments_finish's bag tree over part [rows,12] into sums[12]; with W != nullptr thread 0 then makes the
// dictionary update of include/mil_hip.h in fp64, one rounded operation at a time, and writes W, the history row and the next coder
__global__ __launch_bounds__(ST_THREADS) void od_snmf_finish(const double* __restrict__ part, int rows, double* __restrict__ sums,
                                                              double* __restrict__ W, const double* __restrict__ moments, float lam,
                                                              float* __restrict__ coder, double* __restrict__ hist) {
    __shared__ double red[ST_THREADS / 64][SNMF_TERMS];
    __shared__ double fin[SNMF_TERMS];
    MIL_POISON_STATIC(red); MIL_POISON_STATIC(fin);
    const int tid = threadIdx.x;
    double acc[SNMF_TERMS];
#pragma unroll
    for (int k = 0; k < SNMF_TERMS; ++k) acc[k] = 0.0;
    for (int r = tid; r < rows; r += ST_THREADS) {
#pragma unroll
        for (int k = 0; k < SNMF_TERMS; ++k) acc[k] = rn_dadd(acc[k], part[(size_t)r * SNMF_TERMS + k]);
    }
    const double v = od_block_sums(acc, red);
    if (tid < SNMF_TERMS) { sums[tid] = v; fin[tid] = v; }
    if (W == nullptr) return;                                            // uniform over the workgroup
    __syncthreads();
    if (tid != 0) return;
    double s[SNMF_TERMS], w[6], old[6];
#pragma unroll
    for (int k = 0; k < SNMF_TERMS; ++k) s[k] = fin[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) old[k] = w[k] = W[k];
    const double A[2][2] = {{s[1], s[2]}, {s[2], s[3]}};
    // the objective of the W the codes were made with
    const double sv2 = rn_dadd(rn_dadd(moments[4], moments[7]), moments[9]);
    const double n00 = rn_dadd(rn_dadd(rn_dmul(w[0], w[0]), rn_dmul(w[2], w[2])), rn_dmul(w[4], w[4]));
    const double n01 = rn_dadd(rn_dadd(rn_dmul(w[0], w[1]), rn_dmul(w[2], w[3])), rn_dmul(w[4], w[5]));
    const double n11 = rn_dadd(rn_dadd(rn_dmul(w[1], w[1]), rn_dmul(w[3], w[3])), rn_dmul(w[5], w[5]));
    double wb = rn_dadd(rn_dadd(rn_dmul(w[0], s[4]), rn_dmul(w[2], s[6])), rn_dmul(w[4], s[8]));
    wb = rn_dadd(rn_dadd(rn_dadd(wb, rn_dmul(w[1], s[5])), rn_dmul(w[3], s[7])), rn_dmul(w[5], s[9]));
    const double quad = rn_dadd(rn_dadd(rn_dmul(A[0][0], n00), rn_dmul(rn_dmul(2.0, A[0][1]), n01)), rn_dmul(A[1][1], n11));
    const double f = rn_dadd(rn_dadd(rn_dsub(rn_dmul(sv2, 0.5), wb), rn_dmul(quad, 0.5)), rn_dmul((double)lam, rn_dadd(s[10], s[11])));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double ajj = A[j][j];
        if (!(ajj > 0.0)) continue;                                      // this stain coded no pixel: the column stays
        double u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double wa = rn_dadd(rn_dmul(w[2 * c], A[0][j]), rn_dmul(w[2 * c + 1], A[1][j]));
            const double x = rn_dadd(w[2 * c + j], rn_ddiv(rn_dsub(s[4 + 2 * c + j], wa), ajj));
            u[c] = x < 0.0 ? 0.0 : x;
        }
        const double nn = rn_dadd(rn_dadd(rn_dmul(u[0], u[0]), rn_dmul(u[1], u[1])), rn_dmul(u[2], u[2]));
        if (!(nn > 0.0)) continue;
        const double len = __builtin_sqrt(nn);
#pragma unroll
        for (int c = 0; c < 3; ++c) w[2 * c + j] = rn_ddiv(u[c], len);
    }
    double move = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double dlt = __builtin_fabs(rn_dsub(w[k], old[k]));
        move = dlt > move ? dlt : move;
        W[k] = w[k];
    }
    hist[0] = f; hist[1] = move;
    snmf_put_coder(w, lam, coder);
}

// four fp32 values to map element i on: one 16-byte store where the address allows, else one by one
__device__ __forceinline__ void st_store4f(float* p, int cnt, const float v[4]) {
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<f32x4_t*>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < cnt) p[q] = v[q];
    }
}

template <int MODE>
__global__ __launch_bounds__(ST_THREADS) void od_project_kernel(const uint8_t* __restrict__ tiles, const float* __restrict__ tables,
                                                                 const float* __restrict__ P, float* __restrict__ map0, float* __restrict__ map1,
                                                                 int* __restrict__ valid, int n, float beta) {
    __shared__ float tab[256];
    __shared__ int red[ST_THREADS / 64];
    MIL_POISON_STATIC(tab); MIL_POISON_STATIC(red);
    const int tid = threadIdx.x, t = blockIdx.y;
    tab[tid] = tables[tid];
    __syncthreads();
    constexpr int NP = MODE == 2 ? SNMF_CODER : 6;                       // MODE 2 ("sparse"): P is the coder of snmf_code
    float p[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) p[k] = P[k];
    const uint8_t* const pr = tiles + (size_t)t * 3 * (size_t)n;
    const uint8_t* const pg = pr + n;
    const uint8_t* const pb = pg + n;
    float* const m0 = map0 + (size_t)t * (size_t)n;
    float* const m1 = MODE != 1 ? map1 + (size_t)t * (size_t)n : nullptr;
    const int base = blockIdx.x * ST_PIX;
    const float inf = __builtin_inff();
    int count = 0;
    for (int j = 0; j < ST_GROUPS; ++j) {
        const int i = base + (j * ST_THREADS + tid) * 4;
        if (i >= n) break;
        const int cnt = min(4, n - i);
        int r[4], g[4], b[4];
        st_load4(pr, i, cnt, r); st_load4(pg, i, cnt, g); st_load4(pb, i, cnt, b);
        float v0[4], v1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float lr = tab[r[q]], lg = tab[g[q]], lb = tab[b[q]];
            const bool tissue = lr >= beta && lg >= beta && lb >= beta;
            v0[q] = v1[q] = inf;
            if (MODE == 2) {
                float a0, a1;
                snmf_code(p, lr, lg, lb, a0, a1);
                if (tissue) { v0[q] = a0; v1[q] = a1; count += q < cnt; }
                continue;
            }
            const float p0 = rn_add(rn_add(rn_mul(p[0], lr), rn_mul(p[1], lg)), rn_mul(p[2], lb));
            const float p1 = rn_add(rn_add(rn_mul(p[3], lr), rn_mul(p[4], lg)), rn_mul(p[5], lb));
            if (MODE == 0) {
                if (tissue) { v0[q] = p0; v1[q] = p1; count += q < cnt; }
            } else if (tissue && p0 > 0.0f) {
                v0[q] = rn_div(p1, p0);
                count += q < cnt;
            }
        }
        st_store4f(m0 + i, cnt, v0);
        if (MODE != 1) st_store4f(m1 + i, cnt, v1);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) count += __shfl_xor(count, s);
    if ((tid & 63) == 0) red[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < ST_THREADS / 64; ++w) v += red[w];
        if (v) atomicAdd(valid + t, v);
    }
}

// what the three entries share: MIL_OK when T tiles of H x W are a stack their kernels index in 32 bits
static int stain_shape(int T, int H, int W) {
    if (T < 0 || H < 1 || W < 1) return MIL_ERR_ARG;
    if ((unsigned long long)H * (unsigned long long)W > (unsigned long long)(INT_MAX - ST_PIX)) return MIL_ERR_UNSUPPORTED;
    return MIL_OK;
}

extern "C" int mil_stain_affine_u8(uint8_t* tiles, const float* affine, const float* tables, int T, int H, int W, int shared, void* stream) {
    if (!tiles || !affine || !tables || (shared != 0 && shared != 1)) return MIL_ERR_ARG;
    const int rc = stain_shape(T, H, W);
    if (rc != MIL_OK) return rc;
    if (T == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int n = H * W, split = (n + ST_PIX - 1) / ST_PIX;
    for (int done = 0; done < T; done += 65535) {               // grid.y limit
        const int m = T - done < 65535 ? T - done : 65535;
        hipLaunchKernelGGL(stain_affine_kernel, dim3(split, m), dim3(ST_THREADS), 0, st, tiles + (size_t)done * 3 * (size_t)n,
                           affine + (shared ? 0 : 12 * (size_t)done), tables, n, shared);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_od_moments_u8(const uint8_t* tiles, const float* tables, int T, int H, int W, float beta, int bag, double* workspace,
                                 size_t workspace_bytes, double* out, void* stream) {
    if (!tiles || !tables || !workspace || !out || (bag != 0 && bag != 1) || beta != beta) return MIL_ERR_ARG;
    const int rc = stain_shape(T, H, W);
    if (rc != MIL_OK) return rc;
    if (T > INT_MAX / OD_SLICES) return MIL_ERR_UNSUPPORTED;
    if (workspace_bytes < (size_t)T * OD_SLICES * OD_TERMS * sizeof(double)) return MIL_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (T == 0) {                                               // a bag of no tiles has ten zero sums; no tile, no group
        if (bag && hipMemsetAsync(out, 0, OD_TERMS * sizeof(double), st) != hipSuccess) return MIL_ERR_LAUNCH;
        return MIL_OK;
    }
    const int n = H * W, groups = (n + 3) / 4, per = (groups + OD_SLICES - 1) / OD_SLICES;
    hipLaunchKernelGGL(od_moments_kernel, dim3(T * OD_SLICES), dim3(ST_THREADS), 0, st, tiles, tables, workspace, n, per, beta);
    MIL_CHECK_LAUNCH();
    hipLaunchKernelGGL(od_moments_finish, dim3(bag ? 1 : T), dim3(ST_THREADS), 0, st, workspace, out, T * OD_SLICES, bag);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_od_snmf_sums_u8(const uint8_t* tiles, const float* tables, const float* coder, int T, int H, int W, float beta,
                                   double* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (!tiles || !tables || !coder || !workspace || !out || beta != beta) return MIL_ERR_ARG;
    const int rc = stain_shape(T, H, W);
    if (rc != MIL_OK) return rc;
    if (T > INT_MAX / OD_SLICES) return MIL_ERR_UNSUPPORTED;
    if (workspace_bytes < (size_t)T * OD_SLICES * SNMF_TERMS * sizeof(double)) return MIL_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (T == 0) return hipMemsetAsync(out, 0, SNMF_TERMS * sizeof(double), st) == hipSuccess ? MIL_OK : MIL_ERR_LAUNCH;
    const int n = H * W, groups = (n + 3) / 4, per = (groups + OD_SLICES - 1) / OD_SLICES;
    hipLaunchKernelGGL(od_snmf_kernel, dim3(T * OD_SLICES), dim3(ST_THREADS), 0, st, tiles, tables, coder, workspace, n, per, beta);
    MIL_CHECK_LAUNCH();
    hipLaunchKernelGGL(od_snmf_finish, dim3(1), dim3(ST_THREADS), 0, st, workspace, T * OD_SLICES, out, static_cast<double*>(nullptr),
                       static_cast<const double*>(nullptr), 0.0f, static_cast<float*>(nullptr), static_cast<double*>(nullptr));
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_od_snmf_fit_u8(const uint8_t* tiles, const float* tables, double* W, const double* moments, int T, int H, int Wd,
                                  float lam, int iters, float beta, double* workspace, size_t workspace_bytes, double* history,
                                  void* stream) {
    if (!tiles || !tables || !W || !moments || !workspace || !history || beta != beta || !(lam >= 0.0f) || lam > FLT_MAX || iters < 1)
        return MIL_ERR_ARG;
    const int rc = stain_shape(T, H, Wd);
    if (rc != MIL_OK) return rc;
    if (T > INT_MAX / OD_SLICES) return MIL_ERR_UNSUPPORTED;
    const size_t part = (size_t)T * OD_SLICES * SNMF_TERMS;
    if (workspace_bytes < (part + SNMF_EXTRA) * sizeof(double)) return MIL_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* const sums = workspace + part;                              // [12], then the coder's nine floats
    float* const coder = reinterpret_cast<float*>(sums + SNMF_TERMS);
    const int n = H * Wd, groups = (n + 3) / 4, per = (groups + OD_SLICES - 1) / OD_SLICES;
    hipLaunchKernelGGL(od_snmf_init, dim3(1), dim3(64), 0, st, W, lam, coder);
    MIL_CHECK_LAUNCH();
    for (int it = 0; it < iters; ++it) {
        if (T > 0) {                                                     // no tile: no slice sum, the finish adds zero rows
            hipLaunchKernelGGL(od_snmf_kernel, dim3(T * OD_SLICES), dim3(ST_THREADS), 0, st, tiles, tables, coder, workspace, n, per, beta);
            MIL_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(od_snmf_finish, dim3(1), dim3(ST_THREADS), 0, st, workspace, T * OD_SLICES, sums, W, moments, lam, coder,
                           history + 2 * (size_t)it);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

// what mil_od_project_u8 (modes 0, 1) and mil_od_code_u8 (mode 2, "sparse": P is the coder) share
static int project_launch(const uint8_t* tiles, const float* tables, const float* P, int T, int H, int W, int mode, float beta,
                          float* maps, int32_t* valid, void* stream) {
    if (!tiles || !tables || !P || !maps || !valid || beta != beta) return MIL_ERR_ARG;
    const int rc = stain_shape(T, H, W);
    if (rc != MIL_OK) return rc;
    if (T == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(valid, 0, (size_t)T * sizeof(int32_t), st) != hipSuccess) return MIL_ERR_LAUNCH;
    const int n = H * W, split = (n + ST_PIX - 1) / ST_PIX;
    float* const second = maps + (size_t)T * (size_t)n;         // modes 0 and 2: maps [2,T,H,W]
    for (int done = 0; done < T; done += 65535) {               // grid.y limit
        const int m = T - done < 65535 ? T - done : 65535;
        const uint8_t* const src = tiles + (size_t)done * 3 * (size_t)n;
        const size_t off = (size_t)done * (size_t)n;
        if (mode == 0)
            hipLaunchKernelGGL(od_project_kernel<0>, dim3(split, m), dim3(ST_THREADS), 0, st, src, tables, P, maps + off, second + off,
                               valid + done, n, beta);
        else if (mode == 2)
            hipLaunchKernelGGL(od_project_kernel<2>, dim3(split, m), dim3(ST_THREADS), 0, st, src, tables, P, maps + off, second + off,
                               valid + done, n, beta);
        else
            hipLaunchKernelGGL(od_project_kernel<1>, dim3(split, m), dim3(ST_THREADS), 0, st, src, tables, P, maps + off,
                               static_cast<float*>(nullptr), valid + done, n, beta);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_od_project_u8(const uint8_t* tiles, const float* tables, const float* P, int T, int H, int W, int mode, float beta,
                                 float* maps, int32_t* valid, void* stream) {
    if (mode != 0 && mode != 1) return MIL_ERR_ARG;
    return project_launch(tiles, tables, P, T, H, W, mode, beta, maps, valid, stream);
}

extern "C" int mil_od_code_u8(const uint8_t* tiles, const float* tables, const float* coder, int T, int H, int W, float beta, float* maps,
                              int32_t* valid, void* stream) {
    return project_launch(tiles, tables, coder, T, H, W, 2, beta, maps, valid, stream);
}
