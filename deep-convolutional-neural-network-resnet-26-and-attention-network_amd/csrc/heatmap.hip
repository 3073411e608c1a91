// Attention heat maps on the device: what the reference's visualize() -> create_map() (gbm/classify_combined.py:142-218) draws
// on its five tissue axes, as five uint8 RGB panels at thumbnail scale, rendered from the resident slide.  create_map takes every
// kept ROI as pixels ([T,1200,1200,3]), imshow()s each and puts one coloured rectangle per tile on the axes; here one kernel reads
// every kept window once where it lies, box-reduces it by D in both directions and blends the attention colours:
//     panel 0      the tissue (box mean of the window), under the mean map's jet colour at alpha_tissue    (ax[0,0], :189-193)
//     panel 1      per tile, its 80 features as an 8 x 10 viridis image, inset by `inset` slide pixels     (ax[0,1], :203)
//     panels 2-4   the three attention maps as jet rectangles at alpha_map on the caller's canvas          (ax[1,0..2], :194-202)
// All arithmetic is integer (include/mil_hip.h states it), so the picture does not depend on the order of anything.
//
// Source convention and loads: roi_select.hip's.  Row y of window t starts at byte win_off[t] + y * row_pitch of the source at ANY
// byte alignment; a row is cut into 48-byte chunks on the 16-byte grid of the source, a lane loads its chunk with three aligned
// 16-byte loads, takes the dword behind it from the next lane, funnel-shifts by the pixel phase p = al % 3 and has the sixteen
// pixels that START in the chunk at compile-time byte positions: pixel j of chunk c is pixel k0 + j of the row, k0 = 16c - al / 3.
// Every load goes through a buffer descriptor that starts at the grid point below the workgroup's first row and ends with the
// source (rounded up to the 16-byte grid); offsets are 32-bit (the host bounds rows-per-workgroup * row_pitch).
//
// Layout of the work.  n = S / D.  A workgroup takes output rows [a0, a0 + rpb) of one window = source rows [a0 D, (a0 + rpb) D):
// whole output rows, so nothing is accumulated across workgroups.  Its LDS holds, per output row, n + 2 bins of three 32-bit
// channel sums: bin b + 1 for output pixel b, bin 0 for the pixels left of the window and bin n + 1 for those right of it (a
// chunk's pixels outside [0, S) are not masked: they are summed into the two dump bins nobody reads).  Work items (row, chunk)
// are walked row-major as in roi_stats_kernel, the next item's bytes travel while this one is summed.
//   D >= 16: the sixteen pixels of a chunk lie in at most two neighbouring bins (dump bins included), split at pixel
//     jsplit = D - (k0 + D) % D.  The three bytes of a channel of four pixels are gathered into one dword (two v_perm_b32), summed
//     with v_sad_u8 once as they are (the chunk's total) and once under the byte mask of the pixels below jsplit: 6 LDS adds a
//     chunk.  (k0 + D) / D by a multiply-high with 2^32 / D + 1 and one correction.
//   D < 16: every valid pixel is added to its bin on its own (3 LDS adds a pixel); the bin advances by counting.
// LDS adds of 32-bit integers: sums stay below 2^32 for D <= 4096 (255 D^2 + D^2 / 2), and their order does not matter.
// Epilogue: one thread per output pixel of the workgroup's rows divides, blends and stores bytes; a pixel outside the
// [Ht, Wt] canvas is not stored (out_pos is a device array the host cannot check).
#include "pf_common.cuh"

#define HEAT_THREADS 256
#define HEAT_MAX_D 4096
#define HEAT_MAX_N 4000                     // (n + 2) * 12 bytes of LDS for ONE output row stay below 48 KB
#define HEAT_LDS_TARGET 16384               // rows per workgroup are chosen so that the bins stay below this where one row does
#define HEAT_LDS_MAX 49152

struct HeatArgs {
    const uint8_t* base_al;         // source pointer rounded down to the 16-byte grid
    const long long* win_off;       // [T] byte offset of each window's first pixel from the (unrounded) source pointer
    const int* pos;                 // [T,2] top-left output pixel (row, col) of each window
    const short* jidx;              // jet index of map r, window t at jidx[r * jstride + t]; < 0: no rectangle
    const uint8_t* fidx;            // [T,80] viridis indices or null
    const uint8_t* jet;             // [105,3]
    const uint8_t* vir;             // [256,3]
    uint8_t* out;                   // [5,Ht,Wt,3]
    long long total;                // bytes from base_al to the grid point at or behind the end of the source
    long long pitch;                // bytes between two rows of a window
    long long jstride;              // windows in the whole call (a launch takes 65535 of them)
    int delta;                      // source pointer - base_al (0..15)
    int S, D, n, rpb, C, Ht, Wt, g, q0, q1;     // rpb: OUTPUT rows per workgroup; C: chunks per row; g: inset in output pixels
    unsigned rcpD;                  // 2^32 / D + 1 (D >= 16)
};

__device__ __forceinline__ unsigned heat_byte(const unsigned (&e)[12], int b) { return (e[b >> 2] >> ((b & 3) * 8)) & 0xffu; }

// byte mask of the first s (0..4) bytes of a dword
__device__ __forceinline__ unsigned heat_low_bytes(int s) { return s >= 4 ? 0xffffffffu : (1u << (8 * s)) - 1u; }

template <bool BIG>
__global__ __launch_bounds__(HEAT_THREADS) void heatmap_kernel(HeatArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned hsm[];
    MIL_POISON(hsm);
    const int tid = threadIdx.x, lane = tid & 63, t = blockIdx.y;
    const int S = a.S, C = a.C, D = a.D, n = a.n, slots = n + 2;
    const int a0 = blockIdx.x * a.rpb;
    const int orows = min(a.rpb, n - a0);
    if (orows <= 0) return;
    const int rows = orows * D, y0 = a0 * D;
    for (int i = tid; i < orows * slots * 3; i += HEAT_THREADS) hsm[i] = 0u;
    __syncthreads();

    // descriptor of this workgroup: from the grid point below its first row to the end of the source
    const long long woff = a.win_off[t];
    const long long r0 = (long long)a.delta + woff + (long long)y0 * a.pitch;
    const long long B = r0 & ~15ll;
    const long long left = a.total - B;
    const unsigned range = (woff < 0 || left <= 0) ? 0u : (left > 0x80000000ll ? 0x80000000u : (unsigned)left);
    const __amdgpu_buffer_rsrc_t rs = mil_rsrc(a.base_al + B, range);
    const unsigned rel0 = (unsigned)(r0 - B), pitch = (unsigned)a.pitch;
    const int row_bytes = 3 * S;

    // work items (row, chunk), row-major: this thread takes items tid, tid + 256, ... — walked with carries; the row is kept
    // as (output row ya, source row yrem inside it) too, so that no item divides by D for it
    int yr = tid / C, c = tid - yr * C;
    int ya = yr / D, yrem = yr - ya * D;
    const int dy = HEAT_THREADS / C, dc = HEAT_THREADS - dy * C;
    const int dya = dy / D, dyrem = dy - dya * D;
    const int nit = (rows * C + HEAT_THREADS - 1) / HEAT_THREADS;

    u32x4_t q[3];
    unsigned own = 0, al = 0;
    bool live = false;
    auto fetch = [&]() {
        const unsigned r = rel0 + (unsigned)yr * pitch;
        al = r & 15u;
        live = yr < rows && 48 * c < (int)al + row_bytes;                       // the chunk holds bytes of the row
        const unsigned off = live ? (r & ~15u) + 48u * (unsigned)c : MIL_OOB;
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, live ? off + 16u * i : MIL_OOB, 0, 0);
        own = __builtin_amdgcn_raw_buffer_load_b32(rs, (live && lane == 63) ? off + 48u : MIL_OOB, 0, 0);
    };
    fetch();

    for (int it = 0; it < nit; ++it) {
        unsigned d[13];
#pragma unroll
        for (int i = 0; i < 12; ++i) d[i] = q[i >> 2][i & 3];
        const unsigned nxt = __shfl_down(d[0], 1);
        d[12] = lane == 63 ? own : nxt;
        const int k0 = 16 * c - (int)(al / 3u);
        const unsigned p = al % 3u;
        const bool cur = live;
        unsigned* const acc = hsm + ya * slots * 3;

        yr += dy; c += dc; ya += dya; yrem += dyrem;
        if (c >= C) { c -= C; ++yr; ++yrem; }
        if (yrem >= D) { yrem -= D; ++ya; }
        if (it + 1 < nit) fetch();                      // the next item's bytes travel while this one is summed

        if (!cur) continue;                             // a chunk without bytes of the row (or behind the last row): no bin
        unsigned e[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) e[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], p);

        if constexpr (BIG) {
            // pixels [0, jsplit) of the chunk -> bin qb, the rest -> bin qb + 1 (bins counted with the left dump bin as 0)
            const unsigned kk = (unsigned)(k0 + D);                 // k0 >= -5 and D >= 16
            unsigned qb = __umulhi(kk, a.rcpD);                     // floor(kk / D) or one more
            int rem = (int)(kk - qb * (unsigned)D);
            if (rem < 0) { --qb; rem += D; }
            const int jsplit = D - rem;
            unsigned tot0 = 0, tot1 = 0, tot2 = 0, lo0 = 0, lo1 = 0, lo2 = 0;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const unsigned d0 = e[3 * g4], d1 = e[3 * g4 + 1], d2 = e[3 * g4 + 2];
                // v_perm_b32(s0, s1, sel): selector 0-3 = byte of s1, 4-7 = byte of s0, 0x0c = 0x00
                const unsigned r4 = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x0c060300u), 0x05020100u);
                const unsigned g_4 = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x0c070401u), 0x06020100u);
                const unsigned b4 = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x0c0c0502u), 0x07040100u);
                const unsigned mk = heat_low_bytes(min(max(jsplit - 4 * g4, 0), 4));
                tot0 = __builtin_amdgcn_sad_u8(r4, 0u, tot0); lo0 = __builtin_amdgcn_sad_u8(r4 & mk, 0u, lo0);
                tot1 = __builtin_amdgcn_sad_u8(g_4, 0u, tot1); lo1 = __builtin_amdgcn_sad_u8(g_4 & mk, 0u, lo1);
                tot2 = __builtin_amdgcn_sad_u8(b4, 0u, tot2); lo2 = __builtin_amdgcn_sad_u8(b4 & mk, 0u, lo2);
            }
            unsigned* const pa = acc + 3 * min((int)qb, n + 1);
            atomicAdd(pa, lo0); atomicAdd(pa + 1, lo1); atomicAdd(pa + 2, lo2);
            if (jsplit < 16) {
                unsigned* const pb = acc + 3 * min((int)qb + 1, n + 1);
                atomicAdd(pb, tot0 - lo0); atomicAdd(pb + 1, tot1 - lo1); atomicAdd(pb + 2, tot2 - lo2);
            }
        } else {
            // valid pixels of this chunk: j in [jlo, jhi) with row pixel k0 + j in [0, S)
            const int jlo = min(max(-k0, 0), 16), jhi = min(max(S - k0, 0), 16);
            if (jhi > jlo) {
                int bin = (k0 + jlo) / D, rem = (k0 + jlo) - bin * D;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (j >= jlo && j < jhi) {
                        unsigned* const pa = acc + 3 * (bin + 1);
                        atomicAdd(pa, heat_byte(e, 3 * j)); atomicAdd(pa + 1, heat_byte(e, 3 * j + 1));
                        atomicAdd(pa + 2, heat_byte(e, 3 * j + 2));
                        if (++rem == D) { rem = 0; ++bin; }
                    }
                }
            }
        }
    }
    __syncthreads();

    // epilogue: one thread per output pixel (a, b) of the workgroup's rows
    const int oy0 = a.pos[2 * (size_t)t], ox0 = a.pos[2 * (size_t)t + 1];
    const int i0 = min((int)a.jidx[t], 104), i1 = min((int)a.jidx[a.jstride + t], 104);
    const int i2 = min((int)a.jidx[2 * a.jstride + t], 104), i3 = min((int)a.jidx[3 * a.jstride + t], 104);
    const unsigned DD = (unsigned)D * (unsigned)D, half = DD / 2u;
    const int g = a.g, w = n - 2 * g, q0 = a.q0, q1 = a.q1;
    const size_t plane = (size_t)a.Ht * a.Wt * 3;
    for (int pix = tid; pix < orows * n; pix += HEAT_THREADS) {
        const int arow = pix / n, b = pix - arow * n, aa = a0 + arow;
        const int oy = oy0 + aa, ox = ox0 + b;
        if ((unsigned)oy >= (unsigned)a.Ht || (unsigned)ox >= (unsigned)a.Wt) continue;
        const unsigned* const s = hsm + (arow * slots + b + 1) * 3;
        uint8_t* const o = a.out + ((size_t)oy * a.Wt + ox) * 3;
        const bool feat = a.fidx != nullptr && aa >= g && aa < n - g && b >= g && b < n - g;
        int code = 0;
        if (feat) code = a.fidx[(size_t)t * 80 + ((aa - g) * 8 / w) * 10 + (b - g) * 10 / w];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int m = (int)((s[ch] + half) / DD);
            o[ch] = (uint8_t)(i0 < 0 ? m : (m * (256 - q0) + (int)a.jet[3 * i0 + ch] * q0 + 128) >> 8);
            if (feat) o[plane + ch] = a.vir[3 * code + ch];
            if (i1 >= 0) o[2 * plane + ch] = (uint8_t)((255 * (256 - q1) + (int)a.jet[3 * i1 + ch] * q1 + 128) >> 8);
            if (i2 >= 0) o[3 * plane + ch] = (uint8_t)((255 * (256 - q1) + (int)a.jet[3 * i2 + ch] * q1 + 128) >> 8);
            if (i3 >= 0) o[4 * plane + ch] = (uint8_t)((255 * (256 - q1) + (int)a.jet[3 * i3 + ch] * q1 + 128) >> 8);
        }
    }
}

// The five panels of create_map (gbm/classify_combined.py:169-218) for T windows of a resident source; include/mil_hip.h has
// the contract.  Everything that can be refused is refused here, on the host, before any GPU call.
extern "C" int mil_heatmap_render(const uint8_t* base, int64_t base_bytes, const int64_t* win_off, int64_t row_pitch, int T, int S,
                                  int D, const int32_t* out_pos, const int16_t* jet_idx, const uint8_t* feat_idx,
                                  const uint8_t* jet_lut, const uint8_t* viridis_lut, int inset, int alpha_tissue, int alpha_map,
                                  uint8_t* out, int Ht, int Wt, void* stream) {
    if (!base || !win_off || !out_pos || !jet_idx || !jet_lut || !out || (feat_idx && !viridis_lut)) return MIL_ERR_ARG;
    if (base_bytes < 0 || T < 0 || S < 1 || D < 1 || S % D != 0 || inset < 0 || Ht < 1 || Wt < 1) return MIL_ERR_ARG;
    if (alpha_tissue < 0 || alpha_tissue > 256 || alpha_map < 0 || alpha_map > 256) return MIL_ERR_ARG;
    if (row_pitch < 3 * (int64_t)S) return MIL_ERR_ARG;
    const int n = S / D;
    if (D > HEAT_MAX_D || n > HEAT_MAX_N) return MIL_ERR_UNSUPPORTED;
    const int C = (3 * S + 15 + 47) / 48;
    // 32-bit offsets inside a workgroup's descriptor: the source rows of its output rows + one row of chunks below 2 GiB
    const int64_t rpb_max = ((int64_t)0x7fff0000 - 48 * (int64_t)C) / row_pitch / D;
    if (rpb_max < 1) return MIL_ERR_UNSUPPORTED;
    if (T == 0) return MIL_OK;

    // output rows per workgroup: about 4096 workgroups in the launch (16 per CU), but at least ~8 work items per thread,
    // and bins of no more than HEAT_LDS_TARGET bytes (one output row's are always allowed)
    const int want = (4096 + T - 1) / T;
    int rpb = (n + want - 1) / want;
    const int64_t items_row = (int64_t)C * D;
    const int rpb_min = (int)((8 * HEAT_THREADS + items_row - 1) / items_row);
    if (rpb < rpb_min) rpb = rpb_min;
    const int rpb_lds = HEAT_LDS_TARGET / ((n + 2) * 12);
    if (rpb > rpb_lds) rpb = rpb_lds;
    if (rpb > n) rpb = n;
    if (rpb > rpb_max) rpb = (int)rpb_max;
    if (rpb < 1) rpb = 1;
    const int split = (n + rpb - 1) / rpb;
    const size_t lds = (size_t)rpb * (n + 2) * 12;
    if (lds > HEAT_LDS_MAX) return MIL_ERR_UNSUPPORTED;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HeatArgs a{};
    const uintptr_t bp = reinterpret_cast<uintptr_t>(base);
    a.delta = (int)(bp & 15);
    a.base_al = base - a.delta;
    a.total = ((int64_t)a.delta + base_bytes + 15) & ~(int64_t)15;
    a.pitch = row_pitch;
    a.jstride = T;
    a.jet = jet_lut; a.vir = viridis_lut; a.out = out;
    a.S = S; a.D = D; a.n = n; a.rpb = rpb; a.C = C; a.Ht = Ht; a.Wt = Wt; a.q0 = alpha_tissue; a.q1 = alpha_map;
    a.g = inset / D;
    if (n - 2 * a.g < 1) a.g = 0;
    a.rcpD = (unsigned)(((uint64_t)1 << 32) / (uint64_t)D + 1);
    for (int done = 0; done < T; done += 65535) {               // grid.y limit
        const int m = T - done < 65535 ? T - done : 65535;
        a.win_off = reinterpret_cast<const long long*>(win_off) + done;
        a.pos = out_pos + 2 * (size_t)done;
        a.jidx = jet_idx + done;
        a.fidx = feat_idx ? feat_idx + 80 * (size_t)done : nullptr;
        if (D >= 16) hipLaunchKernelGGL(heatmap_kernel<true>, dim3(split, m), dim3(HEAT_THREADS), lds, st, a);
        else hipLaunchKernelGGL(heatmap_kernel<false>, dim3(split, m), dim3(HEAT_THREADS), lds, st, a);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}
