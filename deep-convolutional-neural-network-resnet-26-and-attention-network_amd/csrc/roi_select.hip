// Tissue selection on the device: the statistics the reference's RoiBuilder.build() loop (RoiBuilder.py:156-169) takes of
// every roi_size window of a whole-slide image — ImageStat.Stat(roi).stddev[0] (from sum R and sum R^2) and the number of
// pixels with h > 120, 50 < v < 210 of roi.convert('HSV') — as exact integers, so that the keep / reject decision made from
// them on the host (mil_amd.RoiSelector) is bit for bit the reference's.
//
// Hue without a division: Pillow's rgb2hsv_row computes h = (int)(fmod(hh / 6 + 1, 1) * 255) from float32 rc, gc, bc.  With
// mx / mn the largest / smallest channel, d = mx - mn and
//     num = g - b            if r == mx
//         = 2d + (b - r)     else if g == mx          (Pillow's branch order)
//         = 4d + (r - g)     otherwise,               num += 6d if num < 0,
// hh / 6 + 1 is num / (6d) + 1 and, over all 2^24 colours, h > 120 <=> d > 0 and 255 num >= 726 d (0 mismatches against Pillow
// 12.2.0; tests/test_cpu_roi_select.py repeats the comparison where Pillow is installed).  726 = (120 + 1) * 6: the kernel
// keeps the threshold general as (hue_min + 1) * 6, the exhaustive check pins 120.  v = mx.
//
// Layout of the work.  Window t is S rows of 3S bytes; row y starts at byte win_off[t] + y * row_pitch of the source, at ANY
// byte alignment (a slide's pitch 3W and a window's 3 * col are multiples of neither 4 nor 16).  A row is cut into 48-byte
// chunks on the 16-byte grid of the SOURCE: chunk c of a row that starts al bytes (0..15) behind a grid point is the bytes
// [48c, 48c + 48) counted from that grid point.  48 = 16 pixels = three aligned 16-byte loads, so the pixels that START in a
// chunk sit at the same byte phase p = al % 3 in every chunk of the row, and sixteen of them start in every chunk: a lane
// loads its 48 bytes once, takes the two bytes its last pixel may reach into the next chunk from the next lane's registers
// (the next lane holds the next chunk: work items are numbered row-major over (row, chunk); lane 63 loads that dword itself),
// funnel-shifts by p and has its 16 pixels at compile-time byte positions.  Head and tail of a row: pixel j of chunk c is
// pixel 16c - al / 3 + j of the row; every lane carries the 16-bit mask of its pixels that lie in [0, S) — all ones except in
// the first chunk of a row (when al >= 3) and the last one — and a pixel outside the mask is not counted, whatever its bytes.
// Chunks that hold no byte of the row are not loaded.
//
// A workgroup takes rows [y0, y0 + rpb) of one window: the host chooses rpb by n so that a bag of a few dozen windows still
// covers the chip.  Every load goes through a buffer descriptor that starts at the grid point below the workgroup's first row
// and ends with the source (rounded up to the 16-byte grid, so that the last, partial granule of a source whose size is no
// multiple of 16 is still delivered: a granule never crosses a page; its bytes outside the source belong to no pixel of a
// window that lies inside the source).  Offsets are 32-bit: rpb * row_pitch stays below 2 GiB (host).  An offset outside
// the descriptor returns zeros, and a zero pixel adds nothing to any of the three sums (r = 0, d = 0).
//
// Sums: per work item (16 pixels) in 32 bits (sum R^2 <= 16 * 255^2), then per lane in 64 bits — no 32-bit partial sum can
// overflow at any S.  Wave shuffle, four partials in LDS, three 64-bit vector atomics per workgroup into out[t] (zeroed by the
// entry point on the same stream).  Integer sums: the result does not depend on the order.
#include "pf_common.cuh"

#define ROI_MAX_S 4096
#define ROI_THREADS 256

struct RoiArgs {
    const uint8_t* base_al;         // source pointer rounded down to the 16-byte grid
    const long long* win_off;       // [n] byte offset of each window's first pixel from the (unrounded) source pointer
    long long* out;                 // [n,4]
    long long total;                // bytes from base_al to the grid point at or behind the end of the source
    long long pitch;                // bytes between two rows of a window
    int delta;                      // source pointer - base_al (0..15)
    int S, rpb, C, hue_k, v_min, v_max;     // C: chunks per row (upper bound over alignments); hue_k = (hue_min + 1) * 6
};

__device__ __forceinline__ unsigned roi_byte(const unsigned (&e)[12], int b) { return (e[b >> 2] >> ((b & 3) * 8)) & 0xffu; }

// sums of one chunk's 16 pixels (e: its 48 bytes from the first pixel start on), of which those with their bit set in m count
__device__ __forceinline__ void roi_chunk(const unsigned (&e)[12], unsigned m, int hue_k, int v_min, int v_max,
                                          unsigned& s1, unsigned& s2, unsigned& cnt) {
    s1 = 0; s2 = 0; cnt = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int r = (int)roi_byte(e, 3 * j), g = (int)roi_byte(e, 3 * j + 1), b = (int)roi_byte(e, 3 * j + 2);
        const int mx = max(r, max(g, b)), mn = min(r, min(g, b)), d = mx - mn;
        // all three candidates, then two selects (no branch per pixel); 255 num >= k d as 256 num >= k d + num (no 32-bit multiply)
        const int n_r = g - b, n_g = 2 * d + (b - r), n_b = 4 * d + (r - g);
        const int is_r = -(int)(r == mx), is_g = -(int)(g == mx);
        int num = (n_r & is_r) | (~is_r & ((n_g & is_g) | (n_b & ~is_g)));
        num += (num >> 31) & (6 * d);
        const bool pass = (d > 0) & ((num << 8) >= __mul24(hue_k, d) + num) & (mx > v_min) & (mx < v_max);
        const unsigned ok = 0u - ((m >> j) & 1u);                   // all ones / zero
        const unsigned rr = (unsigned)r & ok;
        s1 += rr; s2 += __umul24(rr, rr); cnt += pass ? ok & 1u : 0u;
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // four pixels (three dwords) at a time: keeps the live set small
    }
}

__device__ __forceinline__ unsigned long long roi_wave_sum(unsigned long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, s), hi = __shfl_xor((unsigned)(v >> 32), s);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(ROI_THREADS) void roi_stats_kernel(RoiArgs a) {
    __shared__ unsigned long long red[ROI_THREADS / 64][4];
    MIL_POISON_STATIC(red);
    const int tid = threadIdx.x, lane = tid & 63, t = blockIdx.y;
    const int S = a.S, C = a.C, y0 = blockIdx.x * a.rpb;
    const int rows = min(a.rpb, S - y0);
    if (blockIdx.x == 0 && tid == 0) a.out[4 * (size_t)t + 3] = (long long)S * S;
    if (rows <= 0) return;

    // descriptor of this workgroup: from the grid point below its first row to the end of the source
    const long long woff = a.win_off[t];
    const long long r0 = (long long)a.delta + woff + (long long)y0 * a.pitch;
    const long long B = r0 & ~15ll;
    const long long left = a.total - B;
    const unsigned range = (woff < 0 || left <= 0) ? 0u : (left > 0x80000000ll ? 0x80000000u : (unsigned)left);
    const __amdgpu_buffer_rsrc_t rs = mil_rsrc(a.base_al + B, range);
    const unsigned rel0 = (unsigned)(r0 - B), pitch = (unsigned)a.pitch;
    const int row_bytes = 3 * S;

    // work items (row, chunk), row-major: this thread takes items tid, tid + 256, ... — walked with carries
    int yr = tid / C, c = tid - yr * C;
    const int dy = ROI_THREADS / C, dc = ROI_THREADS - dy * C;
    const int nit = (rows * C + ROI_THREADS - 1) / ROI_THREADS;

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

    unsigned long long acc1 = 0, acc2 = 0;
    unsigned accn = 0;
    for (int it = 0; it < nit; ++it) {
        unsigned d[13];
#pragma unroll
        for (int i = 0; i < 12; ++i) d[i] = q[i >> 2][i & 3];
        const unsigned nxt = __shfl_down(d[0], 1);
        d[12] = !live ? 0u : lane == 63 ? own : nxt;    // a chunk without bytes of the row stays all zeros: it adds nothing
        // valid pixels of this chunk: j in [jlo, jhi) with row pixel k0 + j in [0, S)
        const int k0 = 16 * c - (int)(al / 3u);
        const unsigned p = al % 3u;
        const int jlo = min(max(-k0, 0), 16), jhi = min(max(S - k0, 0), 16);
        const unsigned m = jhi > jlo ? ((1u << jhi) - 1u) & ~((1u << jlo) - 1u) : 0u;

        yr += dy; c += dc;
        if (c >= C) { c -= C; ++yr; }
        if (it + 1 < nit) fetch();                      // the next item's bytes travel while this one is summed

        unsigned e[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) e[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], p);
        unsigned s1, s2, cnt;
        roi_chunk(e, m, a.hue_k, a.v_min, a.v_max, s1, s2, cnt);
        acc1 += s1; acc2 += s2; accn += cnt;
    }

    acc1 = roi_wave_sum(acc1); acc2 = roi_wave_sum(acc2);
    const unsigned long long accc = roi_wave_sum((unsigned long long)accn);
    if (lane == 0) { red[tid >> 6][0] = acc1; red[tid >> 6][1] = acc2; red[tid >> 6][2] = accc; }
    __syncthreads();
    if (tid < 3) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < ROI_THREADS / 64; ++w) v += red[w][tid];
        atomicAdd(reinterpret_cast<unsigned long long*>(a.out) + 4 * (size_t)t + tid, v);
    }
}

// out[t] = (sum R, sum R^2, #{h > hue_min, v_min < v < v_max}, S^2) of window t (RoiBuilder.py:156-169).  Everything that can
// be refused is refused here, on the host, before any GPU call.
extern "C" int mil_roi_stats(const uint8_t* base, int64_t base_bytes, const int64_t* win_off, int64_t row_pitch, int n, int S,
                             int hue_min, int v_min, int v_max, int64_t* out, void* stream) {
    if (!base || !win_off || !out || base_bytes < 0 || n < 0 || S < 1 || hue_min < 0 || hue_min > 255) return MIL_ERR_ARG;
    if (S > ROI_MAX_S) return MIL_ERR_UNSUPPORTED;
    if (row_pitch < 3 * (int64_t)S) return MIL_ERR_ARG;
    const int C = (3 * S + 15 + 47) / 48;
    // 32-bit offsets inside a workgroup's descriptor: rows * pitch + one row of chunks below 2 GiB
    const int64_t rpb_max = ((int64_t)0x7fff0000 - 48 * (int64_t)C) / row_pitch;
    if (rpb_max < 1) return MIL_ERR_UNSUPPORTED;
    if (n == 0) return MIL_OK;

    // rows per workgroup: about 4096 workgroups in the launch (16 per CU), but at least ~8 work items per thread
    const int want = (4096 + n - 1) / n;
    int rpb = (S + want - 1) / want;
    const int rpb_min = (8 * ROI_THREADS + C - 1) / C;
    if (rpb < rpb_min) rpb = rpb_min;
    if (rpb > S) rpb = S;
    if (rpb > rpb_max) rpb = (int)rpb_max;
    const int split = (S + rpb - 1) / rpb;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, (size_t)n * 4 * sizeof(int64_t), st) != hipSuccess) return MIL_ERR_LAUNCH;
    RoiArgs a{};
    const uintptr_t bp = reinterpret_cast<uintptr_t>(base);
    a.delta = (int)(bp & 15);
    a.base_al = base - a.delta;
    a.total = ((int64_t)a.delta + base_bytes + 15) & ~(int64_t)15;
    a.pitch = row_pitch;
    a.S = S; a.rpb = rpb; a.C = C; a.hue_k = (hue_min + 1) * 6; a.v_min = v_min; a.v_max = v_max;
    for (int done = 0; done < n; done += 65535) {               // grid.y limit
        const int m = n - done < 65535 ? n - done : 65535;
        a.win_off = reinterpret_cast<const long long*>(win_off) + done;
        a.out = reinterpret_cast<long long*>(out) + 4 * (size_t)done;
        hipLaunchKernelGGL(roi_stats_kernel, dim3(split, m), dim3(ROI_THREADS), 0, st, a);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}
