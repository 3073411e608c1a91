// Pillow's GaussianBlur on stacks of uint8 planes, all six box passes in one launch: the defocus augmentation of the train chain on
// `U8Tiles` and the smoothing of uint8 attribution maps; DESIGN.md section 3.52.
//
//   gaussian_blur_u8_kernel   a workgroup owns one 64 x 64 output block of one plane: it stages the block with this item's halo into
//                             LDS as bytes, runs three horizontal passes over every staged row and three vertical passes over the
//                             block's own columns between two LDS byte arrays, a barrier after each, and writes the sixth pass to
//                             global memory
//
// The byte contract (include/mil_hip.h): one pass along a line of length n is
//     out[x] = (ww * sum_{k=-r..r} in[c(x+k)] + fw * (in[c(x-r-1)] + in[c(x+r+1)]) + 2^23) >> 24,   c(i) = min(max(i, 0), n - 1)
// in uint32, three passes along W and then three along H, each reading the bytes of the one before.  There is no floating point
// here.  ww == 2^24 on an axis is the identity: that axis has no halo and no pass.
//
// Geometry.  A horizontal pass reads LDS as dwords, so its reach is E = 4 bytes per side for r <= 3 and 8 for r >= 4, a work item
// owns E consecutive outputs of one row (3 E / 4 dword reads for E outputs, a sliding sum in registers), and the halo along W is 3 E:
// pass i computes the columns [E (i + 1), Wst - E (i + 1)) of the staged width Wst = twp + 6 E, exactly what pass i + 1 reads.  A
// vertical pass reads one dword = 4 columns per row, so rows need no grid: the halo along H is 3 (r + 1) and pass i computes the rows
// [(r + 1)(i + 1), rows - (r + 1)(i + 1)).  Every LDS byte that is read was written by the staging or by the pass before.
//
// The border of the PLANE, per pass, as Pillow clamps it:
//   along W   columns staged outside the plane hold the border column's byte, and every pass keeps it so: a segment left of column 0
//             or right of column W - 1 is computed as the border's segment and takes the border output (gb_hpass)
//   along H   rows outside the plane are neither staged nor computed: a vertical read clamps its row to the plane (and to the rows
//             the pass before wrote), one v_med3 per dword
//
// LDS: two arrays of 112 rows x 29 dwords (112 staged bytes + 4: an odd pitch, so the lanes of a horizontal pass, one row each,
// hit 32 banks) = 25984 bytes static, six workgroups per CU.  The halo is this item's, so sigma <= 2 (r <= 1) stages 88 x 76 bytes.
#include "common.cuh"
#include <climits>

#define GB_THREADS 256
#define GB_TILE 64
#ifndef MIL_BLUR_U8_MAX_BOX
#define MIL_BLUR_U8_MAX_BOX 7            // include/mil_hip.h
#endif
#define GB_ROWS (GB_TILE + 6 * (MIL_BLUR_U8_MAX_BOX + 1))      // 112 staged rows / bytes per row at most
#define GB_PITCH (GB_ROWS / 4 + 1)                              // dwords
#define GB_IDENT (1 << 24)

static_assert(MIL_BLUR_U8_MAX_BOX == 7, "the pass templates cover r = 0..7");

// ww < 2^24 wherever a pass runs, fw <= 2^23, s <= 15 * 255, e <= 510: 24-bit products, and the sum stays below 2^32
__device__ __forceinline__ unsigned gb_round(unsigned ww, unsigned fw, unsigned s, unsigned e) {
    return (__umul24(ww, s) + __umul24(fw, e) + (1u << 23)) >> 24;
}

// E consecutive outputs of one row; p: the dword E bytes before the first.  Every index is a constant.
template <int E, int R>
__device__ __forceinline__ void gb_hrun(const unsigned* p, unsigned ww, unsigned fw, unsigned (&o)[E]) {
    static_assert(R < E && (E == 4 || E == 8), "the reach covers r + 1");
    unsigned b[3 * E];
#pragma unroll
    for (int q = 0; q < 3 * E / 4; ++q) {
        const unsigned d = p[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[4 * q + e] = (d >> (8 * e)) & 255u;
    }
    unsigned s = 0;
#pragma unroll
    for (int j = E - R; j <= E + R; ++j) s += b[j];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        o[m] = gb_round(ww, fw, s, b[E + m - R - 1] + b[E + m + R + 1]);
        if (m + 1 < E) s = s + b[E + m + R + 1] - b[E + m - R];
    }
}

struct GbGeom {
    int rlo, nrows;          // the staged rows that lie inside the plane: rlo .. rlo + nrows - 1
    int nsegtot;             // segments of E bytes in the staged width
    int smin, smax, lcmax;   // the segments of the plane's first and last column, and the last column, in staged coordinates
    int row0, seg0, drow, dseg;   // item tid = (seg0, row0) with the row fastest; item + 256 = (+dseg, +drow)
};

// One horizontal pass over every staged row: the segments pass + 1 .. nsegtot - pass - 2.
template <int E>
__device__ __forceinline__ void gb_hpass(const unsigned* src, unsigned* dst, int pass, int r, unsigned ww, unsigned fw, const GbGeom& g) {
    const int nseg = g.nsegtot - 2 * (pass + 1);
    int row = g.row0, seg = g.seg0;
    while (seg < nseg) {
        const int s = seg + pass + 1;
        const int se = s < g.smin ? g.smin : (s > g.smax ? g.smax : s);
        const unsigned* p = src + (g.rlo + row) * GB_PITCH + (se - 1) * (E / 4);
        unsigned o[E];
        if constexpr (E == 4) {
            switch (r) {
                case 0: gb_hrun<4, 0>(p, ww, fw, o); break;
                case 1: gb_hrun<4, 1>(p, ww, fw, o); break;
                case 2: gb_hrun<4, 2>(p, ww, fw, o); break;
                default: gb_hrun<4, 3>(p, ww, fw, o); break;
            }
        } else {
            switch (r) {
                case 4: gb_hrun<8, 4>(p, ww, fw, o); break;
                case 5: gb_hrun<8, 5>(p, ww, fw, o); break;
                case 6: gb_hrun<8, 6>(p, ww, fw, o); break;
                default: gb_hrun<8, 7>(p, ww, fw, o); break;
            }
        }
        if (g.smax < g.nsegtot) {                 // the plane's last column lies in the staged width: what follows it repeats it
#pragma unroll
            for (int j = 1; j < E; ++j)
                if (se * E + j > g.lcmax) o[j] = o[j - 1];
        }
        if (s != se) {
            const unsigned v = s < se ? o[0] : o[E - 1];
#pragma unroll
            for (int j = 0; j < E; ++j) o[j] = v;
        }
        unsigned* d = dst + (g.rlo + row) * GB_PITCH + s * (E / 4);
#pragma unroll
        for (int q = 0; q < E / 4; ++q) d[q] = o[4 * q] | (o[4 * q + 1] << 8) | (o[4 * q + 2] << 16) | (o[4 * q + 3] << 24);
        row += g.drow;
        seg += g.dseg;
        if (row >= g.nrows) {
            row -= g.nrows;
            ++seg;
        }
    }
}

// Four consecutive output rows q0 .. q0 + 3 of one dword column (4 plane columns): the even and the odd bytes of a dword are summed
// as two 16-bit lanes each (15 * 255 < 2^16).  A read row is clamped to lo .. hi.  o[m]: the four output bytes of row q0 + m.
template <int R>
__device__ __forceinline__ void gb_vrun(const unsigned* col, int q0, int lo, int hi, unsigned ww, unsigned fw, unsigned (&o)[4]) {
    constexpr int N = 2 * R + 6;
    unsigned ev[N], od[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int q = q0 - R - 1 + j;
        q = q < lo ? lo : (q > hi ? hi : q);
        const unsigned d = col[q * GB_PITCH];
        ev[j] = d & 0x00FF00FFu;
        od[j] = (d >> 8) & 0x00FF00FFu;
    }
    unsigned se = 0, so = 0;
#pragma unroll
    for (int j = 1; j <= 2 * R + 1; ++j) {
        se += ev[j];
        so += od[j];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const unsigned ee = ev[m] + ev[m + 2 * R + 2], eo = od[m] + od[m + 2 * R + 2];
        o[m] = gb_round(ww, fw, se & 0xFFFFu, ee & 0xFFFFu) | (gb_round(ww, fw, so & 0xFFFFu, eo & 0xFFFFu) << 8) |
               (gb_round(ww, fw, se >> 16, ee >> 16) << 16) | (gb_round(ww, fw, so >> 16, eo >> 16) << 24);
        if (m < 3) {
            se = se + ev[m + 2 * R + 2] - ev[m + 1];
            so = so + od[m + 2 * R + 2] - od[m + 1];
        }
    }
}

__device__ __forceinline__ void gb_vrun_r(int r, const unsigned* col, int q0, int lo, int hi, unsigned ww, unsigned fw, unsigned (&o)[4]) {
    switch (r) {
        case 0: gb_vrun<0>(col, q0, lo, hi, ww, fw, o); break;
        case 1: gb_vrun<1>(col, q0, lo, hi, ww, fw, o); break;
        case 2: gb_vrun<2>(col, q0, lo, hi, ww, fw, o); break;
        case 3: gb_vrun<3>(col, q0, lo, hi, ww, fw, o); break;
        case 4: gb_vrun<4>(col, q0, lo, hi, ww, fw, o); break;
        case 5: gb_vrun<5>(col, q0, lo, hi, ww, fw, o); break;
        case 6: gb_vrun<6>(col, q0, lo, hi, ww, fw, o); break;
        default: gb_vrun<7>(col, q0, lo, hi, ww, fw, o); break;
    }
}

// Four bytes of output row y at column x: one dword where they lie inside the plane on the 4-byte grid, byte by byte otherwise.
__device__ __forceinline__ void gb_store(uint8_t* op, int y, int x, int W, unsigned v) {
    uint8_t* d = op + (size_t)y * W + x;
    if (x + 3 < W && !(reinterpret_cast<uintptr_t>(d) & 3)) {
        *reinterpret_cast<unsigned*>(d) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x + e < W) d[e] = (uint8_t)(v >> (8 * e));
    }
}

__global__ __launch_bounds__(GB_THREADS) void gaussian_blur_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                     const int* __restrict__ params, int planes_per_item, int H, int W,
                                                                     int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) unsigned gb_lds[2][GB_ROWS * GB_PITCH];
    MIL_POISON_STATIC(gb_lds);
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, plane = b / tiles_y;
    const int x0 = tx * GB_TILE, y0 = ty * GB_TILE;
    const int tw = W - x0 < GB_TILE ? W - x0 : GB_TILE, th = H - y0 < GB_TILE ? H - y0 : GB_TILE;
    const int twp = (tw + 7) & ~7;
    const uint8_t* xp = in + (size_t)plane * H * W;
    uint8_t* op = out + (size_t)plane * H * W;

    // this item's six integers; r is forced into 0..7 whatever the array holds (the host layer checks the ranges): the halo, and
    // with it every LDS index below, then stays inside the arrays
    const int* pp = params + 6 * (plane / planes_per_item);
    int rx = pp[0], ry = pp[3];
    const unsigned wwx = (unsigned)pp[1], fwx = (unsigned)pp[2], wwy = (unsigned)pp[4], fwy = (unsigned)pp[5];
    rx = rx < 0 ? 0 : (rx > MIL_BLUR_U8_MAX_BOX ? MIL_BLUR_U8_MAX_BOX : rx);
    ry = ry < 0 ? 0 : (ry > MIL_BLUR_U8_MAX_BOX ? MIL_BLUR_U8_MAX_BOX : ry);
    const bool idx_x = wwx == (unsigned)GB_IDENT, idx_y = wwy == (unsigned)GB_IDENT;
    const int E = idx_x ? 0 : (rx <= 3 ? 4 : 8), HX = 3 * E;
    const int hy = idx_y ? 0 : 3 * (ry + 1);
    const int wst = twp + 2 * HX, rows = th + 2 * hy;              // staged bytes per row (<= 112), staged rows (<= 112)
    // staged row q is the plane's row y0 - hy + q, staged column lc its column x0 - HX + lc
    const int lrmin = hy - y0, lrmax = hy + (H - 1 - y0);
    const int rlo = lrmin > 0 ? lrmin : 0, rhi = lrmax < rows - 1 ? lrmax : rows - 1;
    const int nrows = rhi - rlo + 1;

    unsigned* cur = gb_lds[0];
    unsigned* nxt = gb_lds[1];

    // staging: 32 lanes per row, one dword each
    const int nq = wst >> 2;
    for (int idx = tid; idx < nrows * 32; idx += GB_THREADS) {
        const int q = idx & 31, row = rlo + (idx >> 5);
        if (q >= nq) continue;
        const uint8_t* rowp = xp + (size_t)(y0 - hy + row) * W;
        const int gx = x0 - HX + 4 * q;
        unsigned d;
        if (gx >= 0 && gx + 3 < W && !(reinterpret_cast<uintptr_t>(rowp + gx) & 3)) {
            d = *reinterpret_cast<const unsigned*>(rowp + gx);
        } else {
            d = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int c = gx + e;
                c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
                d |= (unsigned)rowp[c] << (8 * e);
            }
        }
        cur[row * GB_PITCH + q] = d;
    }
    __syncthreads();

    if (!idx_x) {
        GbGeom g;
        g.rlo = rlo;
        g.nrows = nrows;
        g.nsegtot = wst / E;
        g.smin = x0 == 0 ? 3 : 0;
        g.lcmax = HX + (W - 1 - x0);
        g.smax = g.lcmax / E;
        g.row0 = tid % nrows;
        g.seg0 = tid / nrows;
        g.drow = GB_THREADS % nrows;
        g.dseg = GB_THREADS / nrows;
        for (int pass = 0; pass < 3; ++pass) {
            if (E == 4) gb_hpass<4>(cur, nxt, pass, rx, wwx, fwx, g);
            else gb_hpass<8>(cur, nxt, pass, rx, wwx, fwx, g);
            unsigned* t = cur;
            cur = nxt;
            nxt = t;
            __syncthreads();
        }
    }

    const int cd = tid & 15, ncd = twp >> 2;
    const unsigned* col = cur + (HX >> 2) + cd;
    if (idx_y) {                                                   // hy == 0: the staged rows are the block's own
        for (int row = tid >> 4; row < th; row += GB_THREADS / 16)
            if (cd < ncd) gb_store(op, y0 + row, x0 + 4 * cd, W, col[row * GB_PITCH]);
        return;
    }
    int lo = rlo, hi = rhi;                                        // the rows of `cur` that hold the pass before
    for (int pass = 0; pass < 3; ++pass) {
        const int a = (ry + 1) * (pass + 1);
        const int wlo = a > rlo ? a : rlo, whi = rows - a - 1 < rhi ? rows - a - 1 : rhi;      // the rows this pass writes
        for (int q0 = wlo + 4 * (tid >> 4); q0 <= whi; q0 += 4 * (GB_THREADS / 16)) {
            if (cd >= ncd) continue;
            unsigned o[4];
            gb_vrun_r(ry, col, q0, lo, hi, wwy, fwy, o);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (q0 + m > whi) continue;
                if (pass < 2) nxt[(q0 + m) * GB_PITCH + (HX >> 2) + cd] = o[m];
                else gb_store(op, y0 - hy + q0 + m, x0 + 4 * cd, W, o[m]);
            }
        }
        if (pass == 2) break;
        unsigned* t = cur;
        cur = nxt;
        nxt = t;
        col = cur + (HX >> 2) + cd;
        lo = wlo;
        hi = whi;
        __syncthreads();
    }
}

// include/mil_hip.h has the contract.  Every status but MIL_ERR_LAUNCH is decided here, before any GPU call; `params` lies in
// device memory and is not read here.
extern "C" int mil_gaussian_blur_u8(const uint8_t* in, uint8_t* out, const int32_t* params, int planes, int planes_per_item, int H, int W,
                                    void* stream) {
    if (!in || !out || !params || planes < 0 || planes_per_item < 1 || H < 1 || W < 1) return MIL_ERR_ARG;
    if (planes % planes_per_item) return MIL_ERR_ARG;
    const unsigned long long hw = (unsigned long long)H * W;
    const unsigned long long tiles = (unsigned long long)((W + GB_TILE - 1) / GB_TILE) * (unsigned long long)((H + GB_TILE - 1) / GB_TILE);
    // a plane as large as the stain kernels take, a grid that fits an int
    if (planes > 0 && (hw > 0x7fffffffull - 4096 || tiles * (unsigned long long)planes > (unsigned long long)INT_MAX)) return MIL_ERR_UNSUPPORTED;
    if (mil_overlap(out, in, (unsigned long long)planes * hw)) return MIL_ERR_ARG;
    if (planes == 0) return MIL_OK;
    const int tiles_x = (W + GB_TILE - 1) / GB_TILE, tiles_y = (H + GB_TILE - 1) / GB_TILE;
    hipLaunchKernelGGL(gaussian_blur_u8_kernel, dim3((unsigned)(tiles * planes)), dim3(GB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), in, out,
                       params, planes_per_item, H, W, tiles_x, tiles_y);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
